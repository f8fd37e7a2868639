"""Region decode: only the tiles a crop rectangle touches (include/xpng_hip.h "region decode", include/xpng_region.h).

CPU: the tile selection against the oracle's tile table, the host-only forms of xpng_load_region (level 7, whole-image single
colour), and the rejection of invalid rectangles.  GPU (-m gpu): crops of the reference-written corpus goldens, one batched
launch with a different rectangle per image at a padded row pitch, and a file whose unselected tiles are corrupt."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from _kit import built, gpu, po
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(4096, 4096), (16384, 16384), (1500, 1200), (445, 444), (300, 4000), (3799, 1927), (100, 100)]


def rect_set(W, H, tiles, seed=0, n_random=24):
    """full image; a pixel at every tile corner; rects ending on a tile boundary and one pixel past it; one-pixel rows and
    columns across every tile row / column; seeded random rects"""
    rects = [(0, 0, W, H)]
    for (x, y, w, h) in tiles:
        for (cx, cy) in ((x, y), (x + w - 1, y), (x, y + h - 1), (x + w - 1, y + h - 1)):
            rects.append((cx, cy, 1, 1))
        ex, ey = x + w, y + h
        rects.append((x, y, w, h))                                    # exactly the tile
        rects.append((0, 0, ex, ey))                                  # ends on the tile's bottom-right boundary
        if ex < W:
            rects.append((x, y, w + 1, h))                            # one pixel past it (right)
        if ey < H:
            rects.append((x, y, w, h + 1))                            # (down)
        if x > 0:
            rects.append((x - 1, y, 1, 1))                            # the last pixel left of the boundary
    for y in sorted({t[1] for t in tiles}):
        rects.append((0, y, W, 1))
    for x in sorted({t[0] for t in tiles}):
        rects.append((x, 0, 1, H))
    rng = random.Random(seed * 1_000_003 + W * 31 + H)
    for _ in range(n_random):
        w = rng.randint(1, min(W, 700))
        h = rng.randint(1, min(H, 700))
        rects.append((rng.randint(0, W - w), rng.randint(0, H - h), w, h))
    return list(dict.fromkeys(rects))


def invalid_rects(W, H):
    big = (1 << 64) - 1
    return [(0, 0, 0, 1), (0, 0, 1, 0), (W, 0, 1, 1), (0, H, 1, 1), (W - 1, 0, 2, 1), (0, H - 1, 1, 2), (0, 0, W + 1, H),
            (0, 0, W, H + 1), (big, 0, 2, 1), (1, 0, big, 1), (0, 1, 1, big)]


def intersecting(tiles, rect):
    t = np.asarray(tiles, dtype=np.int64)
    x, y, w, h = rect
    hit = (t[:, 0] < x + w) & (x < t[:, 0] + t[:, 2]) & (t[:, 1] < y + h) & (y < t[:, 1] + t[:, 3])
    return [int(i) for i in np.nonzero(hit)[0]]


def test_region_tiles_match_the_oracle_tile_table(po):
    for (W, H) in GEOMETRIES:
        tiles = po.tile_table(W, H, 4)
        rects = rect_set(W, H, tiles)
        if len(rects) > 3000:  # (16384^2: keep every structured rect of a sample of tiles, all the random ones)
            rects = rects[:1] + rects[1:-24:3] + rects[-24:]
        for r in rects:
            assert api.region_tiles(W, H, r) == intersecting(tiles, r), (W, H, r)
        assert api.region_tiles(W, H, (0, 0, W, H)) == list(range(len(tiles)))
        for r in invalid_rects(W, H):
            arr = (C.c_uint32 * len(tiles))()
            assert api.hip_lib().xpnghip_region_tiles(W, H, (C.c_uint64 * 4)(*r), arr, len(tiles)) == -1, (W, H, r)
        # cap too small
        if len(tiles) > 1:
            arr = (C.c_uint32 * 1)()
            assert api.hip_lib().xpnghip_region_tiles(W, H, (C.c_uint64 * 4)(0, 0, W, H), arr, 1) == -1


def test_region_header_is_exported_by_the_host_library():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpng_region.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(xpng_\w*)\s*\(", txt)))
    assert names == sorted(api.HOST_EXT_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.HOST_SO], text=True)
    ex = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(names) <= ex


def _host_only_files(po, tmp_path):
    from xpng_amd.synth import synth_raster
    files = []
    for (W, H, alpha) in [(1500, 1200, False), (445, 444, True), (300, 700, True)]:
        r = synth_raster("photo", W, H, alpha, seed=W)
        p = tmp_path / f"l7_{W}x{H}_{int(alpha)}.xpng"
        p.write_bytes(po.encode_image(7, r))
        files.append((p, W, H))
    flat = synth_raster("flat", 1000, 900, False)
    data = po.encode_image(2, flat)
    assert len(data) == 11                                     # the whole-image single-colour file of level 2
    p = tmp_path / "single.xpng"
    p.write_bytes(data)
    files.append((p, 1000, 900))
    return files


def test_load_region_host_only_forms_equal_the_oracle_crop(po, tmp_path):
    for (p, W, H) in _host_only_files(po, tmp_path):
        full = po.decode_image(p.read_bytes())
        assert full.shape[:2] == (H, W)
        rects = rect_set(W, H, po.tile_table(W, H, full.shape[2]), n_random=16)
        for (x, y, w, h) in rects[::max(1, len(rects) // 80)]:
            got = api.load_region(str(p), x, y, w, h)
            assert got.shape == (h, w, full.shape[2]) and np.array_equal(got, full[y:y + h, x:x + w]), (p.name, x, y, w, h)


def test_load_region_rejects_invalid_rects(po, tmp_path):
    L = api.host_lib()
    for (p, W, H) in _host_only_files(po, tmp_path):
        for (x, y, w, h) in invalid_rects(W, H):
            pm = api.XpngT()
            assert L.xpng_load_region(str(p).encode(), x, y, w, h, C.byref(pm)) == 1, (p.name, x, y, w, h)
            with pytest.raises(api.XpngError):
                api.load_region(str(p), x, y, w, h)
    pm = api.XpngT()
    assert L.xpng_load_region(str(tmp_path / "missing.xpng").encode(), 0, 0, 1, 1, C.byref(pm)) == 1


def test_decode_region_rejects_invalid_rects_before_device_work(po):
    """An invalid rectangle fails with a message and writes nothing, with or without a GPU."""
    from xpng_amd.synth import synth_raster
    W, H = 1500, 1200
    blobs = po.encode_tiles(1, synth_raster("photo", W, H, False))
    lib = api.hip_lib()
    buf = np.frombuffer(blobs, dtype=np.uint8)
    for r in invalid_rects(W, H):
        out = np.full(64, 0xA5, dtype=np.uint8)
        rc = lib.xpnghip_decode_region(1, buf.ctypes.data_as(C.c_void_p), len(blobs), W, H, 3, (C.c_uint64 * 4)(*r),
                                       out.ctypes.data_as(C.c_void_p))
        assert rc != 0 and "region" in api._err(), r
        assert (out == 0xA5).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["XPNG_WIDE_RANS", "XPNG_NARROW_RANS"])
def test_corpus_regions_equal_the_oracle_crop(gpu, po, manifest, monkeypatch, form):
    """Every reference-written level-1 / level-2 corpus golden (mode-2 gray, single-colour and raw tiles among them), cropped
    over the rect set of test_region_tiles_match_the_oracle_tile_table: load_region and decode_region equal the oracle's
    full decode, cropped."""
    from conftest import GOLD, corpus_entries
    monkeypatch.setenv(form, "1")
    done = 0
    for name, ent in corpus_entries(manifest):
        for level in (1, 2):
            path = os.path.join(GOLD, ent[f"L{level}"]["file"])
            data = open(path, "rb").read()
            full = po.decode_image(data)
            H, W, ch = full.shape
            mode = data[3]
            # (a level-7 file and the whole-image single-colour file of level 2 carry no tile body: load_region only)
            tile_body = mode in (1, 2) and not (len(data) == 11 + (ch == 4) and data[7] & 2)
            rects = rect_set(W, H, po.tile_table(W, H, ch), seed=level)
            for k, (x, y, w, h) in enumerate(rects):
                if k % 2 == 0 or not tile_body:
                    got = gpu.load_region(path, x, y, w, h)
                else:
                    got = gpu.decode_region(mode, data[8:], W, H, ch, (x, y, w, h))
                assert np.array_equal(got, full[y:y + h, x:x + w]), (name, level, form, (x, y, w, h))
                done += 1
    assert done > 17 * 2 * 20


def _batch_rects(W, H, n, seed):
    rng = random.Random(seed)
    rects = [(17, 29, 224, 224), (0, 0, W, H), (444 + 100 - 112, 444 + 100 - 112, 224, 224), (W - 224, H - 224, 224, 224)]
    while len(rects) < n:
        w, h = (224, 224) if len(rects) % 3 else (rng.randint(1, 600), rng.randint(1, 600))
        rects.append((rng.randint(0, W - w), rng.randint(0, H - h), w, h))
    return rects


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha,walk", [(1, True, "device"), (1, False, "host"), (2, False, "device")])
def test_batched_regions_at_a_padded_pitch(gpu, po, mode, alpha, walk):
    """One decode_region_batch launch over 48 distinct 4096^2 rasters, a different rectangle per image (one inside tile 0, the
    biggest; one the whole image): every crop equals the oracle's decode, cropped; every pitch-padding and tail byte of the
    0xA5-filled outputs is untouched; the launch's status is 0."""
    import torch
    from xpng_amd.api import walk_tile_offsets
    from xpng_amd.synth import synth_raster_torch
    W = H = 4096
    B, ch = 48, 4 if alpha else 3
    ctx = gpu.Context(W, H, ch, batch=B)
    try:
        d_r = [synth_raster_torch("photo", W, H, alpha, seed=100 * mode + b + 1) for b in range(B)]
        d_b = [torch.empty(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
        lens = ctx.encode_device_batch(mode, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
        del d_r
        torch.cuda.synchronize()
        rects = _batch_rects(W, H, B, seed=mode * 7 + ch)
        assert len(set(rects)) == B
        out_bpr = max(r[2] for r in rects) * ch + 64
        tail = 256
        d_o = [torch.full((r[3] * out_bpr + tail,), 0xA5, dtype=torch.uint8, device="cuda") for r in rects]
        blobs = [d_b[b][: lens[b]].cpu().numpy().tobytes() for b in range(B)]
        offs = [walk_tile_offsets(bl, ctx.n_tiles)[0] for bl in blobs] if walk == "host" else None
        torch.cuda.synchronize()
        ctx.decode_region_batch(mode, [t.data_ptr() for t in d_b], lens, rects, [t.data_ptr() for t in d_o], out_bpr,
                                tile_offs=offs)
        assert ctx.decode_status() == 0
        torch.cuda.synchronize()
        for b, (x, y, w, h) in enumerate(rects):
            want = po.decode_tiles(mode, blobs[b], W, H, ch)[y:y + h, x:x + w]
            got = d_o[b].cpu().numpy()
            rows = got[: h * out_bpr].reshape(h, out_bpr)
            assert np.array_equal(rows[:, : w * ch].reshape(h, w, ch), want), (mode, alpha, b, rects[b])
            assert (rows[:, w * ch:] == 0xA5).all() and (got[h * out_bpr:] == 0xA5).all(), (mode, alpha, b, "padding written")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_region_decode_never_reads_the_other_tiles(gpu, po, mode):
    """Every tile the rectangle does not touch gets type byte 0x7F (both parsers reject it; its 24-bit size word stays, so the
    size walk still finds every tile): a full decode of that file reports a rejected tile, a region decode of the rectangle
    reports none and equals the oracle's crop of the original file."""
    import torch
    from xpng_amd.api import walk_tile_offsets
    from xpng_amd.synth import special_cases, synth_raster
    if mode == 1:
        raster = synth_raster("photo", 1500, 1200, True, seed=5)
    else:
        raster = dict(special_cases())["mixed_tiles"]
    H, W, ch = raster.shape
    blobs = po.encode_tiles(mode, raster)
    ctx = gpu.Context(W, H, ch)
    try:
        off, end = walk_tile_offsets(blobs, ctx.n_tiles)
        assert end == len(blobs)
        for rect in [(400, 380, 130, 150), (0, 0, 10, 10), (W - 5, H - 300, 5, 300)]:
            keep = set(api.region_tiles(W, H, rect))
            assert 0 < len(keep) < ctx.n_tiles
            bad = bytearray(blobs)
            for t in range(ctx.n_tiles):
                if t not in keep:
                    bad[off[t] + 3] = 0x7F          # top byte of the tile's first little-endian word
            bad = bytes(bad)
            d_b = torch.from_numpy(np.frombuffer(bad + b"\0" * 64, dtype=np.uint8).copy()).cuda()
            d_full = torch.zeros(H * W * ch + 64, dtype=torch.uint8, device="cuda")
            ctx.decode_device(mode, d_b.data_ptr(), len(bad), off, d_full.data_ptr())
            assert ctx.decode_status() == 1
            x, y, w, h = rect
            d_o = torch.full((h * w * ch,), 0xA5, dtype=torch.uint8, device="cuda")
            ctx.decode_region_batch(mode, [d_b.data_ptr()], [len(bad)], [rect], [d_o.data_ptr()], w * ch)
            assert ctx.decode_status() == 0
            want = po.decode_tiles(mode, blobs, W, H, ch)[y:y + h, x:x + w]
            assert np.array_equal(d_o.cpu().numpy().reshape(h, w, ch), want), (mode, rect)
            assert np.array_equal(gpu.decode_region(mode, bad, W, H, ch, rect), want), (mode, rect)
    finally:
        ctx.close()
