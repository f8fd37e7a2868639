"""Layouts: decode into and encode from planar, BGR and 3/4-channel device buffers (include/xpng_hip.h XPNGHIP_LAYOUT_*,
xpnghip_decode_varsize_device_batch_as, xpnghip_encode_varsize_device_batch_from; xpng_amd/tensors.py load_files).

The checker is the oracle's decode or encode and a numpy rearrangement (transpose, channel flip, alpha pad or strip); every
comparison is bit-exact.  CPU: the symbols, the layout word, argument failures that need no device, and load_files on the kinds
of file it answers from the host bytes.  GPU (-m gpu): every layout word on batches whose widths cover every row and plane-row
alignment, inside sentinel-filled buffers at shifted offsets; the decode status; the encode from every layout; a round trip in
both orders; misuse; load_files on the reference-written goldens."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _kit
from _kit import FORMATS, GUARD, SENTINEL, _offsets, _upload, arrange, built, gpu, po
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_layout_channels", "xpnghip_decode_varsize_device_batch_as", "xpnghip_encode_varsize_device_batch_from"]
# one tile across and two (445 x 444, 889 x 445), a tall and a wide image; 701 x 300 makes the staging pitch wider than every other row
COMMON_DIMS = [(17, 4), (64, 64), (445, 444), (889, 445), (100, 1100), (701, 300)]
RGB_DIMS = [(w, h) for w in range(1, 9) for h in range(1, 10)] + COMMON_DIMS   # rows and plane rows at every alignment, shorter than a dword
RGBA_DIMS = [(4, 4), (5, 7), (6, 5), (7, 4)] + COMMON_DIMS
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]
Arena = functools.partial(_kit.Arena, phases=4)                  # buffer i starts LEAD + i % 4 bytes into its region; GUARD bytes behind it


def arrange_word(r, word):
    return arrange(r, bool(word & 1), bool(word & 2), (word >> 8) or r.shape[2])


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_layout_symbols_are_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpng_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(xpnghip_\w*)\s*\(", txt))
    assert set(NEW) <= names and set(NEW) <= set(api.HIP_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.HIP_SO], text=True)
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for macro, value in (("PLANAR", 0x001), ("BGR", 0x002), ("C3", 0x300), ("C4", 0x400)):
        assert re.search(r"#define\s+XPNGHIP_LAYOUT_%s\s+0x%03xu" % (macro, value), txt), macro
    import xpng_amd
    for name in ("layout", "layout_channels"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert hasattr(api.MixedContext, "decode_batch_as") and hasattr(api.MixedContext, "encode_batch_from")
    assert api.hip_lib().xpnghip_abi_version() == 2


def test_layout_channels_of_every_word():
    lib = api.hip_lib()
    assert len(set(WORDS)) == 12
    for word in WORDS:
        for pxsz in (3, 4):
            want = (word >> 8) or pxsz
            assert lib.xpnghip_layout_channels(word, pxsz) == want == api.layout_channels(word, pxsz), (hex(word), pxsz)
        for pxsz in (2, 5, 0, -1):
            assert lib.xpnghip_layout_channels(word, pxsz) == -1, (hex(word), pxsz)
    for bad in (0x004, 0x008, 0x080, 0x1000, 0x80000000, 0x100, 0x200, 0x500, 0xF00, 0x304):
        for pxsz in (3, 4):
            assert lib.xpnghip_layout_channels(bad, pxsz) == -1, hex(bad)
        with pytest.raises(api.XpngError):
            api.layout_channels(bad, 3)
    assert api.layout() == 0 and api.layout(planar=True) == 1 and api.layout(bgr=True) == 2
    assert api.layout(True, True, 3) == 0x303 and api.layout(channels=4) == 0x400
    for ch in (2, 1, 5, 15):
        with pytest.raises(api.XpngError):
            api.layout(channels=ch)


def test_null_context_is_refused_by_both_entry_points():
    lib = api.hip_lib()
    one, n = (C.c_void_p * 1)(0), (C.c_uint64 * 1)(0)
    assert lib.xpnghip_decode_varsize_device_batch_as(None, 1, one, n, 1, None, one, 0, None) != 0
    assert "null context" in api._err()
    assert lib.xpnghip_encode_varsize_device_batch_from(None, 1, one, 0, 1, one, None, None) != 0
    assert "null context" in api._err()


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(5, 7, False), (3, 3, True)]:
        p = tmp_path / f"l7_{w}x{h}_{int(alpha)}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if alpha else "photo", w, h, alpha, seed=w)))  # (noise: translucent, stays RGBA)
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_files_answers_host_kinds_without_a_gpu(po, tmp_path):
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(7, 5, 3), (1000, 1000, 3), (3, 3, 4)]
    for lay in ("hwc", "chw"):
        for ch in (None, 3, 4):
            for bgr in (False, True):
                got = tensors.load_files(paths, layout=lay, channels=ch, bgr=bgr, device="cpu")
                assert len(got) == len(paths)
                for g, r in zip(got, want):
                    w = arrange(r, lay == "chw", bgr, ch or r.shape[2])
                    assert g.device.type == "cpu" and g.is_contiguous() and tuple(g.shape) == w.shape, (lay, ch, bgr)
                    assert np.array_equal(g.numpy(), w), (lay, ch, bgr, r.shape)
    with pytest.raises(api.XpngError):
        tensors.load_files([], device="cpu")
    with pytest.raises(api.XpngError):
        tensors.load_files(paths + [str(tmp_path / "missing.xpng")], device="cpu")
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, layout="nchw", device="cpu")
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, channels=2, device="cpu")
    import torch
    if not torch.cuda.is_available():                               # the default device is the GPU: without one, an XpngError too
        with pytest.raises(api.XpngError):
            tensors.load_files(paths)
    with pytest.raises(api.XpngError):                              # a file that needs the codec: no CPU fallback
        tensors.load_files(paths + [os.path.join(GOLD, "img_juicy.L1.xpng")], device="cpu")


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): dims, the rasters and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "flat"]
    out = {}
    for mode, alpha in FORMATS:
        dims = RGBA_DIMS if alpha else RGB_DIMS
        rasters = [synth_raster(kinds[i % 4], w, h, alpha, seed=i + 1) for i, (w, h) in enumerate(dims)]
        if alpha:
            a = np.concatenate([r[..., 3].ravel() for r in rasters])
            assert (a == 0).any() and (a == 255).any()
        blobs = [po.encode_tiles(mode, r) for r in rasters]
        for r, b, (w, h) in zip(rasters[-3:], blobs[-3:], dims[-3:]):
            assert np.array_equal(po.decode_tiles(mode, b, w, h, r.shape[2]), r)
        out[(mode, alpha)] = (dims, rasters, blobs)
    return out


def _decode_as(ctx, mode, d_b, lens, word, offs=None, expect_status=0):
    ch = api.layout_channels(word, ctx.pxsz)
    ar = Arena([ch * w * h for (w, h) in ctx.dims])
    ctx.decode_batch_as(mode, [t.data_ptr() for t in d_b], lens, ar.ptrs, word, tile_offs=offs)
    assert ctx.decode_status() == expect_status
    return ar.fetch()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_decode_into_every_layout(gpu, batches, mode, alpha):
    """All 12 layout words on one batch: the image's bytes are the rearranged oracle raster, every sentinel byte before and
    behind is intact; layout 0 is the tight form; both size walks agree; two layouts back to back on the same pointers."""
    import torch
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ws0 = None
        for word in WORDS:
            got = _decode_as(ctx, mode, d_b, lens, word)
            for i, (g, r) in enumerate(zip(got, rasters)):
                assert np.array_equal(g, arrange_word(r, word).reshape(-1)), (hex(word), i, dims[i])
            ws0 = ws0 or ctx.workspace_bytes()
        assert ctx.workspace_bytes() < ws0 + 4096                     # no second staging raster, whatever the layout
        # layout 0 against the tight form of the same context
        tight = Arena([px * w * h for (w, h) in dims])
        ctx.decode_batch(mode, [t.data_ptr() for t in d_b], lens, tight.ptrs, out_bpr=0)
        assert ctx.decode_status() == 0
        for a, b in zip(tight.fetch(), _decode_as(ctx, mode, d_b, lens, 0)):
            assert np.array_equal(a, b)
        # host-given offsets against the device-side walk
        word = api.layout(planar=True, bgr=True, channels=7 - px)
        for a, b in zip(_decode_as(ctx, mode, d_b, lens, word, _offsets(blobs, ctx)), _decode_as(ctx, mode, d_b, lens, word)):
            assert np.array_equal(a, b)
        # two layouts, back to back, on the same output pointers
        ar = Arena([4 * w * h for (w, h) in dims])
        for word in (api.layout(planar=True, channels=4), api.layout(bgr=True, channels=4), api.layout(planar=True, bgr=True, channels=4)):
            ar.t.fill_(SENTINEL)
            ctx.decode_batch_as(mode, [t.data_ptr() for t in d_b], lens, ar.ptrs, word)
            assert ctx.decode_status() == 0
            for i, (g, r) in enumerate(zip(ar.fetch(), rasters)):
                assert np.array_equal(g, arrange_word(r, word).reshape(-1)), (hex(word), i)
        torch.cuda.synchronize()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_decode_status_passes_through(gpu, po):
    """One tile of one image gets type byte 0x7F (both parsers reject it; its size word stays, so the walk finds every tile):
    the launch reports 1 and every other image is exact in a planar layout."""
    from xpng_amd.synth import synth_raster
    dims = [(300, 200), (889, 445), (100, 100), (64, 70)]
    rasters = [synth_raster("photo", w, h, True, seed=s + 1) for s, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    ctx = gpu.MixedContext(dims, 4)
    try:
        k = 1
        offs = _offsets(blobs, ctx)
        bad = bytearray(blobs[k])
        bad[offs[k][1] + 3] = 0x7F                               # top byte of the tile's first little-endian word
        bb = blobs[:k] + [bytes(bad)] + blobs[k + 1:]
        word = api.layout(planar=True, channels=3)
        got = _decode_as(ctx, 1, _upload(bb), [len(b) for b in bb], word, expect_status=1)
        for i, (g, r) in enumerate(zip(got, rasters)):
            if i != k:
                assert np.array_equal(g, arrange_word(r, word).reshape(-1)), i
        got = _decode_as(ctx, 1, _upload(blobs), [len(b) for b in blobs], word)     # and the intact batch afterwards
        for i, (g, r) in enumerate(zip(got, rasters)):
            assert np.array_equal(g, arrange_word(r, word).reshape(-1)), i
    finally:
        ctx.close()


def _encode_from(ctx, mode, rasters, word):
    """the rasters rearranged by numpy and uploaded at shifted offsets -> the blobs, after checking that the blob buffers hold
    the sentinel from the returned length on and that no input byte changed"""
    src = Arena([r.size for r in rasters], fill=[arrange_word(r, word) for r in rasters])
    bounds = [ctx.blob_bound(i) for i in range(ctx.nimg)]
    dst = Arena([b + 3 - (b + 3) % 4 for b in bounds])
    dst.ptrs = [p - p % 4 for p in dst.ptrs]                        # (blob buffers are 4-byte aligned)
    lens = ctx.encode_batch_from(mode, src.ptrs, word, dst.ptrs)
    assert src.untouched()
    got = dst.t.cpu().numpy()
    base = dst.t.data_ptr()
    out = []
    for p, n, b in zip(dst.ptrs, lens, bounds):
        o = p - base
        assert 0 < n <= b and (got[o + n:o + b + GUARD] == SENTINEL).all() and (got[o - 32:o] == SENTINEL).all()
        out.append(got[o:o + n].tobytes())
    return out, lens


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_encode_from_every_layout(gpu, batches, mode, alpha):
    """The four layout words whose channel count is the context's (named by the channel field or left to it): every blob is
    the oracle's, the returned length is right, the blob buffer is untouched from that length on."""
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    ctx = gpu.MixedContext(dims, px)
    try:
        for k, (planar, bgr) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
            word = api.layout(planar=planar, bgr=bgr, channels=px if k % 2 else 0)
            got, lens = _encode_from(ctx, mode, rasters, word)
            assert lens == [len(b) for b in blobs], hex(word)
            for i, (g, b) in enumerate(zip(got, blobs)):
                assert g == b, (hex(word), i, dims[i])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_round_trip_on_one_context_in_both_orders(gpu, batches):
    dims, rasters, blobs = batches[(1, True)]
    word = api.layout(planar=True, bgr=True)
    ctx = gpu.MixedContext(dims, 4)
    try:                                                         # encode first, then decode what it wrote
        got, lens = _encode_from(ctx, 1, rasters, word)
        back = _decode_as(ctx, 1, _upload(got), lens, word)
        for i, (g, r) in enumerate(zip(back, rasters)):
            assert np.array_equal(g, arrange_word(r, word).reshape(-1)), i
    finally:
        ctx.close()
    ctx = gpu.MixedContext(dims, 4)
    try:                                                         # decode first: the encode re-allocates the shared scratch
        back = _decode_as(ctx, 1, _upload(blobs), [len(b) for b in blobs], word)
        for i, (g, r) in enumerate(zip(back, rasters)):
            assert np.array_equal(g, arrange_word(r, word).reshape(-1)), i
        got, lens = _encode_from(ctx, 1, rasters, word)
        assert got == blobs
    finally:
        ctx.close()


@pytest.mark.gpu
def test_layout_misuse_is_refused_and_writes_nothing(gpu, po):
    from xpng_amd.synth import synth_raster
    lib = api.hip_lib()
    dims = [(300, 200), (64, 64), (17, 9)]
    for px in (3, 4):
        rasters = [synth_raster("photo", w, h, px == 4, seed=7) for (w, h) in dims]
        blobs = [po.encode_tiles(1, r) for r in rasters]
        ctx = gpu.MixedContext(dims, px)
        try:
            d_b, lens = _upload(blobs), [len(b) for b in blobs]
            ins = [t.data_ptr() for t in d_b]
            outs = Arena([4 * w * h for (w, h) in dims])
            src = Arena([r.size for r in rasters], fill=rasters)
            dst = Arena([ctx.blob_bound(i) + 4 for i in range(ctx.nimg)])
            dst.ptrs = [p - p % 4 for p in dst.ptrs]

            def refused(words, fn):
                with pytest.raises(gpu.XpngError) as e:
                    fn()
                assert all(w in str(e.value) for w in words), (words, str(e.value))
                assert outs.untouched() and dst.untouched() and src.untouched(), words

            for bad in (0x004, 0x500, 0x1000):                    # an unknown bit, channel field 5
                refused(["layout"], lambda: ctx.decode_batch_as(1, ins, lens, outs.ptrs, bad))
                refused(["layout"], lambda: ctx.encode_batch_from(1, src.ptrs, bad, dst.ptrs))
            other = api.layout(planar=True, channels=7 - px)     # a lossless encoder does not drop or invent a channel
            refused(["layout", str(px), str(7 - px)], lambda: ctx.encode_batch_from(1, src.ptrs, other, dst.ptrs))
            word = api.layout(planar=True, bgr=True)
            refused(["nimg"], lambda: ctx.decode_batch_as(1, ins[:2], lens[:2], outs.ptrs[:2], word))
            refused(["nimg"], lambda: ctx.encode_batch_from(1, src.ptrs[:2], word, dst.ptrs[:2]))
            refused(["null"], lambda: ctx.decode_batch_as(1, ins, lens, [outs.ptrs[0], 0, outs.ptrs[2]], word))
            refused(["null"], lambda: ctx.encode_batch_from(1, [src.ptrs[0], 0, src.ptrs[2]], word, dst.ptrs))
            refused(["tile mode"], lambda: ctx.decode_batch_as(3, ins, lens, outs.ptrs, word))
            # an ordinary context is refused as it is by the tight forms
            plain = gpu.Context(300, 200, px)
            try:
                vp, u64 = C.c_void_p, C.c_uint64
                one_in, one_out, one_len = (vp * 1)(ins[0]), (vp * 1)(outs.ptrs[0]), (u64 * 1)(lens[0])
                assert lib.xpnghip_decode_varsize_device_batch_as(plain._h, 1, one_in, one_len, 1, None, one_out, word, None) != 0
                assert "mixed context" in api._err()
                assert lib.xpnghip_encode_varsize_device_batch_from(plain._h, 1, (vp * 1)(src.ptrs[0]), word, 1, (vp * 1)(dst.ptrs[0]), None, None) != 0
                assert "mixed context" in api._err()
            finally:
                plain.close()
            assert outs.untouched() and dst.untouched() and src.untouched()
            # the context still works after all that
            for g, r in zip(_decode_as(ctx, 1, d_b, lens, word), rasters):
                assert np.array_equal(g, arrange_word(r, word).reshape(-1))
        finally:
            ctx.close()


@pytest.mark.gpu
def test_load_files_on_the_reference_written_goldens(gpu, po, manifest, tmp_path):
    """The committed reference-written goldens of at most 1.2 Mpx (levels 1 and 2, RGB and RGBA), the single-colour file and a
    level-7 file in one list: several codec groups and both host-answered kinds."""
    import torch
    from xpng_amd import tensors
    names = [n for n, e in sorted(manifest.items()) if e["w"] * e["h"] <= 1_200_000 and
             (n.startswith(("crop_", "img_", "imgfull_")) or n in ("special_hidden_colour", "special_opaque_alpha"))]
    assert {"img_juicy", "img_pigz-logo", "special_hidden_colour", "special_opaque_alpha"} <= set(names)
    files = sorted({manifest[n][lv]["file"] for n in names for lv in ("L1", "L2") if manifest[n].get(lv, {}).get("file")})
    paths = [os.path.join(GOLD, f) for f in files]
    host, _ = _host_files(po, tmp_path)
    paths = paths[:5] + host[:1] + paths[5:] + host[2:]          # (host[1], the single-colour golden, is in the list already)
    heads = [open(p, "rb").read(8) for p in paths]
    assert {(h[3], h[7] & 1) for h in heads} >= {(1, 0), (1, 1), (2, 0), (7, 0), (7, 1)}
    assert any(os.path.getsize(p) == 11 for p in paths)
    want = [gpu.load(p) for p in paths]
    got = tensors.load_files(paths, layout="hwc")
    assert len(got) == len(paths)
    for p, g, r in zip(paths, got, want):
        assert g.is_cuda and g.dtype == torch.uint8 and g.is_contiguous() and tuple(g.shape) == r.shape, p
        assert np.array_equal(g.cpu().numpy(), r), p
    assert {r.shape[2] for r in want} == {3, 4}
    chw3 = tensors.load_files(paths, layout="chw", channels=3)
    chw4 = tensors.load_files(paths, layout="chw", channels=4, bgr=True)
    for p, a, b, r in zip(paths, chw3, chw4, want):
        assert a.is_cuda and b.is_cuda and a.is_contiguous() and b.is_contiguous(), p
        assert np.array_equal(a.cpu().numpy(), arrange(r, True, False, 3)), p
        assert np.array_equal(b.cpu().numpy(), arrange(r, True, True, 4)), p
    by_size = {}
    for t in chw3:                                               # RGB and RGBA files alike: one batch per size
        by_size.setdefault(tuple(t.shape), []).append(t)
    assert any(len(v) > 1 for v in by_size.values())
    for shape, ts in by_size.items():
        assert tuple(torch.stack(ts).shape) == (len(ts),) + shape
    bad = tmp_path / "bad.xpng"                                    # a rejected tile fails the whole call
    data = bytearray(open(os.path.join(GOLD, "img_juicy.L1.xpng"), "rb").read())
    data[8 + 3] = 0x7F
    bad.write_bytes(bytes(data))
    with pytest.raises(api.XpngError):
        tensors.load_files(paths[:3] + [str(bad)], layout="chw")
