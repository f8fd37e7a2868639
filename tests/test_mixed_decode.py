"""Mixed-size batch decode: images of different sizes in one device call (include/xpng_hip.h "mixed-size batch decode",
include/xpng_batch.h).

CPU: the new symbols are exported, xpng_load_batch answers its host-only forms (level 7, whole-image single colour) like the
oracle, a list with a missing or truncated file fails as a whole, and nothing computes without a device.  GPU (-m gpu): the
reference-written corpus goldens grouped by (level, alpha), synthetic batches of seeded random sizes in both output forms with
sentinel-filled padding and guards, the device-side size walk against host-given offsets, rejected tiles, truncated size chains,
misuse, xpng_load_batch against xpng_load, and a same-size batch against the ordinary batched context.  Every comparison is
bit-exact."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from _kit import built_with_probes as built, declared, exported, gpu, _offsets, po, SENTINEL, _upload
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# geometries every synthetic batch holds: one tile (100 x 100, 444 x 444), the two-tile split (445 x 444, 889 x 445), the
# narrow-image tile shapes (300 x 4000, 4000 x 300)
FIXED_DIMS = [(100, 100), (445, 444), (889, 445), (300, 4000), (4000, 300), (444, 444)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_mixed_symbols_are_declared_and_exported():
    batch = declared("xpng_batch.h", "xpng_")
    assert batch == sorted(api.HOST_BATCH_SYMBOLS) == ["xpng_load_batch"]
    assert set(batch) <= exported(api.HOST_SO)
    mixed = [n for n in declared("xpng_hip.h", "xpnghip_") if "mixed" in n]
    assert mixed == sorted(["xpnghip_ctx_create_mixed", "xpnghip_ctx_mixed_first_tile", "xpnghip_decode_mixed_device_batch",
                            "xpnghip_decode_mixed"])
    assert set(mixed) <= set(api.HIP_SYMBOLS)
    for so in (api.HIP_SO, api.PROBES_SO):
        assert set(mixed) <= exported(so), so
    import xpng_amd
    for name in ("MixedContext", "decode_mixed", "load_batch"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)


def _host_only_files(po, tmp_path):
    """level-7 files of different sizes, RGB and RGBA, and the whole-image single-colour file of level 2"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (W, H, alpha) in [(1500, 1200, False), (445, 444, True), (300, 700, True), (3, 50, False), (1, 1, True)]:
        p = tmp_path / f"l7_{W}x{H}_{int(alpha)}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("photo", W, H, alpha, seed=W)))
        paths.append(str(p))
    data = po.encode_image(2, synth_raster("flat", 1000, 900, False))
    assert len(data) == 11                                     # the whole-image single-colour file of level 2
    p = tmp_path / "single.xpng"
    p.write_bytes(data)
    paths.insert(2, str(p))
    return paths


def test_load_batch_host_only_forms_equal_the_oracle(po, tmp_path):
    paths = _host_only_files(po, tmp_path)
    got = api.load_batch(paths)
    assert len(got) == len(paths)
    for p, g in zip(paths, got):
        want = po.decode_image(open(p, "rb").read())
        assert g.shape == want.shape and np.array_equal(g, want), p
    assert {g.shape[2] for g in got} == {3, 4} and len({g.shape[:2] for g in got}) == len(paths)


def test_load_batch_fails_as_a_whole(po, tmp_path):
    good = _host_only_files(po, tmp_path)
    cut = tmp_path / "cut.xpng"
    cut.write_bytes(open(good[0], "rb").read()[:1000])          # a level-7 file shorter than its raster
    short = tmp_path / "short.xpng"
    short.write_bytes(b"\0\0\0")                                # shorter than a header
    badmode = tmp_path / "badmode.xpng"
    badmode.write_bytes(b"\x09\0\0\x05\x09\0\0\0" + b"\0" * 400)
    L = api.host_lib()
    for bad in (str(tmp_path / "missing.xpng"), str(cut), str(short), str(badmode)):
        for pos in (0, len(good) // 2, len(good)):
            paths = good[:pos] + [bad] + good[pos:]
            with pytest.raises(api.XpngError):
                api.load_batch(paths)
            pms = (api.XpngT * len(paths))()
            arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
            assert L.xpng_load_batch(arr, len(paths), pms) == 1
            assert all(not pm.p for pm in pms), (bad, pos)       # everything it allocated was freed and cleared
    with pytest.raises(api.XpngError):
        api.load_batch([])


def test_mixed_context_arguments_and_no_device():
    lib = api.hip_lib()
    h = C.c_void_p()
    for dims, pxsz, word in [([(0, 5)], 3, "size of image 0"), ([(5, 5), (5, (1 << 24) + 1)], 4, "size of image 1"),
                             ([(5, 5)], 5, "bad arguments"), ([], 3, "4096"), ([(8, 8)] * 4097, 3, "4096"),
                             ([(1 << 24, 1 << 24)] * 4, 3, "32 bits")]:
        flat = (C.c_uint64 * max(2 * len(dims), 1))(*[v for d in dims for v in d])
        assert lib.xpnghip_ctx_create_mixed(C.byref(h), 0, flat, len(dims), pxsz) != 0
        assert word in api._err(), (dims[:2], api._err())
    assert lib.xpnghip_ctx_mixed_first_tile(None, 0) == (1 << 64) - 1
    if api.device_count() > 0:
        ctx = api.MixedContext([(100, 100), (889, 445)], 3)
        assert ctx.n_tiles == 3 and ctx.first_tile == [0, 1, 3]
        ctx.close()
    else:
        with pytest.raises(api.XpngError):
            api.MixedContext([(100, 100), (889, 445)], 3)


def test_decode_mixed_rejects_bad_input_before_device_work(po):
    """Truncated bodies, a bad mode and mode 2 with RGBA fail with a message and write nothing, with or without a GPU."""
    from xpng_amd.synth import synth_raster
    a = po.encode_tiles(1, synth_raster("photo", 889, 445, False))
    b = po.encode_tiles(1, synth_raster("photo", 100, 100, False))
    dims = [(889, 445), (100, 100)]
    for bodies, mode, pxsz, word in [([a[:5], b], 1, 3, "truncated"), ([a, b[:-1]], 1, 3, "truncated"), ([a[: len(a) // 2], b], 1, 3, "truncated"),
                                     ([a, b], 3, 3, "tile mode"), ([a, b], 2, 4, "RGB only"), ([a, b], 1, 5, "geometry")]:
        with pytest.raises(api.XpngError) as e:
            api.decode_mixed(mode, bodies, dims, pxsz)
        assert word in str(e.value), (word, str(e.value))
    if api.device_count() == 0:
        with pytest.raises(api.XpngError):
            api.decode_mixed(1, [a, b], dims, 3)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _decode_padded(ctx, mode, d_b, lens, pad, offs=None, expect_status=0):
    """padded form at a pitch `pad` bytes beyond the widest row, `extra` sentinel rows behind every image: returns the rasters
    after checking that every byte outside [0, w * pxsz) of rows < h, and every row >= h, still holds the sentinel"""
    import torch
    ch, extra = ctx.pxsz, 3
    bpr = max(w for (w, h) in ctx.dims) * ch + pad
    d_o = [torch.full(((h + extra) * bpr,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in ctx.dims]
    ctx.decode_batch(mode, [t.data_ptr() for t in d_b], lens, [t.data_ptr() for t in d_o], out_bpr=bpr, tile_offs=offs)
    assert ctx.decode_status() == expect_status
    torch.cuda.synchronize()
    out = []
    for (w, h), t in zip(ctx.dims, d_o):
        rows = t.cpu().numpy().reshape(h + extra, bpr)
        assert (rows[:h, w * ch:] == SENTINEL).all(), ("bytes past the row written", w, h)
        assert (rows[h:] == SENTINEL).all(), ("rows below the image written", w, h)
        out.append(rows[:h, : w * ch].reshape(h, w, ch).copy())
    return out


def _decode_tight(ctx, mode, d_b, lens, offs=None, expect_status=0):
    """tight form with a 256-byte sentinel guard behind every raster: returns the rasters after checking the guards"""
    import torch
    ch, guard = ctx.pxsz, 256
    d_o = [torch.full((h * w * ch + guard,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in ctx.dims]
    ctx.decode_batch(mode, [t.data_ptr() for t in d_b], lens, [t.data_ptr() for t in d_o], tile_offs=offs)
    assert ctx.decode_status() == expect_status
    torch.cuda.synchronize()
    out = []
    for (w, h), t in zip(ctx.dims, d_o):
        got = t.cpu().numpy()
        assert (got[h * w * ch:] == SENTINEL).all(), ("guard behind the raster written", w, h)
        out.append(got[: h * w * ch].reshape(h, w, ch).copy())
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (what, i, w.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["XPNG_WIDE_RANS", "XPNG_NARROW_RANS"])
def test_corpus_groups_in_one_mixed_call(gpu, po, manifest, monkeypatch, form):
    """The 17 reference-written goldens of each level, grouped by the (level, alpha) of their header: every group is ONE mixed
    call, in both output forms, and every image equals the oracle's decode."""
    from conftest import GOLD, corpus_entries
    monkeypatch.setenv(form, "1")
    done, sizes = 0, set()
    for level in (1, 2):
        groups = {}
        for name, ent in corpus_entries(manifest):
            data = open(os.path.join(GOLD, ent[f"L{level}"]["file"]), "rb").read()
            mode, ch = data[3], 3 + (data[7] & 1)
            if mode not in (1, 2) or (len(data) == 11 + (ch == 4) and data[7] & 2):
                continue                                         # (no tile body: xpng_load_batch answers these on the host)
            groups.setdefault((mode, ch), []).append((name, data))
        for (mode, ch), members in sorted(groups.items()):
            want = [po.decode_image(d) for _, d in members]
            dims = [(r.shape[1], r.shape[0]) for r in want]
            blobs = [d[8:] for _, d in members]
            ctx = gpu.MixedContext(dims, ch)
            try:
                d_b, lens = _upload(blobs), [len(b) for b in blobs]
                _same(_decode_padded(ctx, mode, d_b, lens, 64), want, (level, mode, ch, form, "padded"))
                _same(_decode_tight(ctx, mode, d_b, lens), want, (level, mode, ch, form, "tight"))
                _same(gpu.decode_mixed(mode, blobs, dims, ch), want, (level, mode, ch, form, "host buffers"))
            finally:
                ctx.close()
            done += len(members)
            sizes |= set(dims)
    assert done >= 30 and len(sizes) == 17


def _synthetic_batch(po, mode, alpha, n=48):
    from xpng_amd.synth import synth_raster
    rng = random.Random(1000 * mode + alpha)
    dims = list(FIXED_DIMS)
    if not alpha:
        dims += [(3, 500), (1, 37)]                              # RGB narrower than 4 px
    while len(dims) < n:
        dims.append((rng.randint(5, 1400), rng.randint(5, 1100)))
    rng.shuffle(dims)
    kinds = ["photo", "photo", "noise", "gray", "photo", "flat"]
    rasters = [synth_raster(kinds[i % len(kinds)], w, h, alpha, seed=i + 1) for i, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(mode, r) for r in rasters]
    return dims, rasters, blobs


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", [(1, False), (2, False), (1, True)])
def test_synthetic_sizes_both_output_forms_and_both_walks(gpu, po, mode, alpha):
    """48 oracle-encoded images of seeded random sizes and the fixed geometries: the padded form at a pitch beyond the widest
    row leaves every sentinel byte of the padding and of the rows below each image alone, the tight form leaves its guards alone,
    and the device-side size walk and host-given offsets give the same rasters - the oracle's."""
    dims, rasters, blobs = _synthetic_batch(po, mode, alpha)
    assert len(dims) >= 48 and set(FIXED_DIMS) <= set(dims)
    ch = 4 if alpha else 3
    want = [po.decode_tiles(mode, b, w, h, ch) for b, (w, h) in zip(blobs, dims)]
    _same(want, rasters, "oracle round trip")
    ctx = gpu.MixedContext(dims, ch)
    try:
        assert ctx.first_tile[0] == 0 and ctx.first_tile[-1] == ctx.n_tiles
        for i, (w, h) in enumerate(dims):
            tiles = [ctx.tile(t) for t in range(ctx.first_tile[i], ctx.first_tile[i + 1])]
            assert tiles == [tuple(t) for t in po.tile_table(w, h, ch)], (w, h)
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        offs = _offsets(blobs, ctx)
        ws0 = ctx.workspace_bytes()
        a = _decode_padded(ctx, mode, d_b, lens, 100)
        _same(a, want, (mode, alpha, "padded, device walk"))
        _same(_decode_padded(ctx, mode, d_b, lens, 100, offs), a, (mode, alpha, "padded, host offsets"))
        ws1 = ctx.workspace_bytes()
        _same(_decode_tight(ctx, mode, d_b, lens, offs), a, (mode, alpha, "tight, host offsets"))
        _same(_decode_tight(ctx, mode, d_b, lens), a, (mode, alpha, "tight, device walk"))
        # the staging raster is allocated by the first tight call and counted: sum of h_i rows at the widest pitch (rounded up to 16)
        pitch = -(-max(w for w, _ in dims) * ch // 16) * 16
        stage = sum(-(-h * pitch // 256) * 256 for (_, h) in dims)
        assert ws1 >= ws0 and ctx.workspace_bytes() >= ws1 + stage
        assert ctx.workspace_bytes() < ws1 + stage + (1 << 20)
    finally:
        ctx.close()


def _corrupt_case(po, mode):
    from xpng_amd.synth import special_cases, synth_raster
    if mode == 1:
        rasters = [synth_raster("photo", w, h, True, seed=s) for s, (w, h) in enumerate([(700, 500), (1500, 1200), (100, 100), (889, 445), (1000, 950)])]
    else:
        rasters = [synth_raster("photo", 700, 500, False, seed=3), dict(special_cases())["mixed_tiles"], synth_raster("gray", 100, 100, False),
                   synth_raster("photo", 889, 445, False, seed=4), synth_raster("noise", 600, 950, False, seed=5)]
    blobs = [po.encode_tiles(mode, r) for r in rasters]
    return rasters, blobs


def _check_all_but(ctx, got, want, k, bad_tiles, what):
    """every image but k is exact, and so is every tile of image k outside bad_tiles (indices inside the image)"""
    for i, (g, w) in enumerate(zip(got, want)):
        if i != k:
            assert np.array_equal(g, w), (what, "image", i)
    n = ctx.first_tile[k + 1] - ctx.first_tile[k]
    for t in range(n):
        if t in bad_tiles:
            continue
        x, y, w, h = ctx.tile(ctx.first_tile[k] + t)
        assert np.array_equal(got[k][y:y + h, x:x + w], want[k][y:y + h, x:x + w]), (what, "tile", t)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_a_rejected_tile_leaves_every_other_tile_exact(gpu, po, mode):
    """One tile of one image gets type byte 0x7F (both parsers reject it; its size word stays, so the walk still finds every
    tile): the launch reports 1, every other image and every other tile of that image are exact, in both forms and walks."""
    rasters, blobs = _corrupt_case(po, mode)
    dims = [(r.shape[1], r.shape[0]) for r in rasters]
    ch = rasters[0].shape[2]
    ctx = gpu.MixedContext(dims, ch)
    try:
        offs = _offsets(blobs, ctx)
        k = 1
        n = len(offs[k])
        assert n >= 4
        for t in (0, n // 2, n - 1):
            bad = bytearray(blobs[k])
            bad[offs[k][t] + 3] = 0x7F                           # top byte of the tile's first little-endian word
            bb = blobs[:k] + [bytes(bad)] + blobs[k + 1:]
            d_b, lens = _upload(bb), [len(b) for b in bb]
            _check_all_but(ctx, _decode_padded(ctx, mode, d_b, lens, 32, None, 1), rasters, k, {t}, (mode, t, "padded, device walk"))
            _check_all_but(ctx, _decode_tight(ctx, mode, d_b, lens, offs, 1), rasters, k, {t}, (mode, t, "tight, host offsets"))
            with pytest.raises(gpu.XpngError):
                gpu.decode_mixed(mode, bb, dims, ch)
        d_b, lens = _upload(blobs), [len(b) for b in blobs]       # and the same context accepts the intact batch afterwards
        _same(_decode_tight(ctx, mode, d_b, lens), rasters, (mode, "intact"))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_a_truncated_size_chain_is_rejected_inside_its_buffer(gpu, po, mode):
    """The device-side walk of an image whose buffer ends inside tile t's size word, or whose tile t claims size 0 or a size
    beyond the buffer, parks tiles t.. at the end of the buffer: they are rejected, nothing outside the buffer is needed, and the
    tiles in front of t and every other image are exact."""
    rasters, blobs = _corrupt_case(po, mode)
    dims = [(r.shape[1], r.shape[0]) for r in rasters]
    ch = rasters[0].shape[2]
    ctx = gpu.MixedContext(dims, ch)
    try:
        offs = _offsets(blobs, ctx)
        k, n = 1, len(offs[1])
        t = n // 2
        assert 0 < t < n - 1
        cut = blobs[k][: offs[k][t] + 2]                         # the buffer ends inside tile t's first word
        zero = bytearray(blobs[k]); zero[offs[k][t]: offs[k][t] + 3] = b"\0\0\0"
        huge = bytearray(blobs[k]); huge[offs[k][t]: offs[k][t] + 3] = b"\xff\xff\xff"
        for what, body in (("cut", cut), ("zero size", bytes(zero)), ("size beyond the buffer", bytes(huge))):
            bb = blobs[:k] + [body] + blobs[k + 1:]
            d_b, lens = _upload(bb), [len(b) for b in bb]
            bad = set(range(t, n))
            _check_all_but(ctx, _decode_padded(ctx, mode, d_b, lens, 16, None, 1), rasters, k, bad, (mode, what, "padded"))
            _check_all_but(ctx, _decode_tight(ctx, mode, d_b, lens, None, 1), rasters, k, bad, (mode, what, "tight"))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_misuse_is_refused_and_writes_nothing(gpu, po):
    import torch
    from xpng_amd.synth import synth_raster
    lib = api.hip_lib()
    dims = [(700, 500), (300, 200), (889, 445)]
    for ch in (3, 4):
        rasters = [synth_raster("photo", w, h, ch == 4, seed=7) for (w, h) in dims]
        blobs = [po.encode_tiles(1, r) for r in rasters]
        ctx = gpu.MixedContext(dims, ch)
        try:
            d_b, lens = _upload(blobs), [len(b) for b in blobs]
            wide = 889 * ch
            d_o = [torch.full((h * wide + 256,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in dims]
            ins, outs = [t.data_ptr() for t in d_b], [t.data_ptr() for t in d_o]

            def refused(word, fn):
                with pytest.raises(gpu.XpngError) as e:
                    fn()
                assert word in str(e.value), (word, str(e.value))
                torch.cuda.synchronize()
                assert all(bool((t == SENTINEL).all()) for t in d_o), word

            refused("out_bpr", lambda: ctx.decode_batch(1, ins, lens, outs, out_bpr=wide - 1))
            refused("nimg", lambda: ctx.decode_batch(1, ins[:2], lens[:2], outs[:2]))
            refused("tile mode", lambda: ctx.decode_batch(3, ins, lens, outs))
            refused("null", lambda: ctx.decode_batch(1, ins, lens, [outs[0], 0, outs[2]]))
            refused("aligned", lambda: ctx.decode_batch(1, ins, lens, [outs[0] + 4] + outs[1:], out_bpr=wide))
            if ch == 4:
                refused("RGB only", lambda: ctx.decode_batch(2, ins, lens, outs))
            # the entry points of an ordinary context refuse a mixed one
            vp, u64 = C.c_void_p, C.c_uint64
            one_in, one_out, one_len = (vp * 1)(ins[0]), (vp * 1)(outs[0]), (u64 * 1)(lens[0])
            calls = [
                lambda: lib.xpnghip_encode_device_batch(ctx._h, 1, one_out, 1, 0, 1, one_in, None, None),
                lambda: lib.xpnghip_encode_device(ctx._h, 1, outs[0], 0, 1, ins[0], None, None),
                lambda: lib.xpnghip_decode_device_batch(ctx._h, 1, one_in, one_len, 1, None, 0, 1, one_out, None),
                lambda: lib.xpnghip_decode_device(ctx._h, 1, ins[0], lens[0], None, 0, 1, outs[0], None),
                lambda: lib.xpnghip_m1_transform_device(ctx._h, outs[0], 0, 1, None),
                lambda: lib.xpnghip_m1_transform_device_batch(ctx._h, one_out, 1, 0, 1, None),
                lambda: lib.xpnghip_decode_region_device_batch(ctx._h, 1, one_in, one_len, 1, None, (u64 * 4)(0, 0, 8, 8), one_out, 8 * ch, None),
            ]
            for k, call in enumerate(calls):
                assert call() != 0 and "mixed context" in api._err(), (k, api._err())
                torch.cuda.synchronize()
                assert all(bool((t == SENTINEL).all()) for t in d_o), k
            # ... and the mixed entry point refuses an ordinary one
            plain = gpu.Context(700, 500, ch)
            try:
                assert lib.xpnghip_decode_mixed_device_batch(plain._h, 1, one_in, one_len, 1, None, one_out, 0, None) != 0
                assert "mixed context" in api._err()
            finally:
                plain.close()
            # the context still works after all that
            _same(_decode_tight(ctx, 1, d_b, lens), rasters, "after misuse")
        finally:
            ctx.close()


@pytest.mark.gpu
def test_load_batch_equals_load_of_each_file(gpu, po, manifest, tmp_path):
    """The 34 corpus files (both levels) and level-7 / single-colour files in one xpng_load_batch call."""
    from conftest import GOLD, corpus_entries
    paths = [os.path.join(GOLD, ent[f"L{level}"]["file"]) for level in (1, 2) for _, ent in corpus_entries(manifest)]
    assert len(paths) == 34
    host = _host_only_files(po, tmp_path)
    paths = paths[:10] + host[:3] + paths[10:] + host[3:]
    got = gpu.load_batch(paths)
    assert len(got) == len(paths)
    for p, g in zip(paths, got):
        want = gpu.load(p)
        assert g.shape == want.shape and np.array_equal(g, want), p
        assert np.array_equal(g, po.decode_image(open(p, "rb").read())), p


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", [(1, True), (1, False), (2, False)])
def test_same_size_batch_equals_the_ordinary_batched_context(gpu, po, mode, alpha):
    """A mixed context whose images all share one size against Context.decode_device_batch on the same blobs."""
    import torch
    from xpng_amd.synth import synth_raster_torch
    W, H, B = 1500, 1200, 12
    ch = 4 if alpha else 3
    uni = gpu.Context(W, H, ch, batch=B)
    mix = gpu.MixedContext([(W, H)] * B, ch)
    try:
        assert mix.n_tiles == B * uni.n_tiles and mix.first_tile == [i * uni.n_tiles for i in range(B + 1)]
        d_r = [synth_raster_torch("photo", W, H, alpha, seed=50 * mode + b) for b in range(B)]
        d_b = [torch.empty(uni.blob_bound() + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
        lens = uni.encode_device_batch(mode, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
        d_u = [torch.zeros(H * W * ch + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
        uni.decode_device_batch(mode, [t.data_ptr() for t in d_b], lens, None, [t.data_ptr() for t in d_u])
        assert uni.decode_status() == 0
        torch.cuda.synchronize()
        want = [t[: H * W * ch].cpu().numpy().reshape(H, W, ch) for t in d_u]
        _same(want, [t.cpu().numpy().reshape(H, W, ch) for t in d_r], "uniform round trip")
        _same(_decode_tight(mix, mode, d_b, lens), want, (mode, alpha, "tight"))
        _same(_decode_padded(mix, mode, d_b, lens, 48), want, (mode, alpha, "padded"))
    finally:
        uni.close()
        mix.close()
