"""Mixed-size batch encode: images of different sizes in one device call (include/xpng_hip.h
xpnghip_encode_varsize_device_batch, xpnghip_images_*; include/xpng_store_batch.h).

CPU: the new symbols are declared, listed and exported; xpng_store_batch writes its host-only forms (level 7, single pixel, the
flat RGB file of level 2) like the oracle with no device present; argument failures create no file; the device entry points
refuse bad arguments with a message.  GPU (-m gpu): one synthetic batch per pixel format with every tile geometry the launch
treats differently, in the padded and the tight input form and in both rANS forms, against the oracle's tile blobs; a round trip
on one context in both orders; a same-size batch against the ordinary batched context; misuse; the staged batch and
xpng_store_batch against xpng_store and the oracle's files.  Every comparison is bit-exact."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from _kit import built_with_probes as built, declared, exported, FORMATS, gpu, po, SENTINEL, _upload
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
# one tile (100 x 100, 444 x 444), two tiles (889 x 445), nine tiles whose widest is 612 px (1500 x 1200), six tiles 715 tall
# (300 x 4000), the smallest RGBA the codec accepts (4 x 4), an odd small size (17 x 4)
STRIP_DIMS = [(100, 100), (444, 444), (889, 445), (1500, 1200), (300, 4000), (4, 4), (17, 4)]
WIDE_DIMS = [(673, 10), (2000, 100)]                             # one tile wider than TR_MAXW = 672: the generic transform for the call
RGB_SMALL = [(1, 7), (2, 1), (3, 3), (5, 7)]                     # rows shorter than a dword; tight RGB rows at all four alignments
FORMS = ["XPNG_WIDE_RANS", "XPNG_NARROW_RANS"]


NEW_HIP = ["xpnghip_encode_varsize_device_batch", "xpnghip_images_begin", "xpnghip_images_single_colour", "xpnghip_images_encode",
           "xpnghip_images_fetch", "xpnghip_images_end", "xpnghip_images_first_pixel", "xpnghip_batch_cuts"]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_and_exported():
    hip = declared("xpng_hip.h", "xpnghip_")
    assert set(NEW_HIP) <= set(hip) and set(NEW_HIP) <= set(api.HIP_SYMBOLS)
    assert not [n for n in NEW_HIP if "mixed" in n]
    for so in (api.HIP_SO, api.PROBES_SO):
        assert set(NEW_HIP) <= exported(so), so
    assert declared("xpng_store_batch.h", "xpng_") == sorted(api.HOST_STORE_BATCH_SYMBOLS) == ["xpng_store_batch"]
    assert "xpng_store_batch" in exported(api.HOST_SO)
    assert declared("xpng_batch.h", "xpng_") == ["xpng_load_batch"] == api.HOST_BATCH_SYMBOLS
    import xpng_amd
    for name in ("store_batch", "StagedImages", "MixedContext"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert hasattr(api.MixedContext, "encode_batch") and hasattr(api.MixedContext, "blob_bound")


def _host_only_list():
    """(level, raster) pairs xpng_store_batch answers on the host"""
    from xpng_amd.synth import special_cases, synth_raster
    out = [(7, synth_raster("photo", W, H, alpha, seed=W)) for (W, H, alpha) in [(700, 500, False), (445, 444, True), (3, 50, True), (1, 1, False)]]
    out.append((7, dict(special_cases())["hidden_colour"]))      # the host's normalize_RGBA shows: hidden colours zeroed
    out.append((7, dict(special_cases())["opaque_alpha"]))       # ... and an opaque RGBA raster is stored as RGB
    out += [(1, synth_raster("photo", 1, 1, False)), (2, synth_raster("photo", 1, 1, True)), (1, synth_raster("photo", 1, 1, True))]
    out.append((2, synth_raster("flat", 1000, 900, False)))      # the 11-byte file
    return out


def test_store_batch_host_only_forms_equal_the_oracle(po, tmp_path):
    items = _host_only_list()
    for level in (1, 2, 7):
        members = [r for (lv, r) in items if lv == level]
        paths = [str(tmp_path / f"h{level}_{i}.xpng") for i in range(len(members))]
        api.store_batch(level, members, paths)
        for r, p in zip(members, paths):
            got, want = open(p, "rb").read(), po.encode_image(level, r)
            assert got == want, (level, r.shape, len(got), len(want))
            if level == 2 and r.shape[0] * r.shape[1] > 1:
                assert len(got) == 11


def _pm(r, s=None):
    r = np.ascontiguousarray(r)
    return api.XpngT(r.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[1], r.shape[0], r.size if s is None else s, r.shape[2] == 4)


def test_store_batch_argument_failures_create_no_file(tmp_path):
    from xpng_amd.synth import synth_raster
    L = api.host_lib()
    good = [np.ascontiguousarray(synth_raster("photo", 40 + i, 30, i % 2 == 1, seed=i)) for i in range(4)]

    def call(mode, rasters, paths, sizes=None):
        n = len(rasters)
        pms = (api.XpngT * max(n, 1))(*[_pm(r, None if sizes is None else sizes[i]) for i, r in enumerate(rasters)])
        arr = (C.c_char_p * max(n, 1))(*[None if p is None else os.fsencode(p) for p in paths])
        return L.xpng_store_batch(mode, pms, arr, n)

    paths = [str(tmp_path / f"f{i}.xpng") for i in range(4)]
    assert call(7, [], []) == 1                                  # n == 0
    assert L.xpng_store_batch(7, None, None, 3) == 1
    assert call(7, good, paths[:2] + [None] + paths[3:]) == 1    # a NULL path
    for mode in (0, 3, 8):
        assert call(mode, good, paths) == 1                      # a bad mode
    for pos in (0, 2, 3):                                        # one image whose s disagrees with w * h * (3 + A): first, middle, last
        sizes = [r.size for r in good]
        sizes[pos] += 1
        for mode in (1, 2, 7):
            assert call(mode, good, paths, sizes) == 1
    assert os.listdir(tmp_path) == []
    assert call(7, good, paths) == 0 and sorted(os.listdir(tmp_path)) == [f"f{i}.xpng" for i in range(4)]
    with pytest.raises(api.XpngError):
        api.store_batch(7, [], [])


def test_batch_cuts_follow_the_chunking_rule():
    """The cut points themselves, on the CPU: a batch closes at max_images, or before the image whose rows - at the pitch of
    the widest image so far, that image included - would take the padded rasters past max_bytes; an image that alone passes the
    budget is a batch of its own; the order is kept."""
    cuts = api.batch_cuts
    dims = [(10, 10)] * 10
    assert cuts(dims, [3] * 10, 4, 1 << 30) == [0, 4, 8]                          # the image count
    assert cuts(dims, [3] * 10, 100, 30 * 10 * 3) == [0, 3, 6, 9]                 # 3 images = 30 rows x 30 B fit exactly; a 4th does not
    assert cuts(dims, [3] * 10, 100, 30 * 10 * 3 - 1) == [0, 2, 4, 6, 8]
    assert cuts(dims, [3] * 10, 100, 1) == list(range(10))                        # every image alone passes the budget
    assert cuts([(10, 10), (10, 10), (100, 1), (10, 10)], [3, 3, 3, 3], 100, 3000) == [0, 2, 3]  # one wide image widens every row: 21 x 300 and 11 x 300 > 3000
    assert cuts([(10, 10), (10, 10)], [3, 4], 100, 20 * 40 - 1) == [0, 1]         # the pitch is w * pxsz of the image as handed in
    assert cuts([(10, 10), (10, 10)], [3, 4], 100, 20 * 40) == [0]
    # the list of test_store_batch_splits_a_list_and_keeps_its_order under xpng_store_batch's own budgets
    assert cuts([(64, 48), (30000, 4), (4, 24000), (100, 100), (30000, 4)], [3] * 5) == [0, 2, 4]
    assert cuts([(8, 8)] * 4100, [4] * 4100) == [0, 4096]
    lib, u64 = api.hip_lib(), C.c_uint64
    one = (u64 * 2)(5, 5)
    assert lib.xpnghip_batch_cuts(0, one, (C.c_uint8 * 1)(3), 4, 100, (C.c_uint32 * 1)(), 1) == -1
    assert lib.xpnghip_batch_cuts(1, None, (C.c_uint8 * 1)(3), 4, 100, (C.c_uint32 * 1)(), 1) == -1
    assert lib.xpnghip_batch_cuts(2, (u64 * 4)(5, 5, 5, 5), (C.c_uint8 * 2)(3, 3), 1, 100, (C.c_uint32 * 1)(), 1) == -1  # cap too small


def test_device_entry_points_refuse_bad_arguments():
    lib = api.hip_lib()
    vp, u64 = C.c_void_p, C.c_uint64
    assert lib.xpnghip_encode_varsize_device_batch(None, 1, (vp * 1)(), 0, 1, (vp * 1)(), None, None) != 0
    assert "null context" in api._err()
    r = np.zeros((5, 6, 3), dtype=np.uint8)
    h = vp()
    ptr, dims, pin, pout = (vp * 1)(r.ctypes.data), (u64 * 2)(6, 5), (C.c_uint8 * 1)(3), (C.c_uint8 * 1)()
    cases = [((None, 1, ptr, dims, pin, pout), "null"), ((C.byref(h), 0, ptr, dims, pin, pout), "4096"),
             ((C.byref(h), 4097, ptr, dims, pin, pout), "4096"), ((C.byref(h), 1, None, dims, pin, pout), "null"),
             ((C.byref(h), 1, (vp * 1)(), dims, pin, pout), "null"), ((C.byref(h), 1, ptr, (u64 * 2)(0, 5), pin, pout), "geometry"),
             ((C.byref(h), 1, ptr, (u64 * 2)(6, (1 << 24) + 1), pin, pout), "geometry"), ((C.byref(h), 1, ptr, dims, (C.c_uint8 * 1)(5), pout), "geometry")]
    for args, word in cases:
        assert lib.xpnghip_images_begin(*args) != 0
        assert word in api._err(), (word, api._err())
        assert not h.value
    assert lib.xpnghip_images_single_colour(None, (C.c_uint8 * 1)()) != 0
    assert lib.xpnghip_images_fetch(None, 0, r.ctypes.data_as(vp)) != 0
    assert lib.xpnghip_images_first_pixel(None, 0, r.ctypes.data_as(vp)) != 0
    lib.xpnghip_images_end(None)
    if api.device_count() == 0:                                  # without a device the calls fail rather than crash
        assert lib.xpnghip_images_begin(C.byref(h), 1, ptr, dims, pin, pout) != 0 and "device" in api._err()
        with pytest.raises(api.XpngError):
            api.StagedImages([r])


# ---- GPU ------------------------------------------------------------------------------------------------------------
_BATCHES = {}


def _batch(po, mode, alpha):
    """The synthetic batch of one format: (dims, rasters, oracle blobs, is-strip-member), computed once."""
    key = (mode, alpha)
    if key not in _BATCHES:
        from xpng_amd.synth import special_cases, synth_raster
        rng = random.Random(77 + 10 * mode + alpha)
        dims = STRIP_DIMS + WIDE_DIMS + ([] if alpha else RGB_SMALL)
        rnd = [(rng.randint(5, 1200), rng.randint(5, 1200)) for _ in range(12)]
        rnd[:4] = [(w - w % 4 + k + 4, h) for k, (w, h) in enumerate(rnd[:4])]  # widths with w mod 4 = 0..3
        assert {w % 4 for (w, h) in rnd} == {0, 1, 2, 3}
        dims = dims + rnd
        kinds = ["photo", "noise", "gray", "flat", "photo"]
        rasters = [synth_raster(kinds[i % len(kinds)], w, h, alpha, seed=i + 1) for i, (w, h) in enumerate(dims)]
        sp = dict(special_cases())
        extra = [po.normalize_rgba(sp["hidden_colour"]), sp["opaque_alpha"]] if alpha else [sp["mixed_tiles"], sp["gray_noise"]]
        rasters += [np.ascontiguousarray(r) for r in extra]
        dims = dims + [(r.shape[1], r.shape[0]) for r in extra]
        assert all(r.shape[2] == 3 + alpha for r in rasters)
        blobs = [po.encode_tiles(mode, r) for r in rasters]
        strip = [max(t[2] for t in po.tile_table(w, h, 3 + alpha)) <= 672 for (w, h) in dims]
        assert all(not strip[dims.index(d)] for d in WIDE_DIMS) and all(strip[dims.index(d)] for d in STRIP_DIMS)
        _BATCHES[key] = (dims, rasters, blobs, strip)
    return _BATCHES[key]


def _members(po, mode, alpha, which):
    dims, rasters, blobs, strip = _batch(po, mode, alpha)
    keep = [i for i in range(len(dims)) if which == "all" or strip[i]]
    return [dims[i] for i in keep], [rasters[i] for i in keep], [blobs[i] for i in keep]


def _blob_buffers(ctx):
    import torch
    return [torch.full((ctx.blob_bound(i) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for i in range(ctx.nimg)]


def _check_blobs(d_b, lens, want, what):
    import torch
    torch.cuda.synchronize()
    for i, (t, n, w) in enumerate(zip(d_b, lens, want)):
        got = t.cpu().numpy()
        assert n == len(w), (what, i, n, len(w))
        assert got[:n].tobytes() == w, (what, "blob", i)
        assert (got[n:] == SENTINEL).all(), (what, "bytes behind the returned length written", i)


def _encode_padded(ctx, mode, rasters, pad, fill):
    """padded form at a pitch `pad` bytes beyond the widest row; row padding and the 16 bytes behind the last row hold `fill`"""
    import torch
    ch = ctx.pxsz
    bpr = max(w for (w, h) in ctx.dims) * ch + pad
    d_r = []
    for r in rasters:
        h, w = r.shape[:2]
        rows = np.full((h * bpr + 16,), fill, dtype=np.uint8)
        rows[: h * bpr].reshape(h, bpr)[:, : w * ch] = r.reshape(h, w * ch)
        d_r.append(torch.from_numpy(rows).cuda())
    d_b = _blob_buffers(ctx)
    lens = ctx.encode_batch(mode, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b], in_bpr=bpr)
    return d_b, lens


def _encode_tight(ctx, mode, rasters, shift=0):
    """tight form; `shift` moves every raster off its 16-byte alignment"""
    import torch
    d_r = [torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), r.reshape(-1)])).cuda() for r in rasters]
    d_b = _blob_buffers(ctx)
    lens = ctx.encode_batch(mode, [t.data_ptr() + shift for t in d_r], [t.data_ptr() for t in d_b])
    return d_b, lens


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["all", "strip"])
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_padded_and_tight_forms_equal_the_oracle(gpu, po, monkeypatch, mode, alpha, which, form):
    """Blob i is the oracle's encode_tiles of raster i: padded form (twice, with different padding bytes), tight form (aligned and
    shifted by one byte), nothing written behind the returned lengths; the first tight call adds the staging raster to the
    workspace and later calls add nothing.  `strip` leaves out the images with a tile wider than 672 px."""
    monkeypatch.setenv(form, "1")
    dims, rasters, blobs = _members(po, mode, alpha, which)
    ch = 4 if alpha else 3
    ctx = gpu.MixedContext(dims, ch)
    try:
        ws0 = ctx.workspace_bytes()
        _check_blobs(*_encode_padded(ctx, mode, rasters, 52, 0x00), blobs, (mode, alpha, which, form, "padded"))
        ws1 = ctx.workspace_bytes()
        assert ws1 > ws0                                         # the encode workspace arrives with the first encode
        _check_blobs(*_encode_padded(ctx, mode, rasters, 52, 0xEE), blobs, (mode, alpha, which, form, "padded, other padding"))
        assert ctx.workspace_bytes() == ws1
        _check_blobs(*_encode_tight(ctx, mode, rasters), blobs, (mode, alpha, which, form, "tight"))
        pitch = -(-max(w for w, _ in dims) * ch // 16) * 16
        stage = sum(-(-h * pitch // 256) * 256 for (_, h) in dims)
        ws2 = ctx.workspace_bytes()
        assert ws1 + stage <= ws2 < ws1 + stage + (1 << 20)
        _check_blobs(*_encode_tight(ctx, mode, rasters, shift=1), blobs, (mode, alpha, which, form, "tight, shifted"))
        _check_blobs(*_encode_padded(ctx, mode, rasters, 0, 0x11), blobs, (mode, alpha, which, form, "padded, no slack"))
        assert ctx.workspace_bytes() == ws2
    finally:
        ctx.close()


def _decode_tight(ctx, mode, d_b, lens):
    import torch
    ch = ctx.pxsz
    d_o = [torch.full((h * w * ch + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for (w, h) in ctx.dims]
    ctx.decode_batch(mode, [t.data_ptr() for t in d_b], lens, [t.data_ptr() for t in d_o])
    assert ctx.decode_status() == 0
    torch.cuda.synchronize()
    out = []
    for (w, h), t in zip(ctx.dims, d_o):
        got = t.cpu().numpy()
        assert (got[h * w * ch:] == SENTINEL).all()
        out.append(got[: h * w * ch].reshape(h, w, ch))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_round_trip_on_one_context_in_both_orders(gpu, po, mode, alpha):
    """encode_batch then decode_batch on the same mixed context reproduces the rasters, and so does a context that decodes
    first: the shared scratch and staging buffers are sized for both."""
    dims, rasters, blobs = _members(po, mode, alpha, "all")
    ch = 4 if alpha else 3
    for first in ("encode", "decode"):
        ctx = gpu.MixedContext(dims, ch)
        try:
            if first == "decode":
                got = _decode_tight(ctx, mode, _upload(blobs), [len(b) for b in blobs])
                assert all(np.array_equal(g, r) for g, r in zip(got, rasters))
            d_b, lens = _encode_tight(ctx, mode, rasters)
            _check_blobs(d_b, lens, blobs, (mode, alpha, first, "encode"))
            got = _decode_tight(ctx, mode, d_b, lens)
            assert all(np.array_equal(g, r) for g, r in zip(got, rasters)), (mode, alpha, first)
            d_b, lens = _encode_padded(ctx, mode, rasters, 16, 0x33)
            _check_blobs(d_b, lens, blobs, (mode, alpha, first, "encode again"))
        finally:
            ctx.close()


@pytest.mark.gpu
def test_many_tiny_images_decode_first_then_encode(gpu, po):
    """700 RGBA images of 4..9 px per side: the stream scratch of an encode (about 6 KB per tile) is larger than the decode's
    planes here, so a context that decoded first re-allocates the shared buffer once - and still decodes afterwards."""
    from xpng_amd.synth import synth_raster
    rng = random.Random(5)
    dims = [(rng.randint(4, 9), rng.randint(4, 9)) for _ in range(700)]
    rasters = [synth_raster("photo" if i % 3 else "noise", w, h, True, seed=i) for i, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    ctx = gpu.MixedContext(dims, 4)
    try:
        got = _decode_tight(ctx, 1, _upload(blobs), [len(b) for b in blobs])
        assert all(np.array_equal(g, r) for g, r in zip(got, rasters))
        d_b, lens = _encode_tight(ctx, 1, rasters)
        _check_blobs(d_b, lens, blobs, "tiny")
        got = _decode_tight(ctx, 1, d_b, lens)
        assert all(np.array_equal(g, r) for g, r in zip(got, rasters))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_same_size_batch_equals_the_ordinary_batched_context(gpu, monkeypatch, mode, alpha, form):
    """A mixed context over 12 x 1500 x 1200 gives the bytes Context.encode_device_batch gives."""
    import torch
    from xpng_amd.synth import synth_raster_torch
    monkeypatch.setenv(form, "1")
    W, H, B = 1500, 1200, 12
    ch = 4 if alpha else 3
    uni = gpu.Context(W, H, ch, batch=B)
    mix = gpu.MixedContext([(W, H)] * B, ch)
    try:
        d_r = [synth_raster_torch("photo", W, H, alpha, seed=50 * mode + b) for b in range(B)]
        d_u = [torch.zeros(uni.blob_bound() + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
        lens = uni.encode_device_batch(mode, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_u])
        torch.cuda.synchronize()
        want = [t[:n].cpu().numpy().tobytes() for t, n in zip(d_u, lens)]
        assert all(mix.blob_bound(i) == uni.blob_bound() for i in range(B))
        d_p = [torch.cat([t.reshape(-1), torch.zeros(16, dtype=torch.uint8, device="cuda")]) for t in d_r]  # (16 readable bytes behind the last row)
        for in_bpr in (0, W * ch):
            d_m = _blob_buffers(mix)
            got = mix.encode_batch(mode, [t.data_ptr() for t in (d_p if in_bpr else d_r)], [t.data_ptr() for t in d_m], in_bpr=in_bpr, sync=False)
            assert got is None
            torch.cuda.synchronize()
            _check_blobs(d_m, [mix.last_blobs_len_at(i) for i in range(B)], want, (mode, alpha, form, in_bpr))
    finally:
        uni.close()
        mix.close()


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
            wide = 889 * ch
            d_r = [torch.from_numpy(np.ascontiguousarray(r).reshape(-1)).cuda() for r in rasters]
            d_p = [torch.zeros(h * wide + 16, dtype=torch.uint8, device="cuda") for (w, h) in dims]
            d_b = _blob_buffers(ctx)
            ins, pads, outs = [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_p], [t.data_ptr() for t in d_b]

            def refused(word, fn):
                with pytest.raises(gpu.XpngError) as e:
                    fn()
                assert word in str(e.value), (word, str(e.value))
                torch.cuda.synchronize()
                assert all(bool((t == SENTINEL).all()) for t in d_b), word

            refused("in_bpr", lambda: ctx.encode_batch(1, pads, outs, in_bpr=wide - 1))
            refused("nimg", lambda: ctx.encode_batch(1, ins[:2], outs[:2]))
            refused("tile mode", lambda: ctx.encode_batch(3, ins, outs))
            refused("null", lambda: ctx.encode_batch(1, ins, [outs[0], 0, outs[2]]))
            refused("null", lambda: ctx.encode_batch(1, [ins[0], 0, ins[2]], outs))
            refused("raster of image 0 must be 16-byte aligned", lambda: ctx.encode_batch(1, [pads[0] + 4] + pads[1:], outs, in_bpr=wide))
            refused("blob buffer of image 1 must be 4-byte aligned", lambda: ctx.encode_batch(1, ins, [outs[0], outs[1] + 2, outs[2]]))
            if ch == 4:
                refused("RGB only", lambda: ctx.encode_batch(2, ins, outs))
            plain = gpu.Context(700, 500, ch)
            try:
                vp = C.c_void_p
                assert lib.xpnghip_encode_varsize_device_batch(plain._h, 1, (vp * 1)(ins[0]), 0, 1, (vp * 1)(outs[0]), None, None) != 0
                assert "mixed context" in api._err()
                torch.cuda.synchronize()
                assert all(bool((t == SENTINEL).all()) for t in d_b)
            finally:
                plain.close()
            if ch == 4:                                          # an RGBA image 3 px wide in the batch
                narrow = gpu.MixedContext([(700, 500), (3, 200), (889, 445)], 4)
                try:
                    with pytest.raises(gpu.XpngError) as e:
                        narrow.encode_batch(1, ins, outs)
                    assert "narrower than 4 px" in str(e.value)
                    torch.cuda.synchronize()
                    assert all(bool((t == SENTINEL).all()) for t in d_b)
                finally:
                    narrow.close()
            lens = ctx.encode_batch(1, ins, outs)                # the context still encodes correctly afterwards
            _check_blobs(d_b, lens, blobs, ("after misuse", ch))
        finally:
            ctx.close()


def _store_list(po, manifest):
    """(name, raster) pairs of the staged-batch test"""
    from conftest import corpus_entries, corpus_raster
    from xpng_amd.synth import special_cases, synth_raster
    ents = [(n, e) for n, e in corpus_entries(manifest) if e["w"] * e["h"] <= 1_500_000]
    rgba = [x for x in ents if x[1]["ch"] == 4][:4]
    rgb = [x for x in ents if x[1]["ch"] == 3][:6]
    out = [(n, corpus_raster(e)) for n, e in rgb[:3] + rgba + rgb[3:]]
    sp = dict(special_cases())
    out += [("hidden_colour", sp["hidden_colour"]), ("opaque_alpha", sp["opaque_alpha"])]
    flat = synth_raster("flat", 300, 200, True); flat[..., 3] = 255
    out.append(("flat_opaque_rgba", flat))
    hidden = synth_raster("noise", 60, 50, True); hidden[..., 3] = 0
    out.append(("all_hidden", hidden))
    out += [("noise_rgb", synth_raster("noise", 200, 150, False)), ("noise_rgba_64", synth_raster("noise", 64, 64, True)),
            ("noise_rgba", synth_raster("noise", 200, 150, True)), ("thin_rgba", synth_raster("photo", 3, 50, True)),
            ("one_pixel", synth_raster("photo", 1, 1, True)), ("mixed_tiles", sp["mixed_tiles"])]
    return [(n, np.ascontiguousarray(r)) for n, r in out]


@pytest.mark.gpu
def test_store_batch_equals_store_and_the_oracle(gpu, po, manifest, tmp_path):
    """One list of RGB and RGBA rasters at levels 1, 2 and 7: file i is what xpng_store writes and what the oracle's encode_image
    gives; load_batch of the written files returns the normalised rasters."""
    items = _store_list(po, manifest)
    rasters = [r for _, r in items]
    assert {r.shape[2] for r in rasters} == {3, 4} and len(rasters) >= 18
    sizes = {}
    for level in (1, 2, 7):
        paths = [str(tmp_path / f"b{level}_{i}.xpng") for i in range(len(items))]
        gpu.store_batch(level, rasters, paths)
        for (name, r), p in zip(items, paths):
            got = open(p, "rb").read()
            one = str(tmp_path / "one.xpng")
            gpu.store(level, r, one)
            assert got == open(one, "rb").read(), (level, name, "xpng_store")
            if name != "thin_rgba" or level == 7:                # (RGBA narrower than 4 px: undefined in the reference below level 7)
                assert got == po.encode_image(level, r), (level, name, "oracle")
            sizes[(level, name)] = len(got)
        back = gpu.load_batch(paths)
        for (name, r), b in zip(items, back):
            want = po.normalize_rgba(r) if r.shape[2] == 4 else r
            assert b.shape == want.shape and np.array_equal(b, want), (level, name)
    assert sizes[(2, "flat_opaque_rgba")] == 11 and sizes[(2, "all_hidden")] == 12 and sizes[(1, "all_hidden")] == 64
    assert sizes[(1, "noise_rgb")] == 90008 and sizes[(1, "noise_rgba_64")] == 16392  # (rewritten to level 7: blen >= s)
    assert sizes[(1, "noise_rgba")] < 200 * 150 * 4 + 8


@pytest.mark.gpu
def test_staged_images_against_the_staged_image(gpu, po, manifest):
    """xpnghip_images_*: pixel sizes, single-colour flags, normalised rasters and tile blobs of a list equal the oracle's, the
    skipped entries stay None."""
    items = _store_list(po, manifest)[4:]
    rasters = [r for _, r in items]
    st = gpu.StagedImages(rasters)
    try:
        norm = [po.normalize_rgba(r) if r.shape[2] == 4 else r for r in rasters]
        assert st.pxsz == [n.shape[2] for n in norm]
        single = st.single_colour()
        assert single == [bool((n.reshape(-1, n.shape[2]) == n.reshape(-1, n.shape[2])[0]).all()) for n in norm]
        for i, n in enumerate(norm):
            assert np.array_equal(st.fetch(i), n), items[i][0]
            assert st.first_pixel(i) == n.reshape(-1)[: n.shape[2]].tobytes(), items[i][0]
        modes = [0 if (n.shape[2] == 4 and min(n.shape[:2]) < 4) or i % 5 == 4 else (2 if n.shape[2] == 3 and i % 2 else 1) for i, n in enumerate(norm)]
        blobs = st.encode(modes)
        for i, (m, n) in enumerate(zip(modes, norm)):
            assert blobs[i] is None if m == 0 else blobs[i] == po.encode_tiles(m, n), (items[i][0], m)
        with pytest.raises(gpu.XpngError):                       # mode 2 on an RGBA image: refused, nothing handed back
            st.encode([2 if n.shape[2] == 4 and min(n.shape[:2]) >= 4 else 0 for n in norm])
    finally:
        st.end()


@pytest.mark.gpu
def test_store_batch_splits_a_list_and_keeps_its_order(gpu, po, tmp_path):
    """30000 x 4 beside 4 x 24000: 24004 rows at 90000 bytes pass the 2 GiB of padded rasters a device call may hold, so the
    list becomes three staged batches (test_batch_cuts_follow_the_chunking_rule checks the cut points: [0, 2, 4]); the files keep
    their places and their bytes."""
    from xpng_amd.synth import synth_raster
    dims = [(64, 48), (30000, 4), (4, 24000), (100, 100), (30000, 4)]
    rasters = [synth_raster("photo", w, h, False, seed=i + 1) for i, (w, h) in enumerate(dims)]
    paths = [str(tmp_path / f"c{i}.xpng") for i in range(len(dims))]
    gpu.store_batch(1, rasters, paths)
    for r, p in zip(rasters, paths):
        assert open(p, "rb").read() == po.encode_image(1, r), r.shape
