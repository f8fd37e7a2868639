"""The workspace of a context (xpng_amd/csrc/common.hpp WsTable; include/xpng_hip.h xpnghip_ctx_workspace_bytes), on the GPU.

One ordinary context (700 x 500 RGB, batch 2: two 350 x 500 tiles per image, the smallest shape with more than one tile and a
batch) and one mixed context (700 x 500 and 64 x 48) run a level-1 and a level-2 encode and decode, each twice, in the narrow and
in the wide rANS form (XPNG_WIDE_RANS=1 reaches the wide level-2 tables at this size).  Every blob is the oracle's encode_tiles and
every decoded raster its input; workspace_bytes() rises with the first call of each kind that allocates - the first level-1 decode
among them: the decode's tables are counted - never falls, and is unchanged by the second call of each kind."""
import numpy as np
import pytest

from _kit import built, gpu, po, _upload

GUARD = 64
FORMS = [None, "XPNG_WIDE_RANS"]
_REF = {}


def _ref(po):
    """the rasters (two 700 x 500, one 64 x 48, RGB) and their oracle blobs per level, computed once"""
    if not _REF:
        from xpng_amd.synth import synth_raster
        rasters = [synth_raster("photo", 700, 500, False, seed=1), synth_raster("noise", 700, 500, False, seed=2),
                   synth_raster("photo", 64, 48, False, seed=3)]
        _REF.update(rasters=rasters, blobs={mode: [po.encode_tiles(mode, r) for r in rasters] for mode in (1, 2)})
    return _REF["rasters"], _REF["blobs"]


class _Meter:
    """workspace_bytes() after every call: it never falls; `rose` / `same` compare the last two readings"""

    def __init__(self, ctx):
        self.ctx, self.seen = ctx, [ctx.workspace_bytes()]

    def step(self, what):
        self.seen.append(self.ctx.workspace_bytes())
        assert self.seen[-1] >= self.seen[-2], (what, "the workspace fell", self.seen)

    def rose(self, what):
        self.step(what)
        assert self.seen[-1] > self.seen[-2], (what, "the first call of its kind added nothing", self.seen)

    def same(self, what):
        self.step(what)
        assert self.seen[-1] == self.seen[-2], (what, "a second call of its kind allocated", self.seen)


def _blobs_equal(d_b, lens, want, what):
    import torch
    torch.cuda.synchronize()
    for i, (t, n, w) in enumerate(zip(d_b, lens, want)):
        assert n == len(w) and t[:n].cpu().numpy().tobytes() == w, (what, "blob", i, n, len(w))


def _rasters_equal(d_o, rasters, what):
    import torch
    torch.cuda.synchronize()
    for i, (t, r) in enumerate(zip(d_o, rasters)):
        assert np.array_equal(t[: r.size].cpu().numpy(), r.reshape(-1)), (what, "raster", i)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_uniform_context_counts_everything_it_allocates(gpu, po, monkeypatch, form):
    import torch
    if form:
        monkeypatch.setenv(form, "1")
    rasters, blobs = _ref(po)
    rasters, blobs = rasters[:2], {m: b[:2] for m, b in blobs.items()}
    ctx = gpu.Context(700, 500, 3, batch=2)
    try:
        assert ctx.n_tiles == 2
        meter = _Meter(ctx)
        d_r = [torch.from_numpy(np.concatenate([r.reshape(-1), np.zeros(GUARD, np.uint8)])).cuda() for r in rasters]
        for mode in (1, 2):
            d_in = _upload(blobs[mode])
            for k, check in enumerate((meter.rose, meter.same)):
                d_b = [torch.zeros(ctx.blob_bound() + GUARD, dtype=torch.uint8, device="cuda") for _ in rasters]
                lens = ctx.encode_device_batch(mode, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
                _blobs_equal(d_b, lens, blobs[mode], (form, mode, "encode", k))
                check((form, mode, "encode", k))
            for k, check in enumerate((meter.rose if mode == 1 else meter.step, meter.same)):
                d_o = [torch.zeros(r.size + GUARD, dtype=torch.uint8, device="cuda") for r in rasters]
                ctx.decode_device_batch(mode, [t.data_ptr() for t in d_in], [len(b) for b in blobs[mode]], None, [t.data_ptr() for t in d_o])
                assert ctx.decode_status() == 0
                _rasters_equal(d_o, rasters, (form, mode, "decode", k))
                check((form, mode, "decode", k))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_mixed_context_decodes_first_then_encodes(gpu, po, monkeypatch, form):
    import torch
    if form:
        monkeypatch.setenv(form, "1")
    rasters, blobs = _ref(po)
    rasters, blobs = [rasters[0], rasters[2]], {m: [b[0], b[2]] for m, b in blobs.items()}
    ctx = gpu.MixedContext([(700, 500), (64, 48)], 3)
    try:
        meter = _Meter(ctx)
        d_r = [torch.from_numpy(r.reshape(-1).copy()).cuda() for r in rasters]
        for mode in (1, 2):
            d_in = _upload(blobs[mode])
            for k, check in enumerate((meter.rose if mode == 1 else meter.step, meter.same)):
                d_o = [torch.zeros(r.size + GUARD, dtype=torch.uint8, device="cuda") for r in rasters]
                ctx.decode_batch(mode, [t.data_ptr() for t in d_in], [len(b) for b in blobs[mode]], [t.data_ptr() for t in d_o])
                assert ctx.decode_status() == 0
                _rasters_equal(d_o, rasters, (form, mode, "decode", k))
                check((form, mode, "decode", k))
            for k, check in enumerate((meter.rose, meter.same)):
                d_b = [torch.zeros(ctx.blob_bound(i) + GUARD, dtype=torch.uint8, device="cuda") for i in range(ctx.nimg)]
                lens = ctx.encode_batch(mode, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
                _blobs_equal(d_b, lens, blobs[mode], (form, mode, "encode", k))
                check((form, mode, "encode", k))
    finally:
        ctx.close()
