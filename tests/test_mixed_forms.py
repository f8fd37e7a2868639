"""Mixed batches: the forms of one direction share ONE table of per-image records on a context, cached on the caller's buffer
pointers (xpng_amd/csrc/xpng_hip.hip mixed_records; DESIGN.md 13 "The record table").  What sharing can break is a table that is
stale, or wrongly believed current, when the form or the buffers change between calls - so this runs the forms of each direction
in a fixed order over two buffer sets A and B on one context per format, and checks every byte of both sets after every call.

The checker is the oracle (blobs and rasters) and the rearrangement / float table of tests/_kit.py (those of
tests/test_layouts.py and tests/test_float_layouts.py); every comparison is bit-exact.  Both sets are kept as a host model of their whole device tensor: a
step writes its expectation into the model of its set, and afterwards BOTH device tensors must equal their models - the image
bytes, what earlier steps left beside them, the sentinels around every buffer, and the set the step did not touch.

An image's buffer has 16 * w * h bytes (4 channels of f32), or h rows at the padded step's pitch where that is more (the small
images beside a 700 px wide one), so the same pointers carry every form.  GPU only (-m gpu)."""
import numpy as np
import pytest

from _kit import F16, F32, FORMATS, GUARD, LEAD, SENTINEL, _upload, arrange, built, expect, gpu, mixed_consts, table
from xpng_amd import api

# rows shorter than a dword, rows and plane rows at every alignment, more than one block of rows, and one image of two tiles
RGB_DIMS = [(1, 1), (2, 1), (3, 3), (5, 7), (9, 4), (17, 4), (64, 64), (257, 17), (700, 500)]
RGBA_DIMS = [d for d in RGB_DIMS if min(d) >= 4]               # (RGBA under 4 px on a side is undefined in the reference)
PAD = 52                                                        # the padded step's pitch: the widest row and this


@pytest.fixture(scope="module")
def batches():
    """per (mode, alpha): dims, the oracle's tile blobs of seeded random pixels and its decode of them - computed once"""
    from oracle import pyoracle as po
    out = {}
    for mode, alpha in FORMATS:
        dims, px = (RGBA_DIMS, 4) if alpha else (RGB_DIMS, 3)
        rng = np.random.default_rng(20 + mode + 2 * alpha)
        pixels = [rng.integers(0, 256, (h, w, px), dtype=np.uint8) for (w, h) in dims]
        blobs = [po.encode_tiles(mode, r) for r in pixels]
        rasters = [po.decode_tiles(mode, b, w, h, px) for b, (w, h) in zip(blobs, dims)]
        assert all(np.array_equal(a, b) for a, b in zip(rasters, pixels))
        out[(mode, alpha)] = (dims, rasters, blobs)
    return out


@pytest.fixture(scope="module")
def contexts(gpu, batches):
    """one mixed context per format, shared by the decode and the encode sequence"""
    made = {}

    def get(mode, alpha):
        if (mode, alpha) not in made:
            dims = batches[(mode, alpha)][0]
            made[(mode, alpha)] = ctx = gpu.MixedContext(dims, 4 if alpha else 3)
            assert ctx.first_tile[-1] - ctx.first_tile[-2] == 2 and ctx.n_tiles == len(dims) + 1   # 700 x 500 splits in two
        return made[(mode, alpha)]

    yield get
    for ctx in made.values():
        ctx.close()


class BufferSet:
    """one device tensor with a 16-byte aligned buffer per image between sentinels, and the host model of all its bytes"""

    def __init__(self, sizes):
        import torch
        self.off, total = [], 0
        for n in sizes:
            self.off.append(total + LEAD)
            total += LEAD + -(-n // 16) * 16 + GUARD
        self.model = np.full(total, SENTINEL, np.uint8)
        self.t = torch.from_numpy(self.model.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptrs = [self.t.data_ptr() + o for o in self.off]

    def expect(self, i, data, pitch=None):
        """image i's buffer will hold `data` from its start on - or, with a pitch, one row of `data` every `pitch` bytes"""
        if pitch is None:
            flat = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            self.model[self.off[i]:self.off[i] + flat.size] = flat
        else:
            for y, row in enumerate(data.reshape(data.shape[0], -1)):
                self.model[self.off[i] + y * pitch:self.off[i] + y * pitch + row.size] = row

    def upload(self):
        """the model's bytes into the device tensor, in place: the same pointers carry another content"""
        import torch
        self.t.copy_(torch.from_numpy(self.model))

    def holds_model(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.t.cpu().numpy(), self.model)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_decode_forms_share_one_record_table(contexts, batches, mode, alpha):
    """tight, _as, _as_float and padded calls in turn over the sets A and B: every call writes what its form says into the set it
    was given and nothing else, whatever the call before it was; no form brings workspace of its own."""
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    ctx = contexts(mode, alpha)
    bpr = max(w for w, _ in dims) * px + PAD
    sets = {k: BufferSet([max(16 * w * h, h * bpr) for (w, h) in dims]) for k in "AB"}
    d_b, lens = _upload(blobs), [len(b) for b in blobs]
    ins = [t.data_ptr() for t in d_b]
    tabs = {dt: table(dt, *mixed_consts(dt)) for dt in (F16, F32)}

    def tight(s):
        ctx.decode_batch(mode, ins, lens, s.ptrs)
        for i, r in enumerate(rasters):
            s.expect(i, r)

    def padded(s):
        ctx.decode_batch(mode, ins, lens, s.ptrs, out_bpr=bpr)
        for i, r in enumerate(rasters):
            s.expect(i, r, pitch=bpr)

    def as_(planar, ch):
        def run(s):
            ctx.decode_batch_as(mode, ins, lens, s.ptrs, api.layout(planar=planar, bgr=True, channels=ch))
            for i, r in enumerate(rasters):
                s.expect(i, arrange(r, planar, True, ch or px))
        return run

    def as_float(dtype, planar):
        def run(s):
            scale, bias = mixed_consts(dtype)
            ctx.decode_batch_as_float(mode, ins, lens, s.ptrs, api.layout(planar=planar), dtype, scale[:px], bias[:px])
            for i, r in enumerate(rasters):
                s.expect(i, expect(r, planar, False, px, tabs[dtype]))
        return run

    steps = [(tight, "A"), (as_(True, 7 - px), "A"), (as_float(F16, False), "A"), (as_float(F32, True), "B"), (tight, "B"),
             (as_(False, 0), "B"), (tight, "A"), (padded, "A"), (tight, "A")]
    ws = []
    for n, (step, k) in enumerate(steps, 1):
        step(sets[k])
        assert ctx.decode_status() == 0, n
        assert sets[k].holds_model(), ("step", n, "the set it wrote")
        assert sets["AB".replace(k, "")].holds_model(), ("step", n, "the set it did not write")
        ws.append(ctx.workspace_bytes())
    assert ws[0] == ws[-1], ws                                    # every allocation of the decode path happened in step 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_encode_forms_share_one_record_table(contexts, batches, mode, alpha):
    """tight and _from calls in turn over the sets A and B, each set rewritten in place before its call: every blob is the
    oracle's, nothing is written behind the returned lengths, no input byte changes; no form brings workspace of its own."""
    import torch
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    ctx = contexts(mode, alpha)
    sets = {k: BufferSet([16 * w * h for (w, h) in dims]) for k in "AB"}
    bounds = [ctx.blob_bound(i) for i in range(ctx.nimg)]
    out = BufferSet(bounds)
    steps = [(None, "A"), ((True, True), "A"), ((False, True), "B"), (None, "B"), (None, "A")]
    ws = []
    for n, (form, k) in enumerate(steps, 1):
        s = sets[k]
        for i, r in enumerate(rasters):
            s.expect(i, arrange(r, *form, px) if form else r)
        s.upload()
        out.t.fill_(SENTINEL)
        if form:
            got = ctx.encode_batch_from(mode, s.ptrs, api.layout(planar=form[0], bgr=form[1]), out.ptrs)
        else:
            got = ctx.encode_batch(mode, s.ptrs, out.ptrs)
        assert got == [len(b) for b in blobs], n
        for i, b in enumerate(blobs):
            out.model[out.off[i]:out.off[i] + bounds[i]] = SENTINEL
            out.expect(i, np.frombuffer(b, np.uint8))
        assert out.holds_model(), ("step", n, "a blob differs from the oracle's, or a byte behind its length was written")
        assert sets["A"].holds_model() and sets["B"].holds_model(), ("step", n, "an input byte changed")
        ws.append(ctx.workspace_bytes())
    torch.cuda.synchronize()
    assert ws[0] == ws[-1], ws                                    # every allocation of the encode path happened in step 1
