"""GPU (-m gpu): tiles whose headers the parsers must reject, one per rejection rule of tests/_hostile.py, on the device.

Only REJECTED tiles go to a GPU: the module's fixture runs the text of k_dec_parse / k_m2_dec_parse on the host (tests/dec_parse_host.cpp,
as tests/test_dec_parse_host.py does, verdicts only) over the very blobs the tests upload and fails before any launch if one of them is
accepted there - so no kernel behind a parser ever runs on hostile bytes.  Each case is the MIDDLE tile of a three-tile photo with one
header field moved (systematic edits of _hostile.py on that tile; the tile's own size word stays wherever another edit reaches the
rule), one image per case, all images of a format in one launch with host-given tile offsets.  For mode 1 RGB, mode 1 RGBA and mode 2,
on the narrow and the forced-wide form, the launch reports status 1, leaves the bad tile's pixels at the sentinel, decodes every other
tile of every image like the oracle, writes nothing before or behind an image, and the same context then decodes the intact file
exactly with status 0."""
import numpy as np
import pytest

import _hostile as H
import _kit as K
from _kit import built, gpu, po  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def rejected(tmp_path_factory, po):
    """{(mode, pxsz): (oracle raster, file body, tile offsets, tile table, [case])} - every case rejected by the parsers' text on the host"""
    out, every = {}, []
    for mode, pxsz in H.FORMATS:
        raster, body, offs, _, picked = H.device_cases(po, mode, pxsz)
        W, Hh, table = H.device_raster(po, pxsz)
        want = po.decode_tiles(mode, body, W, Hh, pxsz)
        assert np.array_equal(want, raster)
        out[(mode, pxsz)] = (want, body, offs, table, picked)
        every += picked
    _, verdicts, _ = H.run_parsers_on_host(tmp_path_factory.mktemp("hostile"), H.Cases(), every, flags=("-DVERDICTS_ONLY",), sanitize=())
    accepted = [c.name for c in every if c.verdict != H.REJECT or verdicts[c.name]]
    assert not accepted, ("not sent to a GPU: accepted on the host", accepted)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["XPNG_NARROW_RANS", "XPNG_WIDE_RANS"])
@pytest.mark.parametrize("mode,pxsz", H.FORMATS)
def test_rejected_tiles_are_skipped_and_every_other_tile_is_exact(gpu, rejected, monkeypatch, mode, pxsz, form):
    monkeypatch.setenv(form, "1")
    want, body, offs, table, cases = rejected[(mode, pxsz)]
    assert len(table) >= 3 and 10 <= len(cases) <= 15
    Hh, W = want.shape[:2]
    B, t = len(cases), 1
    files = []
    for c in cases:
        assert len(c.blob) == offs[t + 1] - offs[t]
        files.append(body[:offs[t]] + c.blob + body[offs[t + 1]:])
        assert len(files[-1]) == len(body) and files[-1] != body
    ctx = gpu.Context(W, Hh, pxsz, batch=B)
    try:
        assert ctx.tiles() == [tuple(x) for x in table]
        arena = K.Arena([W * Hh * pxsz] * B, es=16, phases=1)       # (output rasters are 16-byte aligned)
        d_b = K._upload(files)
        ctx.decode_device_batch(mode, [x.data_ptr() for x in d_b], [len(f) for f in files], [offs] * B, arena.ptrs)
        assert ctx.decode_status() == 1
        x0, y0, tw, th = table[t]
        for c, g in zip(cases, arena.fetch()):                    # (fetch: every byte before and behind an image still holds the sentinel)
            g = g.reshape(Hh, W, pxsz)
            assert (g[y0:y0 + th, x0:x0 + tw] == K.SENTINEL).all(), (c.name, c.rule, "the rejected tile was written")
            keep = np.ones((Hh, W), bool)
            keep[y0:y0 + th, x0:x0 + tw] = False
            assert np.array_equal(g[keep], want[keep]), (c.name, c.rule, "another tile differs")
        # the single-image call on one bad file, then the intact file on the same context
        arena.refill()
        ctx.decode_device(mode, d_b[0].data_ptr(), len(files[0]), offs, arena.ptrs[0])
        assert ctx.decode_status() == 1
        g = arena.fetch([W * Hh * pxsz] + [0] * (B - 1))[0].reshape(Hh, W, pxsz)
        assert (g[y0:y0 + th, x0:x0 + tw] == K.SENTINEL).all() and np.array_equal(g[keep], want[keep])
        arena.refill()
        d_i = K._upload([body] * B)
        ctx.decode_device_batch(mode, [x.data_ptr() for x in d_i], [len(body)] * B, [offs] * B, arena.ptrs)
        assert ctx.decode_status() == 0
        for g in arena.fetch():
            assert np.array_equal(g.reshape(Hh, W, pxsz), want)
    finally:
        ctx.close()
