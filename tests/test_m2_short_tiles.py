"""Level-2 tiles shorter than 8 bytes: a raw gray tile is 4 + w * h bytes (reference libxpng.c:875-878), so an image of two or
three gray pixels has a tile of 6 or 7 bytes, and a 1 x 3 file stays at level 2 (7 bytes against 9 raw).  The tile parser of the
decode has to accept them on every path: the ordinary context, the host-buffer call, the mixed context in both output forms."""
import numpy as np
import pytest

from _kit import built

SHAPES = [(1, 3), (3, 1), (1, 2), (2, 1)]


def _gray(w, h):
    v = (np.arange(w * h, dtype=np.uint8) * 37 + 11).reshape(h, w, 1)
    return np.ascontiguousarray(np.repeat(v, 3, axis=2))


def test_the_oracle_writes_raw_gray_tiles_shorter_than_8_bytes():
    from oracle import pyoracle as po
    for (w, h) in SHAPES:
        r = _gray(w, h)
        blob = po.encode_tiles(2, r)
        assert len(blob) == 4 + w * h < 8 and blob[3] >> 4 == 2 and blob[3] & 8, (w, h, blob.hex())
        assert np.array_equal(po.decode_tiles(2, blob, w, h, 3), r)
    data = po.encode_image(2, _gray(1, 3))
    assert data[3] == 2 and len(data) == 8 + 7                   # the 1 x 3 file stays at level 2


@pytest.mark.gpu
def test_short_level2_tiles_decode_on_every_path():
    import torch
    import xpng_amd
    from oracle import pyoracle as po
    if not torch.cuda.is_available() or xpng_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    rasters = [_gray(w, h) for (w, h) in SHAPES]
    blobs = [po.encode_tiles(2, r) for r in rasters]
    d_b = [torch.from_numpy(np.frombuffer(b + b"\0" * 64, dtype=np.uint8).copy()).cuda() for b in blobs]
    for (w, h), r, b, t in zip(SHAPES, rasters, blobs, d_b):
        ctx = xpng_amd.Context(w, h, 3)
        try:
            for offs in ([0], None):                             # host-given offset, device-side walk
                out = torch.zeros(h * w * 3 + 64, dtype=torch.uint8, device="cuda")
                ctx.decode_device(2, t.data_ptr(), len(b), offs, out.data_ptr())
                assert ctx.decode_status() == 0, (w, h, offs)
                assert np.array_equal(out[: h * w * 3].cpu().numpy().reshape(h, w, 3), r), (w, h, offs)
        finally:
            ctx.close()
        assert np.array_equal(xpng_amd.decode_tiles(2, b, w, h, 3), r), (w, h)
    mix = xpng_amd.MixedContext(SHAPES, 3)
    try:
        lens, ins = [len(b) for b in blobs], [t.data_ptr() for t in d_b]
        tight = [torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda") for (w, h) in SHAPES]
        mix.decode_batch(2, ins, lens, [t.data_ptr() for t in tight])
        assert mix.decode_status() == 0
        bpr = 16
        padded = [torch.zeros(h * bpr, dtype=torch.uint8, device="cuda") for (w, h) in SHAPES]
        mix.decode_batch(2, ins, lens, [t.data_ptr() for t in padded], out_bpr=bpr)
        assert mix.decode_status() == 0
        for (w, h), r, a, p in zip(SHAPES, rasters, tight, padded):
            assert np.array_equal(a.cpu().numpy().reshape(h, w, 3), r), (w, h)
            assert np.array_equal(p.cpu().numpy().reshape(h, bpr)[:, : w * 3].reshape(h, w, 3), r), (w, h)
    finally:
        mix.close()
    path_r = _gray(1, 3)
    import tempfile, os
    with tempfile.TemporaryDirectory() as tmp:                   # and the file, through xpng_load
        fn = os.path.join(tmp, "g.xpng")
        with open(fn, "wb") as f:
            f.write(po.encode_image(2, path_r))
        assert np.array_equal(xpng_amd.load(fn), path_r)
