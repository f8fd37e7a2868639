"""An affine map per view: the two lane mappings of k_mixed_views_affine on rotated views, and an identity-matrix call beside the
views-colour call on the same rectangles (GPU).  The protocol of tools/views_colour_timing.py: HIP events on
one stream, the legs interleaved round by round, 9 rounds after 2 of warm-up, the blobs in HBM.

`--batch` synthetic 'photo' RGBA rasters of seeded random sizes (512 .. 2048 px per side), level-1 blobs in HBM; two 224 x 224 views
per image from seeded square rectangles of 224 * zoom pixels a side (zoom 1: the warp samples the source at its own resolution, where
the slant of a wave's reads is all that differs between the mappings; zoom 2: a shrinking map), bilinear, planar C = 3 f16, the
ImageNet constants, fill 0:
  patch45 / row45   every view turned by 45 degrees about its centre: the product's mapping (a wave covers 4 output rows x 16 stores)
                    and the siblings' (a wave walks one output row), which only the probes library has (XPNG_AFFINE_ROW_MAP)
  patch90 / row90   every view turned by 90 degrees: a wave's output row is a source column
  ident             the crop-resize matrices of the rectangles: the affine kernel with nothing to turn
  colour            decode_batch_views with identity colour matrices and filter 0 on the same rectangles: k_mixed_views_colour
Every view of one run of every affine leg is checked against api.resample_affine_host on the bits BEFORE any round is timed.  The
event times are whole calls - the decode of the touched tiles and the copy-out - so the tool is also run once per pair of legs under
`rocprofv3 --kernel-trace --stats` for the time of the copy-out kernel alone (profiles/views_affine_timing.txt has both).  Prints
one JSON line: median GPU milliseconds per leg with the min .. max of the rounds.

    python tools/views_affine_timing.py [--legs patch45,row45,...] [--zoom 1.0] [--batch 32] [--iters 9] [--warmup 2] [--seed 1]
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from views_timing import MEAN, STD  # noqa: E402

LEGS = ("patch45", "row45", "patch90", "row90", "ident", "colour")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--zoom", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lo", type=int, default=512)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    assert set(legs) <= set(LEGS) and 0.25 <= a.zoom <= 2.0
    os.environ["XPNG_USE_PROBES_LIB"] = "1"                          # the row mapping exists in the probes library only
    os.environ.pop("XPNG_AFFINE_ROW_MAP", None)

    import torch
    import xpng_amd
    from xpng_amd import api, tensors
    from xpng_amd.synth import synth_raster_torch

    B, S = a.batch, 224
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    side = int(round(S * a.zoom))
    rects = [(rng.randint(0, w - side), rng.randint(0, h - side), side, side) for _ in range(2) for (w, h) in dims]   # view s * B + i
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    scale = [1.0 / (255.0 * s) for s in STD]
    bias = [-m / s for m, s in zip(MEAN, STD)]

    d_b, lens, keep = [], [], {}
    for b, (w, h) in enumerate(dims):
        c = xpng_amd.Context(w, h, 4)
        r = synth_raster_torch("photo", w, h, True, seed=b + 1)
        t = torch.empty(c.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        lens.append(c.encode_device(1, r.data_ptr(), t.data_ptr()))
        d_b.append(t)
        c.close()
        keep[b] = r.cpu().numpy().reshape(h, w, 4)                    # the rasters the check reads
        del r
    torch.cuda.synchronize()
    blobs = [t.data_ptr() for t in d_b]
    mix = xpng_amd.MixedContext(dims, 4)
    planar3, f16 = xpng_amd.layout(planar=True, channels=3), xpng_amd.DTYPE_F16
    vi = [i for s in range(2) for i in range(B)]
    vs = [(S, S)] * (2 * B)
    mats = {"45": [tensors.affine_matrix(r, (S, S), angle=45.0) for r in rects], "90": [tensors.affine_matrix(r, (S, S), angle=90.0) for r in rects],
            "ident": [tensors.affine_matrix(r, (S, S)) for r in rects]}
    eye = [api.COLOUR_IDENTITY] * (2 * B)
    res = {leg: torch.empty((2 * B, 3, S, S), dtype=torch.float16, device="cuda") for leg in legs}
    ptrs = {leg: [res[leg][v].data_ptr() for v in range(2 * B)] for leg in legs}

    def affine_leg(leg, which, row):
        def fn():
            if row:
                os.environ["XPNG_AFFINE_ROW_MAP"] = "1"
            try:
                mix.decode_batch_views_affine(1, blobs, lens, vi, ptrs[leg], planar3, f16, vs, mats[which], scale, bias, filter=api.FILTER_BILINEAR, stream=sh)
            finally:
                os.environ.pop("XPNG_AFFINE_ROW_MAP", None)
        return fn

    def colour_leg():
        mix.decode_batch_views(1, blobs, lens, vi, ptrs["colour"], planar3, f16, vs, scale, bias, rects=rects, filter=api.FILTER_BILINEAR, stream=sh, colours=eye)

    which = {"patch45": ("45", False), "row45": ("45", True), "patch90": ("90", False), "row90": ("90", True), "ident": ("ident", False)}
    fns = {leg: colour_leg if leg == "colour" else affine_leg(leg, *which[leg]) for leg in legs}

    # first the check, on one run of every leg: no round is timed for a leg that computes something else
    tiles = {}
    for leg, fn in fns.items():
        with torch.cuda.stream(stream):
            fn()
        stream.synchronize()
        assert mix.decode_status(sh) == 0
        tiles[leg] = round(mix.last_decode_tiles() / mix.n_tiles, 3)
    for leg in legs:
        if leg == "colour":
            continue
        got = res[leg].cpu().numpy().view(np.uint16)
        for v in range(2 * B):
            want = np.frombuffer(api.resample_affine_host(keep[vi[v]], (S, S), mats[which[leg][0]][v], planar3, f16, scale, bias), np.uint16).reshape(3, S, S)
            assert np.array_equal(got[v], want), f"leg {leg} differs from the host rule in view {v}"

    ms = {k: [] for k in fns}
    for it in range(a.warmup + a.iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn()
                e1.record(stream)
            e1.synchronize()
            if it >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    px = sum(w * h for w, h in dims)
    out = {"tool": "views_affine_timing", "legs": legs, "zoom": a.zoom, "dtype": "f16", "batch": B, "views": 2 * B, "level": 1, "sizes": f"{a.lo}..{a.hi}",
           "seed": a.seed, "iters": a.iters, "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles, "tiles_over_M": tiles, "affine_legs_equal_the_rule": True}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "spread_ms": round(max(v) - min(v), 3)}
    assert mix.decode_status(sh) == 0
    mix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
