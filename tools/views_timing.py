"""One views call against one resampled call per view set, one stream (GPU).  The protocol of tools/resize_timing.py (DESIGN.md 17,
20): HIP events on one stream, the legs interleaved round by round, 9 rounds after 2 of warm-up, the blobs in HBM.

64 synthetic 'photo' RGBA rasters of seeded random sizes (512 .. 2048 px per side), level-1 blobs in HBM; every leg writes planar
C = 3 f16 tensors normalised with the ImageNet constants from seeded random-resized-crop rectangles (area 8 % .. 100 % of the image
for the 224 x 224 views, 5 % .. 14 % for the 96 x 96 ones, aspect 3/4 .. 4/3), every other view flipped, filter 1:
  a1   one decode_batch_resampled, one 224 x 224 view per image           b1   one decode_batch_views, the same views
  a2   two decode_batch_resampled, two 224 x 224 views per image          b2   one decode_batch_views, the same views
  a10  ten decode_batch_resampled: 2 x 224 x 224 and 8 x 96 x 96          b10  one decode_batch_views, the same views
a1 / b1 isolates the skipped tiles (the copy-out writes the same bytes); a2 / b2 and a10 / b10 add the entropy decodes that one call
per view set repeats.  The a legs use nothing newer than the resampled call, so the tool also runs in a checkout without the views
call (--legs a): that line is the yardstick.  Prints one JSON line: median GPU milliseconds per leg with the min .. max of the
rounds, and for every b leg the share of the table's tiles its launch held (last_decode_tiles / M).  Every b leg is compared with
its a leg on the bits before the times mean anything.

    python tools/views_timing.py [--legs a,b] [--batch 64] [--lo 512] [--hi 2048] [--iters 9] [--warmup 2] [--seed 1]
"""
import argparse
import json
import math
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def crops_for(dims, rng, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """random-resized-crop rectangles from the tool's own seeded generator (so the tool needs nothing newer than the resampled call)"""
    out = []
    for (W, H) in dims:
        rect = None
        for _ in range(10):
            target = W * H * rng.uniform(*scale)
            aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                rect = (rng.randint(0, W - w), rng.randint(0, H - h), w, h)
                break
        out.append(rect or (0, 0, W, H))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=512)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    assert set(legs) <= {"a", "b"}

    import torch
    import xpng_amd
    from xpng_amd.synth import synth_raster_torch

    B = a.batch
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    # ten view sets: one rectangle per image each; sets 0 and 1 at 224 x 224, sets 2 .. 9 at 96 x 96
    sets = [crops_for(dims, rng) for _ in range(2)] + [crops_for(dims, rng, scale=(0.05, 0.14)) for _ in range(8)]
    sizes = [224, 224] + [96] * 8
    flips = [[(i + s) % 2 for i in range(B)] for s in range(10)]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    scale = [1.0 / (255.0 * s) for s in STD]
    bias = [-m / s for m, s in zip(MEAN, STD)]

    d_b, lens = [], []
    for b, (w, h) in enumerate(dims):
        c = xpng_amd.Context(w, h, 4)
        r = synth_raster_torch("photo", w, h, True, seed=b + 1)
        t = torch.empty(c.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        lens.append(c.encode_device(1, r.data_ptr(), t.data_ptr()))
        d_b.append(t)
        c.close()
        del r
    torch.cuda.synchronize()
    blobs = [t.data_ptr() for t in d_b]
    mix = xpng_amd.MixedContext(dims, 4)
    planar3, f16, AA = xpng_amd.layout(planar=True, channels=3), xpng_amd.DTYPE_F16, xpng_amd.FILTER_TRIANGLE_AA
    fns, res, share = {}, {}, {}
    for n in (1, 2, 10):
        for leg in legs:
            res[leg, n] = [torch.empty((B, 3, sizes[s], sizes[s]), dtype=torch.float16, device="cuda") for s in range(n)]
        if "a" in legs:
            p_a = [[t[i].data_ptr() for i in range(B)] for t in res["a", n]]

            def leg_a(n=n, p_a=p_a):
                for s in range(n):
                    mix.decode_batch_resampled(1, blobs, lens, p_a[s], planar3, f16, (sizes[s], sizes[s]), scale, bias, rects=sets[s], flips=flips[s],
                                               filter=AA, stream=sh)
            fns["a%d" % n] = leg_a
        if "b" in legs:
            # view s * B + i is view set s of image i
            vi = [i for s in range(n) for i in range(B)]
            ptrs = [res["b", n][s][i].data_ptr() for s in range(n) for i in range(B)]
            vs = [(sizes[s], sizes[s]) for s in range(n) for i in range(B)]
            vr = [sets[s][i] for s in range(n) for i in range(B)]
            vf = [flips[s][i] for s in range(n) for i in range(B)]
            share["b%d" % n] = len(xpng_amd.view_tiles(dims, vi, vr)) / mix.n_tiles

            def leg_b(vi=vi, ptrs=ptrs, vs=vs, vr=vr, vf=vf):
                mix.decode_batch_views(1, blobs, lens, vi, ptrs, planar3, f16, vs, scale, bias, rects=vr, flips=vf, filter=AA, stream=sh)
            fns["b%d" % n] = leg_b

    ms = {k: [] for k in fns}
    tiles = {}
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
            if hasattr(mix, "last_decode_tiles"):
                tiles[k] = mix.last_decode_tiles()
    px = sum(w * h for w, h in dims)
    out = {"tool": "views_timing", "legs": legs, "dtype": "f16", "batch": B, "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed, "iters": a.iters,
           "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles,
           "crop_share_224": round(sum(r[2] * r[3] for r in sets[0]) / px, 3)}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                  "spread_ms": round(max(v) - min(v), 3)}
        if k in tiles:
            out[k]["tiles_over_M"] = round(tiles[k] / mix.n_tiles, 3)
            assert k not in share or abs(share[k] - tiles[k] / mix.n_tiles) < 1e-12
    assert mix.decode_status(sh) == 0
    if "a" in legs and "b" in legs:  # the two must agree, on the bits, before their times mean anything
        out["agree"] = all(torch.equal(x, y) for n in (1, 2, 10) for x, y in zip(res["a", n], res["b", n]))
    out["decode_workspace_MB"] = round(mix.workspace_bytes() / 2**20, 1)
    mix.close()
    print(json.dumps(out))
    assert out.get("agree", True), "legs a and b disagree"


if __name__ == "__main__":
    main()
