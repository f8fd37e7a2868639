"""A colour jitter per view: one views call plus a torch colour step, against one views call with colour matrices (GPU).  The
protocol of tools/views_timing.py: HIP events on one stream, the legs interleaved round by round, 9 rounds
after 2 of warm-up, the blobs in HBM.

64 synthetic 'photo' RGBA rasters of seeded random sizes (512 .. 2048 px per side), level-1 blobs in HBM; two 224 x 224 views per
image from seeded random-resized-crop rectangles (area 8 % .. 100 %, aspect 3/4 .. 4/3), every other view flipped, filter 1, planar
C = 3 f16, the ImageNet constants, and one seeded colour-jitter matrix per view (brightness, contrast and saturation 0.4, hue 0.1,
p = 0.8, grayscale with 0.2: tensors.random_colour_jitter's recipe, restated here from the tool's own generator so that the tool
needs nothing newer than the views call):
  a   what a caller has without the colour call: one decode_batch_views with scale 1 and bias 0 into two stacked tensors, then the
      colour step in torch on them - a batched 3 x 3 matmul plus the constant (baddbmm), a clamp to 0 .. 255 and the normalisation
      (addcmul), all in f16 as the tensors are
  b   one decode_batch_views with colours= and the ImageNet constants
  c   the plain decode_batch_views with the ImageNet constants: the call that must not have moved
Leg a uses nothing newer than the views call, so the tool also runs in a checkout without the colour call (--legs a, or a,c): that
line is the yardstick.  Where api.resample_colour_host exists, every view of one run of every leg is checked BEFORE any round is
timed: leg b against it on the bits, leg a to f16 rounding (its largest difference is printed, in units of the normalised output,
and must stay within four f16 steps of it).  Prints one JSON line: median GPU milliseconds per leg with the min .. max of the rounds.

    python tools/views_colour_timing.py [--legs a,b,c] [--batch 64] [--lo 512] [--hi 2048] [--iters 9] [--warmup 2] [--seed 1]
"""
import argparse
import json
import math
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from views_timing import MEAN, STD, crops_for  # noqa: E402


def jitter_for(n, rng, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, gray_p=0.2):
    """n (3, 4) float32 matrices: tensors.colour_matrix's composition (brightness, contrast about 127.5, saturation, a hue rotation
    about the gray axis) in float64, rounded once"""
    luma = np.array([[0.299, 0.587, 0.114]])
    K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])

    def matrix(b, c, s, h):
        M = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1) * b * c
        M[:, 3] += (1.0 - c) * 127.5
        M = (s * np.eye(3) + (1.0 - s) * np.ones((3, 1)) * luma) @ M
        co, si = math.cos(2.0 * math.pi * h), math.sin(2.0 * math.pi * h)
        return (co * np.eye(3) + (1.0 - co) / 3.0 * np.ones((3, 3)) + si / math.sqrt(3.0) * K) @ M

    out = []
    for _ in range(n):
        u = [rng.random() for _ in range(6)]
        span = lambda x, r: max(0.0, 1.0 - r) + (1.0 + r - max(0.0, 1.0 - r)) * x   # noqa: E731
        M = matrix(span(u[1], brightness), span(u[2], contrast), span(u[3], saturation), (2.0 * u[4] - 1.0) * hue) if u[0] < p else matrix(1.0, 1.0, 1.0, 0.0)
        if u[5] < gray_p:
            M = (np.ones((3, 1)) * luma) @ M
        out.append(M.astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=512)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    assert set(legs) <= {"a", "b", "c"}

    import torch
    import xpng_amd
    from xpng_amd import api
    from xpng_amd.synth import synth_raster_torch

    B, S = a.batch, 224
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    sets = [crops_for(dims, rng) for _ in range(2)]
    flips = [[(i + s) % 2 for i in range(B)] for s in range(2)]
    mats = jitter_for(2 * B, rng)                                     # view s * B + i is view set s of image i
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
    planar3, f16, AA = xpng_amd.layout(planar=True, channels=3), xpng_amd.DTYPE_F16, xpng_amd.FILTER_TRIANGLE_AA
    vi = [i for s in range(2) for i in range(B)]
    vs = [(S, S)] * (2 * B)
    vr = [sets[s][i] for s in range(2) for i in range(B)]
    vf = [flips[s][i] for s in range(2) for i in range(B)]
    res = {leg: [torch.empty((B, 3, S, S), dtype=torch.float16, device="cuda") for _ in range(2)] for leg in legs}
    ptrs = {leg: [res[leg][s][i].data_ptr() for s in range(2) for i in range(B)] for leg in legs}
    fns = {}
    if "a" in legs:
        raw = [torch.empty((B, 3, S * S), dtype=torch.float16, device="cuda") for _ in range(2)]
        p_raw = [raw[s][i].data_ptr() for s in range(2) for i in range(B)]
        M16 = [torch.tensor(np.stack([m[:, :3] for m in mats[s * B:(s + 1) * B]]), dtype=torch.float16, device="cuda") for s in range(2)]
        K16 = [torch.tensor(np.stack([m[:, 3:] for m in mats[s * B:(s + 1) * B]]), dtype=torch.float16, device="cuda") for s in range(2)]
        sc16 = torch.tensor(scale, dtype=torch.float16, device="cuda").view(1, 3, 1)
        bi16 = torch.tensor(bias, dtype=torch.float16, device="cuda").view(1, 3, 1)

        def leg_a():
            mix.decode_batch_views(1, blobs, lens, vi, p_raw, planar3, f16, vs, [1.0] * 3, [0.0] * 3, rects=vr, flips=vf, filter=AA, stream=sh)
            for s in range(2):
                y = torch.baddbmm(K16[s], M16[s], raw[s]).clamp_(0.0, 255.0)
                torch.addcmul(bi16, y, sc16, out=res["a"][s].view(B, 3, S * S))
        fns["a"] = leg_a
    if "b" in legs:
        def leg_b():
            mix.decode_batch_views(1, blobs, lens, vi, ptrs["b"], planar3, f16, vs, scale, bias, rects=vr, flips=vf, filter=AA, stream=sh, colours=mats)
        fns["b"] = leg_b
    if "c" in legs:
        def leg_c():
            mix.decode_batch_views(1, blobs, lens, vi, ptrs["c"], planar3, f16, vs, scale, bias, rects=vr, flips=vf, filter=AA, stream=sh)
        fns["c"] = leg_c

    # first the check, on one run of every leg: no round is timed for a leg that computes something else
    checked = {}
    with torch.cuda.stream(stream):
        for fn in fns.values():
            fn()
    stream.synchronize()
    assert mix.decode_status(sh) == 0
    if hasattr(api, "resample_colour_host"):  # the rule, for every view
        worst, bits = 0.0, True
        for s in range(2):
            for i in range(B):
                v = s * B + i
                want = np.frombuffer(api.resample_colour_host(keep[i], (S, S), planar3, f16, scale, bias, rect=vr[v], flip=bool(vf[v]), filter=AA,
                                                              colour=mats[v]), np.float16).reshape(3, S, S)
                if "b" in legs:
                    bits = bits and np.array_equal(res["b"][s][i].cpu().numpy().view(np.uint16), want.view(np.uint16))
                if "a" in legs:
                    worst = max(worst, float(np.abs(res["a"][s][i].cpu().numpy().astype(np.float32) - want.astype(np.float32)).max()))
        if "b" in legs:
            checked["b_equals_the_rule"] = bool(bits)
        if "a" in legs:
            checked["a_largest_difference"] = round(worst, 5)
    assert checked.get("b_equals_the_rule", True), "leg b differs from the host rule"
    # leg a rounds to f16 three times where the rule rounds once: the resampled byte (up to 1/16 of a byte unit below 256) through
    # rows whose entries sum to about 2, the product (1/16 again), together 3/16 of a byte unit times the largest scale, 1 / (255 *
    # 0.224): 0.0033; then the output's own half step and the rule's.  The output stays below 4, where a step is 2^-9: four steps
    assert checked.get("a_largest_difference", 0.0) <= 4 * 2.0 ** -9, "leg a is further from the host rule than f16 rounding"

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
    out = {"tool": "views_colour_timing", "legs": legs, "dtype": "f16", "batch": B, "views": 2 * B, "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed,
           "iters": a.iters, "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles, "tiles_over_M": round(mix.last_decode_tiles() / mix.n_tiles, 3)}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "spread_ms": round(max(v) - min(v), 3)}
    assert mix.decode_status(sh) == 0
    out.update(checked)
    out["decode_workspace_MB"] = round(mix.workspace_bytes() / 2**20, 1)
    mix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
