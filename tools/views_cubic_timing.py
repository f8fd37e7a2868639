"""Bicubic views: a full decode plus torch's antialiased bicubic per view, against one cubic views call (GPU).  The protocol of
tools/views_colour_timing.py: HIP events on one stream, the legs interleaved round by round, 9 rounds
after 2 of warm-up, the blobs in HBM, and that tool's workload:

64 synthetic 'photo' RGBA rasters of seeded random sizes (512 .. 2048 px per side), level-1 blobs in HBM; two 224 x 224 views per
image from seeded random-resized-crop rectangles (area 8 % .. 100 %, aspect 3/4 .. 4/3), every other view flipped, planar C = 3
f16, the ImageNet constants, and one seeded colour-jitter matrix per view:
  a   what a caller has without the cubic call: one decode_batch_as_float of the whole batch into planar C = 3 f16 tensors (scale 1,
      bias 0), then per view a crop (a slice), F.interpolate(mode="bicubic", align_corners=False, antialias=True) to 224 x 224 and
      the flip, into two stacked tensors; then on them a clamp to 0 .. 255, the colour step (baddbmm), its clamp and the
      normalisation (addcmul), all in f16 as the tensors are
  b   one decode_batch_views_cubic with colours= and the ImageNet constants
  c   decode_batch_views with the triangle filter, colours= and the ImageNet constants: the call that must not have moved
Legs a and c use nothing newer than the views-colour call, so the tool also runs on a tree without the cubic call: --tree names the
checkout whose xpng_amd is imported (default: this one), and --legs a,c on the parent's tree is the yardstick.  Where
api.resample_cubic_host exists and --check is given, every view of one run is checked BEFORE any round is timed: leg b against it
on the bits, leg a to a grey level (its largest difference is printed, in units of the normalised output).  Where torch's GPU
build lacks the antialiased bicubic, leg a is dropped and the line says so.  Prints one JSON line: median GPU milliseconds per leg
with the min .. max of the rounds.

    python tools/views_cubic_timing.py [--tree DIR] [--legs a,b,c] [--check] [--batch 64] [--lo 512] [--hi 2048] [--iters 9] [--warmup 2] [--seed 1]
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=512)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    assert set(legs) <= {"a", "b", "c"}
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    from views_colour_timing import jitter_for
    from views_timing import MEAN, STD, crops_for

    import torch
    import torch.nn.functional as F
    import xpng_amd
    from xpng_amd import api
    from xpng_amd.synth import synth_raster_torch
    assert os.path.abspath(api.HIP_SO).startswith(tree + os.sep), api.HIP_SO

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
        if a.check:
            keep[b] = r.cpu().numpy().reshape(h, w, 4)                # the rasters the check reads
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
    fns, note = {}, {}
    if "a" in legs:
        full = [torch.empty((3, h, w), dtype=torch.float16, device="cuda") for (w, h) in dims]
        p_full = [t.data_ptr() for t in full]
        raw = [torch.empty((B, 3, S, S), dtype=torch.float16, device="cuda") for _ in range(2)]
        M16 = [torch.tensor(np.stack([m[:, :3] for m in mats[s * B:(s + 1) * B]]), dtype=torch.float16, device="cuda") for s in range(2)]
        K16 = [torch.tensor(np.stack([m[:, 3:] for m in mats[s * B:(s + 1) * B]]), dtype=torch.float16, device="cuda") for s in range(2)]
        sc16 = torch.tensor(scale, dtype=torch.float16, device="cuda").view(1, 3, 1)
        bi16 = torch.tensor(bias, dtype=torch.float16, device="cuda").view(1, 3, 1)

        def leg_a():
            mix.decode_batch_as_float(1, blobs, lens, p_full, planar3, f16, [1.0] * 3, [0.0] * 3, stream=sh)
            for s in range(2):
                for i in range(B):
                    x, y, w, h = sets[s][i]
                    v = F.interpolate(full[i][None, :, y:y + h, x:x + w], size=(S, S), mode="bicubic", align_corners=False, antialias=True)
                    raw[s][i].copy_(v[0].flip(2) if flips[s][i] else v[0])
                v = raw[s].view(B, 3, S * S).clamp_(0.0, 255.0)
                t = torch.baddbmm(K16[s], M16[s], v).clamp_(0.0, 255.0)
                torch.addcmul(bi16, t, sc16, out=res["a"][s].view(B, 3, S * S))
        try:                                                          # (a GPU build of torch without the antialiased bicubic raises here)
            with torch.cuda.stream(stream):
                F.interpolate(torch.zeros((1, 3, 9, 9), dtype=torch.float16, device="cuda"), size=(4, 4), mode="bicubic", align_corners=False, antialias=True)
            stream.synchronize()
            fns["a"] = leg_a
        except (RuntimeError, NotImplementedError) as e:
            note["a_unavailable"] = str(e).splitlines()[0][:200]
    if "b" in legs:
        def leg_b():
            mix.decode_batch_views_cubic(1, blobs, lens, vi, ptrs["b"], planar3, f16, vs, scale, bias, rects=vr, flips=vf, stream=sh, colours=mats)
        fns["b"] = leg_b
    if "c" in legs:
        def leg_c():
            mix.decode_batch_views(1, blobs, lens, vi, ptrs["c"], planar3, f16, vs, scale, bias, rects=vr, flips=vf, filter=AA, stream=sh, colours=mats)
        fns["c"] = leg_c

    # first the check, on one run of every leg: no round is timed for a leg that computes something else
    checked = {}
    with torch.cuda.stream(stream):
        for fn in fns.values():
            fn()
    stream.synchronize()
    assert mix.decode_status(sh) == 0
    if a.check and hasattr(api, "resample_cubic_host"):  # the rule, for every view
        worst, bits = 0.0, True
        for s in range(2):
            for i in range(B):
                v = s * B + i
                want = np.frombuffer(api.resample_cubic_host(keep[i], (S, S), planar3, f16, scale, bias, rect=vr[v], flip=bool(vf[v]), colour=mats[v]),
                                     np.float16).reshape(3, S, S)
                if "b" in fns:
                    bits = bits and np.array_equal(res["b"][s][i].cpu().numpy().view(np.uint16), want.view(np.uint16))
                if "a" in fns:
                    worst = max(worst, float(np.abs(res["a"][s][i].cpu().numpy().astype(np.float32) - want.astype(np.float32)).max()))
        if "b" in fns:
            checked["b_equals_the_rule"] = bool(bits)
        if "a" in fns:
            checked["a_largest_difference"] = round(worst, 5)
    assert checked.get("b_equals_the_rule", True), "leg b differs from the host rule"
    # leg a rounds to f16 where the rule keeps fp32 (the interpolated byte, the matrix product); a grey level of the normalised
    # output is 1 / (255 * 0.224) = 0.0175, and a wrong filter on 'photo' rasters is off by several
    assert checked.get("a_largest_difference", 0.0) <= 0.0175, "leg a is further from the host rule than a grey level"

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
    out = {"tool": "views_cubic_timing", "tree": os.path.basename(tree), "legs": list(fns), "dtype": "f16", "batch": B, "views": 2 * B, "level": 1,
           "sizes": f"{a.lo}..{a.hi}", "seed": a.seed, "iters": a.iters, "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "spread_ms": round(max(v) - min(v), 3)}
    assert mix.decode_status(sh) == 0
    out.update(checked)
    out.update(note)
    mix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
