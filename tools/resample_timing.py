"""The resampled decode (antialiased downscale) against "decode to full-size float tensors, then let torch crop, resize with
antialias=True, flip and stack", one stream (GPU).  The protocol of tools/resize_timing.py.

64 synthetic 'photo' RGBA rasters of seeded random sizes (256 .. 2048 px per side), level-1 blobs in HBM; every leg turns the batch
into ONE stacked (64, 3, 224, 224) tensor of the dtype, normalised with the ImageNet constants, from seeded random-resized-crop
rectangles with every other image flipped; timed with HIP events on one stream, the legs interleaved round by round:
  a_<dtype>   the route without the resampled call: one decode_batch_as_float into full-size planar tensors allocated once, then per
              image slice -> F.interpolate(..., mode="bilinear", antialias=True) in fp32 -> .flip(-1) where asked -> cast -> copy
              into the stacked tensor, as a caller writes it
  b_<dtype>   one decode_batch_resampled with FILTER_TRIANGLE_AA into the stacked tensor
  r_<dtype>   (with leg b) the existing decode_batch_resized, 2 x 2 taps, for scale
Leg a uses nothing newer than the float call, so the tool also runs unchanged in a checkout without the resampled call (--legs a):
that line is the yardstick b is compared against.  Prints one JSON line (median GPU milliseconds per batch with the min .. max of
the rounds).  Leg b is also checked against leg a, loosely: a filters the normalised dtype values in fp32 and rounds twice, b filters
the bytes and rounds once (the bit-exact check of b is tests/test_resample.py).

    python tools/resample_timing.py [--legs a,b] [--dtypes f16,f32] [--batch 64] [--lo 256] [--hi 2048] [--size 224] [--iters 9] [--warmup 2] [--seed 1]
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
    """random-resized-crop rectangles from the tool's own seeded generator (so the tool needs nothing newer than the float call)"""
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
    ap.add_argument("--dtypes", default="f16,f32")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=256)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs, dtypes = a.legs.split(","), a.dtypes.split(",")
    assert set(legs) <= {"a", "b"} and set(dtypes) <= {"f16", "bf16", "f32"}

    import torch
    import torch.nn.functional as F
    import xpng_amd
    from xpng_amd.synth import synth_raster_torch

    B, S = a.batch, a.size
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    rects = crops_for(dims, rng)
    flips = [i % 2 for i in range(B)]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
    codes = {"f16": xpng_amd.DTYPE_F16, "bf16": xpng_amd.DTYPE_BF16, "f32": xpng_amd.DTYPE_F32}
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
    torch.cuda.synchronize()
    blobs = [t.data_ptr() for t in d_b]
    mix = xpng_amd.MixedContext(dims, 4)
    planar3 = xpng_amd.layout(planar=True, channels=3)
    fns, res_a, res_b = {}, {}, {}
    for name in dtypes:
        dt = tdt[name]
        full = [torch.empty((3, h, w), dtype=dt, device="cuda") for (w, h) in dims]
        p_full = [t.data_ptr() for t in full]
        if "a" in legs:
            res_a[name] = torch.empty((B, 3, S, S), dtype=dt, device="cuda")

            def leg_a(code=codes[name], p_full=p_full, full=full, res=res_a[name]):
                mix.decode_batch_as_float(1, blobs, lens, p_full, planar3, code, scale, bias, stream=sh)
                for i, (t, (x, y, w, h)) in enumerate(zip(full, rects)):
                    o = F.interpolate(t[:, y:y + h, x:x + w].float()[None], size=(S, S), mode="bilinear", align_corners=False, antialias=True)[0]
                    if flips[i]:
                        o = o.flip(-1)
                    res[i].copy_(o.to(res.dtype))

            fns["a_" + name] = leg_a
        if "b" in legs:
            res_b[name] = torch.empty((B, 3, S, S), dtype=dt, device="cuda")
            p_b = [res_b[name][i].data_ptr() for i in range(B)]
            fns["b_" + name] = lambda code=codes[name], p_b=p_b: mix.decode_batch_resampled(1, blobs, lens, p_b, planar3, code, (S, S), scale, bias,
                                                                                             rects=rects, flips=flips, filter=xpng_amd.FILTER_TRIANGLE_AA, stream=sh)
            res_r = torch.empty((B, 3, S, S), dtype=dt, device="cuda")
            p_r = [res_r[i].data_ptr() for i in range(B)]
            fns["r_" + name] = lambda code=codes[name], p_r=p_r, keep=res_r: mix.decode_batch_resized(1, blobs, lens, p_r, planar3, code, (S, S), scale, bias,
                                                                                                     rects=rects, flips=flips, stream=sh)

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
    out = {"tool": "resample_timing", "legs": legs, "dtypes": dtypes, "batch": B, "level": 1, "sizes": f"{a.lo}..{a.hi}", "out": S, "seed": a.seed,
           "iters": a.iters, "megapixels": round(px / 1e6, 2), "crop_megapixels": round(sum(r[2] * r[3] for r in rects) / 1e6, 2)}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                  "spread_ms": round(max(v) - min(v), 3)}
    assert mix.decode_status(sh) == 0
    if "a" in legs and "b" in legs:  # the two must agree before their times mean anything
        # a filters values already rounded to the dtype (|y| < 3) and rounds again; b rounds once.  f32: torch's device kernel
        # normalises the weights of a window before it sums and filters the normalised values, so the bound is a coarse one: 1 / 64
        # of one byte step at the largest scale, 1 / (255 * 0.224), rounded down to a power of two.  A wrong window, weight or
        # half-pixel convention is off by whole byte steps.
        tol = {"f16": 2 * 2.0 ** -9, "bf16": 2 * 2.0 ** -6, "f32": 2.0 ** -12}
        for name in dtypes:
            d = (res_a[name].double() - res_b[name].double()).abs().max().item()
            out["max_abs_diff_" + name] = d
            out["agree"] = out.get("agree", True) and d <= tol[name]
    out["decode_workspace_MB"] = round(mix.workspace_bytes() / 2**20, 1)
    mix.close()
    print(json.dumps(out))
    assert out.get("agree", True), "legs a and b disagree"


if __name__ == "__main__":
    main()
