"""The float decode against "decode to uint8, then let torch convert and normalise", one stream (GPU).  The protocol of
tools/layout_timing.py.

64 synthetic 'photo' RGBA rasters of seeded random sizes (256 .. 2048 px per side), level-1 blobs in HBM; every leg decodes the
batch to planar C = 3 tensors of the dtype, normalised with the ImageNet constants; timed with HIP events on one stream, the legs
interleaved round by round:
  a_<dtype>   the route without the float call: one decode_batch_as into uint8 tensors allocated once, then per image
              t.to(dtype) * scale.view(3, 1, 1) + bias.view(3, 1, 1), as a caller writes it (it allocates its results every round)
  b_<dtype>   one decode_batch_as_float into tensors allocated once
Leg a uses nothing newer than the layout calls, so the tool also runs in a checkout without the float call (--legs a): that line is
the yardstick b is compared against.  Prints one JSON line (median GPU milliseconds per batch with the min .. max of the rounds).
Leg b is also checked against leg a, loosely: a rounds its constants and both of its operations to the dtype, b rounds once (the
bit-exact check of b is tests/test_float_layouts.py).

    python tools/float_layout_timing.py [--legs a,b] [--dtypes f16,f32] [--batch 64] [--lo 256] [--hi 2048] [--iters 9] [--warmup 2] [--seed 1]
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--dtypes", default="f16,f32")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=256)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs, dtypes = a.legs.split(","), a.dtypes.split(",")
    assert set(legs) <= {"a", "b"} and set(dtypes) <= {"f16", "bf16", "f32"}

    import torch
    import xpng_amd
    from xpng_amd.synth import synth_raster_torch

    B = a.batch
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
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
    d_u8 = [torch.empty((3, h, w), dtype=torch.uint8, device="cuda") for (w, h) in dims]
    p_u8 = [t.data_ptr() for t in d_u8]
    fns, res_a, res_b = {}, {}, {}
    for name in dtypes:
        dt = tdt[name]
        if "a" in legs:
            t_scale, t_bias = torch.tensor(scale, dtype=dt, device="cuda"), torch.tensor(bias, dtype=dt, device="cuda")
            res_a[name] = [None] * B

            def leg_a(dt=dt, t_scale=t_scale, t_bias=t_bias, res=res_a[name]):
                mix.decode_batch_as(1, blobs, lens, p_u8, planar3, stream=sh)
                for i, t in enumerate(d_u8):
                    res[i] = t.to(dt) * t_scale.view(3, 1, 1) + t_bias.view(3, 1, 1)

            fns["a_" + name] = leg_a
        if "b" in legs:
            code = {"f16": xpng_amd.DTYPE_F16, "bf16": xpng_amd.DTYPE_BF16, "f32": xpng_amd.DTYPE_F32}[name]
            res_b[name] = [torch.empty((3, h, w), dtype=dt, device="cuda") for (w, h) in dims]
            p_b = [t.data_ptr() for t in res_b[name]]
            fns["b_" + name] = lambda code=code, p_b=p_b: mix.decode_batch_as_float(1, blobs, lens, p_b, planar3, code, scale, bias, stream=sh)

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
    out = {"tool": "float_layout_timing", "legs": legs, "dtypes": dtypes, "batch": B, "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed,
           "iters": a.iters, "megapixels": round(px / 1e6, 2)}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                  "spread_ms": round(max(v) - min(v), 3)}
    assert mix.decode_status(sh) == 0
    if "a" in legs and "b" in legs:  # the two must agree before their times mean anything
        ulp = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7, "f32": 2.0 ** -23}
        for name in dtypes:
            for x, y in zip(res_a[name], res_b[name]):
                x, y = x.double(), y.double()
                assert bool(((x - y).abs() <= 40 * ulp[name]).all()), name   # (|v * scale| and |bias| stay below 5)
    out["decode_workspace_MB"] = round(mix.workspace_bytes() / 2**20, 1)
    mix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
