"""Tone views: one tone views call against what a caller has without it - the same call with tones=NULL into un-normalised f32
planes, then torch's own operations per step (aminmax; a histogram, cumsum and gather; floor; where) and the normalisation (GPU).
The protocol of tools/views_blur_timing.py: HIP events on one stream, the legs interleaved round by round,
9 rounds after 2 of warm-up, the blobs in HBM.

The workload is the BYOL / DINO loader of tools/views_blur_timing.py: B synthetic 'photo' RGBA rasters of seeded random sizes (512 ..
2048 px per side), level-1 blobs in HBM; per image two global views of 224 x 224 and eight local views of 96 x 96, every other view
flipped, bicubic, planar C = 3, the ImageNet constants, one seeded colour-jitter matrix per view, the blur and solarise records of
that tool - and on top tensors.random_tone(V, num_ops=2): two steps per view out of autocontrast, equalise, posterise and solarise.
  a   one decode_batch_views_tone with filter 2, colours=, blurs= and tones=None into two stacked f32 tensors, planar, scale 1 and
      bias 0 (the blur call itself); then per stack and per step index the views of each operation are gathered, put through torch
      - aminmax per plane; one bincount over all planes at once (kinder than a histc per plane), cumsum and gather; floor; where -
      and scattered back; then the normalisation (addcmul) into f16
  b   one decode_batch_views_tone with the same arguments, tones= and the ImageNet constants into f16
With --check, before any round is timed, 24 views of leg b are compared with api.resample_tone_host on the bits and every view of
leg a with leg b (the largest difference is printed, in units of the normalised output; an equalise bin that a 1-ulp difference of
the order of summation moves shows there).  Prints one JSON line: median GPU milliseconds per leg with the min .. max of the rounds.

    python tools/views_tone_timing.py [--legs a,b] [--check] [--batch 32] [--lo 512] [--hi 2048] [--iters 9] [--warmup 2] [--seed 1]
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
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lo", type=int, default=512)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    assert set(legs) <= {"a", "b"}
    tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    from views_colour_timing import jitter_for
    from views_timing import MEAN, STD, crops_for

    import torch
    import xpng_amd
    from xpng_amd import api, tensors
    from xpng_amd.synth import synth_raster_torch

    B = a.batch
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    groups = [(2, 224, 23, (0.4, 1.0)), (8, 96, 9, (0.05, 0.4))]
    vi, vs, vr, vf, sig, sol = [], [], [], [], [], []
    for (n, S, ks, sc) in groups:
        for s in range(n):
            rects = crops_for(dims, rng, scale=sc)
            for i in range(B):
                vi.append(i); vs.append((S, S)); vr.append(rects[i]); vf.append((i + s) % 2)
                p = (1.0, 0.1)[s] if S == 224 else 0.5
                sig.append(rng.uniform(0.1, 2.0) if rng.random() < p else None)
                sol.append(128.0 if S == 224 and s == 1 and rng.random() < 0.2 else None)
    V = len(vi)
    mats = jitter_for(V, rng)
    taps = [ks for (n, S, ks, _) in groups for _ in range(n * B)]
    blurs = [None if sg is None and so is None else (sg or 0.0, taps[v] // 2 if sg is not None else 0, so) for v, (sg, so) in enumerate(zip(sig, sol))]
    tones = [tensors._tone_steps("t", t) for t in tensors.random_tone(V, num_ops=2, generator=torch.Generator().manual_seed(a.seed))]
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
            keep[b] = r.cpu().numpy().reshape(h, w, 4)
        del r
    torch.cuda.synchronize()
    blobs = [t.data_ptr() for t in d_b]
    mix = xpng_amd.MixedContext(dims, 4)
    planar3, f16, f32 = xpng_amd.layout(planar=True, channels=3), xpng_amd.DTYPE_F16, xpng_amd.DTYPE_F32
    spans, at = [], 0
    for (n, S, ks, _) in groups:
        spans.append((at, at + n * B, S, ks))
        at += n * B
    res = {leg: [torch.empty((e - s, 3, S, S), dtype=torch.float16, device="cuda") for (s, e, S, _) in spans] for leg in legs}
    ptrs = {leg: [res[leg][g][k].data_ptr() for g, (s, e, _, _) in enumerate(spans) for k in range(e - s)] for leg in legs}
    common = dict(rects=vr, flips=vf, filter=api.FILTER_CUBIC_AA, stream=sh, colours=mats, blurs=blurs)
    fns = {}
    if "a" in legs:
        raw = [torch.empty((e - s, 3, S, S), dtype=torch.float32, device="cuda") for (s, e, S, _) in spans]
        p_raw = [raw[g][k].data_ptr() for g, (s, e, _, _) in enumerate(spans) for k in range(e - s)]
        # per stack and step index: {op: (the views' indices in the stack, their args as (n, 1, 1, 1))}
        plans = []
        for (s, e, S, _) in spans:
            plan = []
            for j in range(2):
                by = {}
                for v in range(s, e):
                    if tones[v] is not None and j < len(tones[v]):
                        by.setdefault(tones[v][j][0], []).append((v - s, tones[v][j][1]))
                plan.append({op: (torch.tensor([k for k, _ in lst], device="cuda"),
                                  torch.tensor([2.0 ** (8 - x) if op == api.TONE_POSTERISE else x for _, x in lst], dtype=torch.float32, device="cuda").view(-1, 1, 1, 1))
                             for op, lst in by.items()})
            plans.append(plan)
        sc32 = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
        bi32 = torch.tensor(bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)

        def torch_step(y, op, arg):
            n, S = y.shape[0], y.shape[2]
            if op == api.TONE_AUTOCONTRAST:
                lo, hi = torch.aminmax(y.view(n * 3, -1), dim=1)
                lo, hi = lo.view(n, 3, 1, 1), hi.view(n, 3, 1, 1)
                return torch.where(hi > lo, ((y - lo) * (255.0 / (hi - lo))).clamp_max(255.0), y)
            if op == api.TONE_EQUALISE:
                P = n * 3
                idx = y.round().long().view(P, -1)
                h = torch.bincount((idx + 256 * torch.arange(P, device=y.device).view(P, 1)).view(-1), minlength=256 * P).view(P, 256)
                last = ((h > 0) * torch.arange(256, device=y.device)).amax(dim=1, keepdim=True)
                step = (S * S - h.gather(1, last)) // 255
                lut = ((step // 2 + h.cumsum(1) - h) // step.clamp_min(1)).clamp_max(255).float()
                return torch.where((step > 0).view(n, 3, 1, 1), lut.gather(1, idx).view_as(y), y)
            if op == api.TONE_POSTERISE:
                return torch.floor(y / arg) * arg
            if op == api.TONE_SOLARISE:
                return torch.where(y >= arg, 255.0 - y, y)
            return 255.0 - y

        def leg_a():
            mix.decode_batch_views_tone(1, blobs, lens, vi, p_raw, planar3, f32, vs, [1.0] * 3, [0.0] * 3, tones=None, **common)
            for g in range(len(spans)):
                x = raw[g].clamp(0.0, 255.0)
                for step in plans[g]:
                    for op, (idx, arg) in step.items():
                        x.index_copy_(0, idx, torch_step(x.index_select(0, idx), op, arg))
                res["a"][g].copy_(torch.addcmul(bi32, x, sc32))
        fns["a"] = leg_a
    if "b" in legs:
        def leg_b():
            mix.decode_batch_views_tone(1, blobs, lens, vi, ptrs["b"], planar3, f16, vs, scale, bias, tones=tones, **common)
        fns["b"] = leg_b

    checked = {}
    with torch.cuda.stream(stream):
        for fn in fns.values():
            fn()
    stream.synchronize()
    assert mix.decode_status(sh) == 0
    if a.check:
        def view(leg, v):
            g = next(k for k, (s, e, _, _) in enumerate(spans) if s <= v < e)
            return res[leg][g][v - spans[g][0]].cpu().numpy()
        if "b" in fns:
            bits = True
            for v in range(0, V, max(V // 24, 1)):
                want = np.frombuffer(api.resample_tone_host(keep[vi[v]], vs[v], planar3, f16, scale, bias, rect=vr[v], flip=bool(vf[v]), filter=api.FILTER_CUBIC_AA,
                                                            colour=mats[v], blur=blurs[v], tone=tones[v]), np.uint16)
                bits = bits and np.array_equal(view("b", v).view(np.uint16).reshape(-1), want)
            checked["b_equals_the_rule"] = bool(bits)
        if "a" in fns and "b" in fns:
            checked["a_b_largest_difference"] = round(max(float(np.abs(view("a", v).astype(np.float32) - view("b", v).astype(np.float32)).max()) for v in range(V)), 5)
    assert checked.get("b_equals_the_rule", True), "leg b differs from the host rule"

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
    steps = [s[0] for t in tones if t for s in t]
    out = {"tool": "views_tone_timing", "legs": list(fns), "dtype": "f16", "batch": B, "views": V, "tone_views": sum(t is not None for t in tones),
           "steps": {name: steps.count(op) for name, op in tensors._TONE_OPS.items() if steps.count(op)}, "blurred": sum(s is not None for s in sig),
           "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed, "iters": a.iters, "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles,
           "workspace_bytes": mix.workspace_bytes()}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "spread_ms": round(max(v) - min(v), 3)}
    assert mix.decode_status(sh) == 0
    out.update(checked)
    mix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
