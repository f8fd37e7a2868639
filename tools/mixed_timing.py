"""Mixed-size batch decode against the per-image loop, one stream (GPU).

64 synthetic 'photo' RGBA rasters of seeded random sizes (256 .. 2048 px per side) are encoded at level 1 into HBM; then, timed
with HIP events on one stream, interleaved round by round:
  mixed_padded : (a) one xpnghip_decode_mixed_device_batch launch, every image at the pitch of the widest
  mixed_tight  : (b) one launch, tight rasters (staging raster + per-image copy)
  loop         : (c) a batch-of-1 context per image, created beforehand, decoded one after another on the same stream
and a uniform-size control, 64 images of one size: the same blobs through a mixed context (tight) and through the ordinary
batched context (xpnghip_decode_device_batch: tile-major, split into two size classes).  All use the device-side size walk.
Prints one JSON line (median GPU milliseconds per batch, with the min .. max of the interleaved rounds).

    python tools/mixed_timing.py [--batch 64] [--lo 256] [--hi 2048] [--uniform 1152] [--iters 9] [--warmup 2] [--seed 1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=256)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--uniform", type=int, default=1152)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch
    import xpng_amd
    from xpng_amd.synth import synth_raster_torch

    B, ch = a.batch, 4
    rng = random.Random(a.seed)
    dims = [(rng.randint(a.lo, a.hi), rng.randint(a.lo, a.hi)) for _ in range(B)]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream

    def encode(dims_):
        """a batch-of-1 context per image (kept: the per-image loop decodes with them), its blob in HBM, its length"""
        ctxs, d_b, lens = [], [], []
        for b, (w, h) in enumerate(dims_):
            c = xpng_amd.Context(w, h, ch)
            r = synth_raster_torch("photo", w, h, True, seed=b + 1)
            t = torch.empty(c.blob_bound() + 64, dtype=torch.uint8, device="cuda")
            lens.append(c.encode_device(1, r.data_ptr(), t.data_ptr()))
            ctxs.append(c); d_b.append(t)
        torch.cuda.synchronize()
        return ctxs, d_b, lens

    def timed_interleaved(fns):
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
        return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}

    # ---- mixed sizes
    ctxs, d_b, lens = encode(dims)
    blobs = [t.data_ptr() for t in d_b]
    mix = xpng_amd.MixedContext(dims, ch)
    bpr = max(w for w, _ in dims) * ch
    d_pad = [torch.empty(h * bpr, dtype=torch.uint8, device="cuda") for (_, h) in dims]
    d_tight = [torch.empty(h * w * ch, dtype=torch.uint8, device="cuda") for (w, h) in dims]
    d_loop = [torch.empty(h * w * ch + 64, dtype=torch.uint8, device="cuda") for (w, h) in dims]
    p_pad, p_tight, p_loop = ([t.data_ptr() for t in d] for d in (d_pad, d_tight, d_loop))

    def loop():
        for c, bp, n, op in zip(ctxs, blobs, lens, p_loop):
            c.decode_device(1, bp, n, None, op, stream=sh)

    res = timed_interleaved({"mixed_padded": lambda: mix.decode_batch(1, blobs, lens, p_pad, out_bpr=bpr, stream=sh),
                             "mixed_tight": lambda: mix.decode_batch(1, blobs, lens, p_tight, stream=sh),
                             "loop": loop})
    assert mix.decode_status(sh) == 0 and all(c.decode_status(sh) == 0 for c in ctxs)
    for (w, h), t, p, l in zip(dims, d_tight, d_pad, d_loop):  # the three must agree before their times mean anything
        assert torch.equal(t, l[: h * w * ch]) and torch.equal(p.view(h, bpr)[:, : w * ch].reshape(-1), t), (w, h)
    px = sum(w * h for w, h in dims)
    out = {"tool": "mixed_timing", "batch": B, "pxsz": ch, "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed, "iters": a.iters,
           "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles, "workspace_MB": round(mix.workspace_bytes() / 2**20, 1), **res,
           "loop_over_mixed_padded": round(res["loop"]["median_ms"] / res["mixed_padded"]["median_ms"], 2),
           "loop_over_mixed_tight": round(res["loop"]["median_ms"] / res["mixed_tight"]["median_ms"], 2)}
    mix.close()
    for c in ctxs:
        c.close()
    del d_pad, d_tight, d_loop, d_b

    # ---- uniform-size control
    U = a.uniform
    udims = [(U, U)] * B
    ctxs, d_b, lens = encode(udims)
    for c in ctxs:
        c.close()
    blobs = [t.data_ptr() for t in d_b]
    mix, uni = xpng_amd.MixedContext(udims, ch), xpng_amd.Context(U, U, ch, batch=B)
    d_m = [torch.empty(U * U * ch, dtype=torch.uint8, device="cuda") for _ in range(B)]
    d_u = [torch.empty(U * U * ch + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
    p_m, p_u = [t.data_ptr() for t in d_m], [t.data_ptr() for t in d_u]
    ctl = timed_interleaved({"mixed": lambda: mix.decode_batch(1, blobs, lens, p_m, stream=sh),
                             "uniform": lambda: uni.decode_device_batch(1, blobs, lens, None, p_u, stream=sh)})
    assert mix.decode_status(sh) == 0 and uni.decode_status(sh) == 0
    assert all(torch.equal(m, u[: U * U * ch]) for m, u in zip(d_m, d_u))
    out["uniform_control"] = {"size": U, **ctl, "mixed_over_uniform": round(ctl["mixed"]["median_ms"] / ctl["uniform"]["median_ms"], 3)}
    mix.close(); uni.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
