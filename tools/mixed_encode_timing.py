"""Mixed-size batch encode against the per-image loop, one stream (GPU).  The encode sibling of tools/mixed_timing.py.

64 synthetic 'photo' RGBA rasters of seeded random sizes (256 .. 2048 px per side) lie in HBM; then, timed with HIP events on one
stream, interleaved round by round, level 1:
  mixed_padded : (a) one xpnghip_encode_varsize_device_batch call, every raster held at the pitch of the widest
  mixed_tight  : (b) one call, tight rasters (pack kernel + staging raster)
  loop         : (c) a batch-of-1 context per image, created beforehand, encoded one after another on the same stream
and a uniform-size control, 64 images of one size: the same rasters through a mixed context (tight, and padded at the exact pitch) and through the ordinary
batched context (xpnghip_encode_device_batch).  No call synchronises (blobs_len == NULL).
Prints one JSON line (median GPU milliseconds per batch, with the min .. max of the interleaved rounds).

    python tools/mixed_encode_timing.py [--batch 64] [--lo 256] [--hi 2048] [--uniform 1152] [--iters 9] [--warmup 2] [--seed 1]
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

    def blob(n):
        return torch.zeros(n + 64, dtype=torch.uint8, device="cuda")

    # ---- mixed sizes
    d_tight = [synth_raster_torch("photo", w, h, True, seed=b + 1).reshape(-1) for b, (w, h) in enumerate(dims)]
    bpr = max(w for w, _ in dims) * ch
    d_pad = []
    for (w, h), t in zip(dims, d_tight):
        p = torch.zeros(h * bpr + 16, dtype=torch.uint8, device="cuda")
        p[: h * bpr].view(h, bpr)[:, : w * ch] = t.view(h, w * ch)
        d_pad.append(p)
    mix = xpng_amd.MixedContext(dims, ch)
    ctxs = [xpng_amd.Context(w, h, ch) for (w, h) in dims]
    b_pad, b_tight, b_loop = ([blob(mix.blob_bound(i)) for i in range(B)] for _ in range(3))
    p_tight, p_pad = [t.data_ptr() for t in d_tight], [t.data_ptr() for t in d_pad]
    o_pad, o_tight, o_loop = ([t.data_ptr() for t in d] for d in (b_pad, b_tight, b_loop))

    def loop():
        for c, rp, op in zip(ctxs, p_tight, o_loop):
            c.encode_device(1, rp, op, stream=sh, sync=False)

    res = timed_interleaved({"mixed_padded": lambda: mix.encode_batch(1, p_pad, o_pad, in_bpr=bpr, stream=sh, sync=False),
                             "mixed_tight": lambda: mix.encode_batch(1, p_tight, o_tight, stream=sh, sync=False),
                             "loop": loop})
    torch.cuda.synchronize()
    total = 0
    for i in range(B):  # the three must agree before their times mean anything
        n = ctxs[i].last_blobs_len()
        assert n == mix.last_blobs_len_at(i) and torch.equal(b_loop[i][:n], b_tight[i][:n]) and torch.equal(b_loop[i][:n], b_pad[i][:n]), i
        total += n
    px = sum(w * h for w, h in dims)
    out = {"tool": "mixed_encode_timing", "batch": B, "pxsz": ch, "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed, "iters": a.iters,
           "megapixels": round(px / 1e6, 2), "tiles": mix.n_tiles, "blob_MB": round(total / 2**20, 1),
           "workspace_MB": round(mix.workspace_bytes() / 2**20, 1), **res,
           "loop_over_mixed_padded": round(res["loop"]["median_ms"] / res["mixed_padded"]["median_ms"], 2),
           "loop_over_mixed_tight": round(res["loop"]["median_ms"] / res["mixed_tight"]["median_ms"], 2),
           "slowest_mixed_round_faster_than_fastest_loop_round":
               max(res["mixed_padded"]["max_ms"], res["mixed_tight"]["max_ms"]) < res["loop"]["min_ms"]}
    mix.close()
    for c in ctxs:
        c.close()
    del d_pad, d_tight, b_pad, b_tight, b_loop

    # ---- uniform-size control
    U = a.uniform
    udims = [(U, U)] * B
    d_r = []
    for b in range(B):  # (16 readable bytes behind the last row: the padded form's contract)
        t = torch.zeros(U * U * ch + 16, dtype=torch.uint8, device="cuda")
        t[: U * U * ch] = synth_raster_torch("photo", U, U, True, seed=b + 1).reshape(-1)
        d_r.append(t)
    p_r = [t.data_ptr() for t in d_r]
    mix, uni = xpng_amd.MixedContext(udims, ch), xpng_amd.Context(U, U, ch, batch=B)
    b_m, b_u = ([blob(uni.blob_bound()) for _ in range(B)] for _ in range(2))
    o_m, o_u = [t.data_ptr() for t in b_m], [t.data_ptr() for t in b_u]
    ctl = timed_interleaved({"mixed": lambda: mix.encode_batch(1, p_r, o_m, stream=sh, sync=False),
                             "mixed_padded": lambda: mix.encode_batch(1, p_r, o_m, in_bpr=U * ch, stream=sh, sync=False),
                             "uniform": lambda: uni.encode_device_batch(1, p_r, o_u, stream=sh, sync=False)})
    torch.cuda.synchronize()
    for i in range(B):
        n = mix.last_blobs_len_at(i)
        assert n == xpng_amd.hip_lib().xpnghip_ctx_last_blobs_len_at(uni._h, i) and torch.equal(b_m[i][:n], b_u[i][:n]), i
    out["uniform_control"] = {"size": U, **ctl, "mixed_over_uniform": round(ctl["mixed"]["median_ms"] / ctl["uniform"]["median_ms"], 3),
                              "mixed_padded_over_uniform": round(ctl["mixed_padded"]["median_ms"] / ctl["uniform"]["median_ms"], 3)}
    mix.close(); uni.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
