"""Layout calls against "code the tight form, then let torch rearrange", one stream (GPU).  The protocol of tools/mixed_timing.py.

64 synthetic 'photo' rasters of seeded random sizes (256 .. 2048 px per side), blobs in HBM; timed with HIP events on one stream,
the legs interleaved round by round:
  a   today's route to planar RGB from an RGBA level-1 batch: one tight mixed decode, then per image
      t.view(h, w, 4).permute(2, 0, 1)[:3].contiguous() (which allocates its result every round; b writes into tensors allocated once)
  b   one decode_batch_as call, planar, C = 3, on the same blobs
  c   layout 0 against the tight call (informational: both run k_mixed_copy)
  da  today's route from planar RGB tensors into a level-1 RGB encode: per image hwc.copy_(t.permute(1, 2, 0)) into a buffer
      allocated once, then one tight mixed encode
  db  one encode_batch_from call, planar, on the same tensors
Legs a and da use nothing newer than the mixed-size batch calls, so the tool also runs in a checkout without the layout calls
(--legs a,da): that line is the yardstick b and db are compared against.  Prints one JSON line (median GPU milliseconds per batch
with the min .. max of the rounds).

    python tools/layout_timing.py [--legs a,b,c,da,db] [--batch 64] [--lo 256] [--hi 2048] [--iters 9] [--warmup 2] [--seed 1]
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
    ap.add_argument("--legs", default="a,b,c,da,db")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lo", type=int, default=256)
    ap.add_argument("--hi", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    legs = a.legs.split(",")
    assert set(legs) <= {"a", "b", "c", "da", "db"}

    import torch
    import xpng_amd
    from xpng_amd.synth import synth_raster_torch

    B = a.batch
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

    px = sum(w * h for w, h in dims)
    out = {"tool": "layout_timing", "legs": legs, "batch": B, "level": 1, "sizes": f"{a.lo}..{a.hi}", "seed": a.seed, "iters": a.iters,
           "megapixels": round(px / 1e6, 2)}

    # ---- decode: an RGBA level-1 batch -> planar RGB
    if set(legs) & {"a", "b", "c"}:
        ch = 4
        d_b, lens = [], []
        for b, (w, h) in enumerate(dims):
            c = xpng_amd.Context(w, h, ch)
            r = synth_raster_torch("photo", w, h, True, seed=b + 1)
            t = torch.empty(c.blob_bound() + 64, dtype=torch.uint8, device="cuda")
            lens.append(c.encode_device(1, r.data_ptr(), t.data_ptr()))
            d_b.append(t)
            c.close()
        torch.cuda.synchronize()
        blobs = [t.data_ptr() for t in d_b]
        mix = xpng_amd.MixedContext(dims, ch)
        d_tight = [torch.empty(h * w * ch, dtype=torch.uint8, device="cuda") for (w, h) in dims]
        p_tight = [t.data_ptr() for t in d_tight]
        res_a = [None] * B
        fns = {}

        def leg_a():
            mix.decode_batch(1, blobs, lens, p_tight, stream=sh)
            for i, ((w, h), t) in enumerate(zip(dims, d_tight)):
                res_a[i] = t.view(h, w, 4).permute(2, 0, 1)[:3].contiguous()

        if "a" in legs:
            fns["a_tight_then_permute"] = leg_a
        if "b" in legs:
            planar3 = xpng_amd.layout(planar=True, channels=3)
            d_chw = [torch.empty((3, h, w), dtype=torch.uint8, device="cuda") for (w, h) in dims]
            p_chw = [t.data_ptr() for t in d_chw]
            fns["b_decode_as_planar_rgb"] = lambda: mix.decode_batch_as(1, blobs, lens, p_chw, planar3, stream=sh)
        if "c" in legs:
            d_l0 = [torch.empty(h * w * ch, dtype=torch.uint8, device="cuda") for (w, h) in dims]
            p_l0 = [t.data_ptr() for t in d_l0]
            fns["c_tight"] = lambda: mix.decode_batch(1, blobs, lens, p_tight, stream=sh)
            fns["c_layout_0"] = lambda: mix.decode_batch_as(1, blobs, lens, p_l0, 0, stream=sh)
        out.update(timed_interleaved(fns))
        assert mix.decode_status(sh) == 0
        if "a" in legs and "b" in legs:  # the two must agree before their times mean anything
            assert all(torch.equal(x, y) for x, y in zip(res_a, d_chw))
        if "c" in legs:
            assert all(torch.equal(x, y) for x, y in zip(d_tight, d_l0))
        out["decode_workspace_MB"] = round(mix.workspace_bytes() / 2**20, 1)
        mix.close()
        del d_b, d_tight, res_a

    # ---- encode: planar RGB tensors -> an RGB level-1 batch
    if set(legs) & {"da", "db"}:
        ch = 3
        d_chw = [synth_raster_torch("photo", w, h, False, seed=b + 1).view(h, w, 3).permute(2, 0, 1).contiguous() for b, (w, h) in enumerate(dims)]
        mix = xpng_amd.MixedContext(dims, ch)
        d_o1 = [torch.empty(mix.blob_bound(i) + 64, dtype=torch.uint8, device="cuda") for i in range(B)]
        d_o2 = [torch.empty(mix.blob_bound(i) + 64, dtype=torch.uint8, device="cuda") for i in range(B)]
        p_o1, p_o2 = [t.data_ptr() for t in d_o1], [t.data_ptr() for t in d_o2]
        p_chw = [t.data_ptr() for t in d_chw]
        keep = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for (w, h) in dims]  # (allocated once: the pointers stay)
        p_keep = [t.data_ptr() for t in keep]
        fns = {}

        def leg_da():
            for k, t in zip(keep, d_chw):
                k.copy_(t.permute(1, 2, 0))
            mix.encode_batch(1, p_keep, p_o1, stream=sh, sync=False)

        if "da" in legs:
            fns["da_permute_then_tight"] = leg_da
        if "db" in legs:
            planar = xpng_amd.layout(planar=True)
            fns["db_encode_from_planar_rgb"] = lambda: mix.encode_batch_from(1, p_chw, planar, p_o2, stream=sh, sync=False)
        out.update(timed_interleaved(fns))
        torch.cuda.synchronize()
        if "da" in legs and "db" in legs:
            for i in range(B):
                n = mix.last_blobs_len_at(i)
                assert torch.equal(d_o1[i][:n], d_o2[i][:n]), i
        out["encode_workspace_MB"] = round(mix.workspace_bytes() / 2**20, 1)
        mix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
