"""Device tensors -> .xpng files: the path a caller had before tensors.store_files against one store_files call (GPU).

64 synthetic 'photo' RGB images of seeded random, corpus-like sizes (352 .. 1600 x 200 .. 1100) lie in HBM as planar float16 tensors
in 0 .. 1, what a model writes.  Timed with the wall clock between two device-wide synchronisations, interleaved round by round,
files written to a fresh temporary directory, level 1:
  torch_then_store_batch : (a) per image (t.float() * 255).round().clamp(0, 255).to(uint8).permute(1, 2, 0).contiguous().cpu(),
                               then ONE api.store_batch of the host rasters (which uploads them again): only code the parent has
  store_files            : (b) ONE tensors.store_files call on the list
The two legs must write the same bytes before their times mean anything (torch.round rounds half to even, as the rule does).
Prints one JSON line: median and min .. max milliseconds per batch of the rounds, and whether (b) is no slower than (a) by more than
the larger spread (max - min) of the two legs.

    python tools/store_tensors_timing.py [--batch 64] [--iters 7] [--warmup 1] [--seed 1] [--level 1]
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--level", type=int, default=1)
    a = ap.parse_args()

    import torch
    from xpng_amd import api, tensors
    from xpng_amd.synth import synth_raster_torch

    rng = random.Random(a.seed)
    dims = [(rng.randint(352, 1600), rng.randint(200, 1100)) for _ in range(a.batch)]
    ts = [(synth_raster_torch("photo", w, h, False, seed=b + 1).permute(2, 0, 1).to(torch.float32) / 255.0).to(torch.float16).contiguous()
          for b, (w, h) in enumerate(dims)]
    tmp = tempfile.mkdtemp(prefix="store_tensors_timing_")
    pa, pb = ([os.path.join(tmp, f"{leg}{i}.xpng") for i in range(a.batch)] for leg in "ab")

    def leg_a():
        rasters = [(t.to(torch.float32) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy() for t in ts]
        api.store_batch(a.level, rasters, pa)

    def leg_b():
        tensors.store_files(ts, pb, level=a.level)

    legs = {"torch_then_store_batch": leg_a, "store_files": leg_b}
    ms = {k: [] for k in legs}
    try:
        for it in range(a.warmup + a.iters):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            if it == 0:
                for x, y in zip(pa, pb):
                    assert open(x, "rb").read() == open(y, "rb").read(), (x, y)
        file_bytes = sum(os.path.getsize(p) for p in pb)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = {k: {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)} for k, v in ms.items()}
    ra, rb = res["torch_then_store_batch"], res["store_files"]
    spread = max(ra["max_ms"] - ra["min_ms"], rb["max_ms"] - rb["min_ms"])
    print(json.dumps({"tool": "store_tensors_timing", "batch": a.batch, "level": a.level, "dtype": "float16", "layout": "chw", "seed": a.seed, "iters": a.iters,
                      "megapixels": round(sum(w * h for w, h in dims) / 1e6, 2), "file_MB": round(file_bytes / 2**20, 1), **res,
                      "a_over_b": round(ra["median_ms"] / rb["median_ms"], 2), "larger_spread_ms": round(spread, 2),
                      "b_no_slower_than_a_by_more_than_the_spread": rb["median_ms"] <= ra["median_ms"] + spread}))


if __name__ == "__main__":
    main()
