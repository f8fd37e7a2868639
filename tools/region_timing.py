"""Region decode against full decode, one context, one stream (GPU).

64 synthetic 4096^2 'photo' RGBA rasters are encoded at level 1 into HBM; then, timed with HIP events on one stream:
  region : one xpnghip_decode_region_device_batch launch, a random 224 x 224 crop per image (tight output)
  full   : one xpnghip_decode_device_batch launch over every tile of the same blobs (full-size output)
Both use the device-side size walk.  Prints one JSON line (median GPU milliseconds per launch).

    python tools/region_timing.py [--batch 64] [--crop 224] [--iters 7] [--warmup 2] [--seed 1]
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
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch
    import xpng_amd
    from xpng_amd.synth import synth_raster_torch

    W = H = a.size
    B, ch = a.batch, 4
    ctx = xpng_amd.Context(W, H, ch, batch=B)
    d_r = [synth_raster_torch("photo", W, H, True, seed=b + 1) for b in range(B)]
    d_b = [torch.empty(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
    lens = ctx.encode_device_batch(1, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
    del d_r
    rng = random.Random(a.seed)
    rects = [(rng.randint(0, W - a.crop), rng.randint(0, H - a.crop), a.crop, a.crop) for _ in range(B)]
    tiles_per_crop = [len(xpng_amd.region_tiles(W, H, r)) for r in rects]
    d_crop = [torch.empty(a.crop * a.crop * ch, dtype=torch.uint8, device="cuda") for _ in range(B)]
    d_full = [torch.empty(W * H * ch, dtype=torch.uint8, device="cuda") for _ in range(B)]
    blobs, outs_c, outs_f = [t.data_ptr() for t in d_b], [t.data_ptr() for t in d_crop], [t.data_ptr() for t in d_full]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream

    def region():
        ctx.decode_region_batch(1, blobs, lens, rects, outs_c, a.crop * ch, stream=sh)

    def full():
        ctx.decode_device_batch(1, blobs, lens, None, outs_f, stream=sh)

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn()
                e1.record(stream)
            e1.synchronize()
            if ctx.decode_status(sh) != 0:
                raise SystemExit("a tile was rejected")
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    r_ms, f_ms = timed(region), timed(full)
    rm, fm = statistics.median(r_ms), statistics.median(f_ms)
    print(json.dumps({"tool": "region_timing", "images": B, "size": f"{W}x{H}", "format": "RGBA8 level 1", "crop": a.crop,
                      "tiles_per_crop_mean": round(sum(tiles_per_crop) / B, 2), "region_ms": round(rm, 3), "full_ms": round(fm, 3),
                      "full_over_region": round(fm / rm, 2), "region_ms_all": [round(v, 3) for v in r_ms],
                      "full_ms_all": [round(v, 3) for v in f_ms]}))
    ctx.close()


if __name__ == "__main__":
    main()
