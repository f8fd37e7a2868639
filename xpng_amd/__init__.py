"""xpng_amd -- MI355X-native xPNG tile codec (host-side Python mirror of the C API).

The product is native: `xpng_amd/lib/libxpng_hip.so` (hand-written HIP kernels for gfx950 behind the C-ABI
of include/xpng_hip.h) and `libxpng.so` / `bin/xpng` (the host C driver and CLI that mirror the reference's
xpng.h / xpng.c).  This package only binds those libraries with ctypes for tests, bench.py and
torch.distributed sharding.  It never falls back to a CPU codec: if the HIP library is missing or no GPU
is visible, compute calls raise.
"""
from .api import (DTYPE_BF16, DTYPE_F16, DTYPE_F32, FILTER_BILINEAR, FILTER_CUBIC_AA, FILTER_NEAREST, FILTER_TRIANGLE_AA, Context, MixedContext, StagedImages, XpngError, affine_footprint, affine_view_tiles, blur_weights, build_native, decode_mixed, decode_region, decode_tiles, device_count, dtype_bytes,
                  encode_tiles, float_table, hip_lib, host_lib, layout, layout_channels, load, load_batch, load_region, native_paths, normalize_device, quantize_host, region_tiles, resample_affine_host, resample_blur_host, resample_colour_host, resample_cubic_host, resample_host, resize_host, store, store_batch,
                  store_tensors, view_tiles, TONE_AUTOCONTRAST, TONE_EQUALISE, TONE_INVERT, TONE_NONE, TONE_POSTERISE, TONE_SOLARISE, ViewTone, resample_affine_tone_host, resample_tone_host)

__all__ = ["DTYPE_BF16", "DTYPE_F16", "DTYPE_F32", "FILTER_BILINEAR", "FILTER_CUBIC_AA", "FILTER_NEAREST", "FILTER_TRIANGLE_AA", "Context", "MixedContext", "StagedImages", "XpngError", "affine_footprint", "affine_view_tiles", "blur_weights", "build_native", "decode_mixed", "decode_region", "decode_tiles", "device_count", "dtype_bytes",
           "encode_tiles", "float_table", "hip_lib", "host_lib", "layout", "layout_channels", "load", "load_batch", "load_region", "native_paths", "normalize_device",
           "quantize_host", "region_tiles", "resample_affine_host", "resample_blur_host", "resample_colour_host", "resample_cubic_host", "resample_host", "resize_host", "store", "store_batch", "store_tensors", "view_tiles",
           "TONE_AUTOCONTRAST", "TONE_EQUALISE", "TONE_INVERT", "TONE_NONE", "TONE_POSTERISE", "TONE_SOLARISE", "ViewTone", "resample_affine_tone_host", "resample_tone_host"]
