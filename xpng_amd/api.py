"""ctypes binding of libxpng_hip.so (include/xpng_hip.h) and libxpng.so (include/xpng.h)."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xpng_amd", "lib")
HIP_SO = os.path.join(LIBDIR, "libxpng_hip.so")
PROBES_SO = os.path.join(LIBDIR, "libxpng_hip_probes.so")  # -DXPNG_PROBES build: timing-study switches, wave probe, fake devices
HOST_SO = os.path.join(LIBDIR, "libxpng.so")
CLI = os.path.join(ROOT, "xpng_amd", "bin", "xpng")

# every symbol include/xpng_hip.h declares (tests/test_abi.py checks the .so exports all of them)
HIP_SYMBOLS = [
    "xpnghip_abi_version", "xpnghip_device_count", "xpnghip_last_error", "xpnghip_encode_tiles",
    "xpnghip_decode_tiles", "xpnghip_ctx_create", "xpnghip_ctx_destroy", "xpnghip_ctx_tile_count",
    "xpnghip_ctx_tile", "xpnghip_ctx_blob_bound", "xpnghip_ctx_workspace_bytes", "xpnghip_encode_device",
    "xpnghip_ctx_last_blobs_len", "xpnghip_decode_device", "xpnghip_m1_transform_device", "xpnghip_debug_fetch",
    "xpnghip_debug_probe", "xpnghip_debug_probe_count",
    "xpnghip_ctx_create_batch", "xpnghip_ctx_batch", "xpnghip_encode_device_batch", "xpnghip_ctx_last_blobs_len_at",
    "xpnghip_decode_device_batch", "xpnghip_m1_transform_device_batch", "xpnghip_ctx_create_range", "xpnghip_ctx_decode_status",
    "xpnghip_image_begin", "xpnghip_image_single_colour", "xpnghip_image_encode", "xpnghip_image_fetch", "xpnghip_image_end",
    "xpnghip_normalize_device", "xpnghip_encode_tiles_T", "xpnghip_decode_tiles_T", "xpnghip_image_encode_T", "xpnghip_devices_for",
    "xpnghip_shard_ranges", "xpnghip_shutdown", "xpnghip_probes_built",
    "xpnghip_region_tiles", "xpnghip_decode_region", "xpnghip_decode_region_device_batch",
    "xpnghip_ctx_create_mixed", "xpnghip_ctx_mixed_first_tile", "xpnghip_decode_mixed_device_batch", "xpnghip_decode_mixed",
    "xpnghip_encode_varsize_device_batch",
    "xpnghip_images_begin", "xpnghip_images_single_colour", "xpnghip_images_encode", "xpnghip_images_fetch", "xpnghip_images_end",
    "xpnghip_images_first_pixel", "xpnghip_batch_cuts",
    "xpnghip_layout_channels", "xpnghip_decode_varsize_device_batch_as", "xpnghip_encode_varsize_device_batch_from",
    "xpnghip_dtype_bytes", "xpnghip_float_table", "xpnghip_decode_varsize_device_batch_as_float",
    "xpnghip_decode_varsize_device_batch_resized", "xpnghip_resize_host",
    "xpnghip_decode_varsize_device_batch_resampled", "xpnghip_resample_host",
    "xpnghip_images_begin_device", "xpnghip_quantize_host",
    "xpnghip_decode_varsize_device_batch_views", "xpnghip_view_tiles", "xpnghip_ctx_last_decode_tiles",
    "xpnghip_resample_colour_host", "xpnghip_decode_varsize_device_batch_views_colour",
    "xpnghip_resample_cubic_host", "xpnghip_decode_varsize_device_batch_views_cubic",
    "xpnghip_blur_weights", "xpnghip_resample_blur_host", "xpnghip_decode_varsize_device_batch_views_blur",
    "xpnghip_affine_footprint", "xpnghip_resample_affine_host", "xpnghip_affine_view_tiles",
    "xpnghip_decode_varsize_device_batch_views_affine",
    "xpnghip_resample_tone_host", "xpnghip_resample_affine_tone_host",
    "xpnghip_decode_varsize_device_batch_views_tone", "xpnghip_decode_varsize_device_batch_views_affine_tone",
]
HOST_SYMBOLS = ["xpng_store", "xpng_load", "xpng_from_jpg", "xpng_store_T", "xpng_load_T", "xpng_from_jpg_T",
                "store_7", "load_7"]
# libxpng.so's own additions beyond the reference's surface (include/xpng_region.h)
HOST_EXT_SYMBOLS = ["xpng_load_region"]
# ... and include/xpng_batch.h
HOST_BATCH_SYMBOLS = ["xpng_load_batch"]
# ... and include/xpng_store_batch.h
HOST_STORE_BATCH_SYMBOLS = ["xpng_store_batch"]
# ... and include/xpng_store_tensors.h
HOST_STORE_TENSORS_SYMBOLS = ["xpng_store_tensors"]


class XpngError(RuntimeError):
    pass


def native_paths():
    return {"hip": HIP_SO, "host": HOST_SO, "cli": CLI}


def build_native(targets=("hip", "host")) -> None:
    """Compile the native libraries in-tree (hipcc --offload-arch=gfx950; works without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", ROOT, *targets])


class XpngT(C.Structure):  # include/xpng.h xpng_t
    _fields_ = [("p", C.POINTER(C.c_uint8)), ("w", C.c_uint64), ("h", C.c_uint64), ("s", C.c_uint64), ("A", C.c_bool)]


_hip = None
_host = None
_probes = None


class ViewBlur(C.Structure):  # include/xpng_hip.h xpnghip_view_blur
    _fields_ = [("sigma", C.c_float), ("radius", C.c_uint32), ("solarise", C.c_float), ("reserved", C.c_uint32)]


class ViewTone(C.Structure):  # include/xpng_hip.h xpnghip_view_tone
    _fields_ = [("op", C.c_uint8 * 4), ("arg", C.c_float * 4)]


def _bind_hip(path):
    L = C.CDLL(path)
    if True:
        u64, vp = C.c_uint64, C.c_void_p
        L.xpnghip_abi_version.restype = C.c_int
        L.xpnghip_device_count.restype = C.c_int
        L.xpnghip_last_error.restype = C.c_char_p
        L.xpnghip_encode_tiles.restype = C.c_int
        L.xpnghip_encode_tiles.argtypes = [C.c_int, vp, u64, u64, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(u64)]
        L.xpnghip_decode_tiles.restype = C.c_int
        L.xpnghip_decode_tiles.argtypes = [C.c_int, vp, u64, u64, u64, C.c_int, vp]
        L.xpnghip_encode_tiles_T.restype = C.c_int
        L.xpnghip_encode_tiles_T.argtypes = [u64, C.c_int, vp, u64, u64, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(u64)]
        L.xpnghip_decode_tiles_T.restype = C.c_int
        L.xpnghip_decode_tiles_T.argtypes = [u64, C.c_int, vp, u64, u64, u64, C.c_int, vp]
        L.xpnghip_devices_for.restype = C.c_int
        L.xpnghip_devices_for.argtypes = [u64, u64, u64]
        L.xpnghip_ctx_create.restype = C.c_int
        L.xpnghip_ctx_create.argtypes = [C.POINTER(vp), C.c_int, u64, u64, C.c_int]
        L.xpnghip_ctx_create_batch.restype = C.c_int
        L.xpnghip_ctx_create_batch.argtypes = [C.POINTER(vp), C.c_int, u64, u64, C.c_int, C.c_uint32]
        L.xpnghip_ctx_create_range.restype = C.c_int
        L.xpnghip_ctx_create_range.argtypes = [C.POINTER(vp), C.c_int, u64, u64, C.c_int, C.c_uint32, u64, u64]
        L.xpnghip_ctx_batch.restype = C.c_uint32
        L.xpnghip_ctx_batch.argtypes = [vp]
        L.xpnghip_encode_device_batch.restype = C.c_int
        L.xpnghip_encode_device_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_uint32, u64, u64, C.POINTER(vp), C.POINTER(u64), vp]
        L.xpnghip_ctx_last_blobs_len_at.restype = u64
        L.xpnghip_ctx_last_blobs_len_at.argtypes = [vp, C.c_uint32]
        L.xpnghip_decode_device_batch.restype = C.c_int
        L.xpnghip_decode_device_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), u64, u64, C.POINTER(vp), vp]
        L.xpnghip_ctx_decode_status.restype = C.c_int
        L.xpnghip_ctx_decode_status.argtypes = [vp, vp]
        L.xpnghip_ctx_destroy.restype = None
        L.xpnghip_ctx_destroy.argtypes = [vp]
        L.xpnghip_ctx_tile_count.restype = u64
        L.xpnghip_ctx_tile_count.argtypes = [vp]
        L.xpnghip_ctx_tile.restype = C.c_int
        L.xpnghip_ctx_tile.argtypes = [vp, u64, C.POINTER(u64)]
        L.xpnghip_ctx_blob_bound.restype = u64
        L.xpnghip_ctx_blob_bound.argtypes = [vp, u64, u64]
        L.xpnghip_ctx_workspace_bytes.restype = u64
        L.xpnghip_ctx_workspace_bytes.argtypes = [vp]
        L.xpnghip_encode_device.restype = C.c_int
        L.xpnghip_encode_device.argtypes = [vp, C.c_int, vp, u64, u64, vp, C.POINTER(u64), vp]
        L.xpnghip_ctx_last_blobs_len.restype = u64
        L.xpnghip_ctx_last_blobs_len.argtypes = [vp]
        L.xpnghip_decode_device.restype = C.c_int
        L.xpnghip_decode_device.argtypes = [vp, C.c_int, vp, u64, C.POINTER(u64), u64, u64, vp, vp]
        L.xpnghip_m1_transform_device.restype = C.c_int
        L.xpnghip_m1_transform_device.argtypes = [vp, vp, u64, u64, vp]
        L.xpnghip_m1_transform_device_batch.restype = C.c_int
        L.xpnghip_m1_transform_device_batch.argtypes = [vp, C.POINTER(vp), C.c_uint32, u64, u64, vp]
        L.xpnghip_debug_fetch.restype = C.c_int64
        L.xpnghip_debug_probe.argtypes = [vp, C.c_uint32]
        L.xpnghip_debug_probe_count.restype = C.c_int64
        L.xpnghip_debug_fetch.argtypes = [vp, C.c_int, u64, vp, u64]
        L.xpnghip_normalize_device.restype = C.c_int
        L.xpnghip_normalize_device.argtypes = [vp, u64, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
        L.xpnghip_shard_ranges.restype = C.c_int
        L.xpnghip_shard_ranges.argtypes = [u64, u64, C.c_int, C.POINTER(u64), C.c_int]
        L.xpnghip_shutdown.restype = None
        L.xpnghip_probes_built.restype = C.c_int
        L.xpnghip_image_begin.restype = C.c_int
        L.xpnghip_image_begin.argtypes = [C.POINTER(vp), vp, u64, u64, C.c_int, C.POINTER(C.c_int)]
        L.xpnghip_image_single_colour.restype = C.c_int
        L.xpnghip_image_single_colour.argtypes = [vp, C.POINTER(C.c_int)]
        L.xpnghip_image_encode_T.restype = C.c_int
        L.xpnghip_image_encode_T.argtypes = [vp, u64, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(u64)]
        L.xpnghip_image_fetch.restype = C.c_int
        L.xpnghip_image_fetch.argtypes = [vp, vp]
        L.xpnghip_image_end.restype = None
        L.xpnghip_image_end.argtypes = [vp]
        L.xpnghip_region_tiles.restype = C.c_int
        L.xpnghip_region_tiles.argtypes = [u64, u64, C.POINTER(u64), C.POINTER(C.c_uint32), C.c_int]
        L.xpnghip_decode_region.restype = C.c_int
        L.xpnghip_decode_region.argtypes = [C.c_int, vp, u64, u64, u64, C.c_int, C.POINTER(u64), vp]
        L.xpnghip_decode_region_device_batch.restype = C.c_int
        L.xpnghip_decode_region_device_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                         C.POINTER(u64), C.POINTER(vp), u64, vp]
        L.xpnghip_ctx_create_mixed.restype = C.c_int
        L.xpnghip_ctx_create_mixed.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(u64), C.c_uint32, C.c_int]
        L.xpnghip_ctx_mixed_first_tile.restype = u64
        L.xpnghip_ctx_mixed_first_tile.argtypes = [vp, C.c_uint32]
        L.xpnghip_decode_mixed_device_batch.restype = C.c_int
        L.xpnghip_decode_mixed_device_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                        C.POINTER(vp), u64, vp]
        L.xpnghip_encode_varsize_device_batch.restype = C.c_int
        L.xpnghip_encode_varsize_device_batch.argtypes = [vp, C.c_int, C.POINTER(vp), u64, C.c_uint32, C.POINTER(vp), C.POINTER(u64), vp]
        L.xpnghip_layout_channels.restype = C.c_int
        L.xpnghip_layout_channels.argtypes = [C.c_uint32, C.c_int]
        L.xpnghip_decode_varsize_device_batch_as.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_as.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                             C.POINTER(vp), C.c_uint32, vp]
        L.xpnghip_encode_varsize_device_batch_from.restype = C.c_int
        L.xpnghip_encode_varsize_device_batch_from.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(u64), vp]
        f32p = C.POINTER(C.c_float)
        L.xpnghip_dtype_bytes.restype = C.c_int
        L.xpnghip_dtype_bytes.argtypes = [C.c_uint32]
        L.xpnghip_float_table.restype = C.c_int
        L.xpnghip_float_table.argtypes = [C.c_uint32, C.c_int, f32p, f32p, vp]
        L.xpnghip_decode_varsize_device_batch_as_float.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_as_float.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                                   C.POINTER(vp), C.c_uint32, C.c_uint32, f32p, f32p, vp]
        u8p = C.POINTER(C.c_uint8)
        L.xpnghip_decode_varsize_device_batch_resized.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_resized.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                                  C.POINTER(vp), C.c_uint32, C.c_uint32, f32p, f32p, C.POINTER(u64), u8p,
                                                                  C.c_uint32, C.c_uint32, vp]
        L.xpnghip_resize_host.restype = C.c_int
        L.xpnghip_resize_host.argtypes = [C.c_int, vp, u64, u64, C.POINTER(u64), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          f32p, f32p, vp]
        L.xpnghip_decode_varsize_device_batch_resampled.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_resampled.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                                    C.POINTER(vp), C.c_uint32, C.c_uint32, f32p, f32p, C.POINTER(u64), u8p,
                                                                    C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.xpnghip_resample_host.restype = C.c_int
        L.xpnghip_resample_host.argtypes = [C.c_int, vp, u64, u64, C.POINTER(u64), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            f32p, f32p, C.c_uint32, vp]
        u32p = C.POINTER(C.c_uint32)
        L.xpnghip_decode_varsize_device_batch_views.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), C.c_uint32, u32p,
                                                                C.POINTER(vp), u32p, C.POINTER(u64), u8p, C.c_uint32, C.c_uint32, f32p, f32p,
                                                                C.c_uint32, vp]
        L.xpnghip_resample_colour_host.restype = C.c_int
        L.xpnghip_resample_colour_host.argtypes = [C.c_int, vp, u64, u64, C.POINTER(u64), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                   f32p, f32p, C.c_uint32, f32p, vp]
        L.xpnghip_decode_varsize_device_batch_views_colour.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views_colour.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), C.c_uint32,
                                                                       u32p, C.POINTER(vp), u32p, C.POINTER(u64), u8p, C.c_uint32, C.c_uint32, f32p,
                                                                       f32p, C.c_uint32, f32p, vp]
        L.xpnghip_resample_cubic_host.restype = C.c_int
        L.xpnghip_resample_cubic_host.argtypes = [C.c_int, vp, u64, u64, C.POINTER(u64), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  f32p, f32p, f32p, vp]
        L.xpnghip_decode_varsize_device_batch_views_cubic.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views_cubic.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), C.c_uint32,
                                                                      u32p, C.POINTER(vp), u32p, C.POINTER(u64), u8p, C.c_uint32, C.c_uint32, f32p,
                                                                      f32p, f32p, vp]
        L.xpnghip_blur_weights.restype = C.c_int
        L.xpnghip_blur_weights.argtypes = [C.c_float, C.c_uint32, f32p]
        L.xpnghip_resample_blur_host.restype = C.c_int
        L.xpnghip_resample_blur_host.argtypes = [C.c_int, vp, u64, u64, C.POINTER(u64), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 f32p, f32p, C.c_uint32, f32p, C.POINTER(ViewBlur), vp]
        L.xpnghip_decode_varsize_device_batch_views_blur.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views_blur.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), C.c_uint32,
                                                                     u32p, C.POINTER(vp), u32p, C.POINTER(u64), u8p, C.c_uint32, C.c_uint32, f32p,
                                                                     f32p, C.c_uint32, f32p, C.POINTER(ViewBlur), vp]
        L.xpnghip_affine_footprint.restype = C.c_int
        L.xpnghip_affine_footprint.argtypes = [u64, u64, f32p, C.c_uint32, C.c_uint32, C.POINTER(u64)]
        L.xpnghip_resample_affine_host.restype = C.c_int
        L.xpnghip_resample_affine_host.argtypes = [C.c_int, vp, u64, u64, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, f32p, C.c_uint32,
                                                   f32p, f32p, vp]
        L.xpnghip_affine_view_tiles.restype = C.c_int64
        L.xpnghip_affine_view_tiles.argtypes = [C.POINTER(u64), C.c_uint32, C.c_uint32, u32p, f32p, u32p, u32p, u64]
        L.xpnghip_decode_varsize_device_batch_views_affine.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views_affine.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), C.c_uint32,
                                                                       u32p, C.POINTER(vp), u32p, f32p, f32p, C.c_uint32, C.c_uint32, f32p, f32p,
                                                                       C.c_uint32, f32p, vp]
        L.xpnghip_resample_tone_host.restype = C.c_int
        L.xpnghip_resample_tone_host.argtypes = [C.c_int, vp, u64, u64, C.POINTER(u64), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 f32p, f32p, C.c_uint32, f32p, C.POINTER(ViewBlur), C.POINTER(ViewTone), vp]
        L.xpnghip_resample_affine_tone_host.restype = C.c_int
        L.xpnghip_resample_affine_tone_host.argtypes = [C.c_int, vp, u64, u64, f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p, f32p,
                                                        C.c_uint32, f32p, f32p, C.POINTER(ViewTone), vp]
        L.xpnghip_decode_varsize_device_batch_views_tone.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views_tone.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64), C.c_uint32,
                                                                     u32p, C.POINTER(vp), u32p, C.POINTER(u64), u8p, C.c_uint32, C.c_uint32, f32p,
                                                                     f32p, C.c_uint32, f32p, C.POINTER(ViewBlur), C.POINTER(ViewTone), vp]
        L.xpnghip_decode_varsize_device_batch_views_affine_tone.restype = C.c_int
        L.xpnghip_decode_varsize_device_batch_views_affine_tone.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64),
                                                                            C.c_uint32, u32p, C.POINTER(vp), u32p, f32p, f32p, C.c_uint32, C.c_uint32,
                                                                            f32p, f32p, C.c_uint32, f32p, C.POINTER(ViewTone), vp]
        L.xpnghip_view_tiles.restype = C.c_int64
        L.xpnghip_view_tiles.argtypes = [C.POINTER(u64), C.c_uint32, C.c_uint32, u32p, C.POINTER(u64), u32p, u64]
        L.xpnghip_ctx_last_decode_tiles.restype = u64
        L.xpnghip_ctx_last_decode_tiles.argtypes = [vp]
        L.xpnghip_images_begin.restype = C.c_int
        L.xpnghip_images_begin.argtypes = [C.POINTER(vp), C.c_uint32, C.POINTER(vp), C.POINTER(u64), u8p, u8p]
        L.xpnghip_images_begin_device.restype = C.c_int
        L.xpnghip_images_begin_device.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.POINTER(vp), C.POINTER(u64), u8p, C.c_uint32, C.c_uint32,
                                                  f32p, f32p, vp, u8p]
        L.xpnghip_quantize_host.restype = C.c_int
        L.xpnghip_quantize_host.argtypes = [C.c_uint32, C.c_uint32, C.c_int, vp, u64, f32p, f32p, vp]
        L.xpnghip_images_single_colour.restype = C.c_int
        L.xpnghip_images_single_colour.argtypes = [vp, u8p]
        L.xpnghip_images_encode.restype = C.c_int
        L.xpnghip_images_encode.argtypes = [vp, u8p, C.POINTER(u8p), C.POINTER(u64)]
        L.xpnghip_images_fetch.restype = C.c_int
        L.xpnghip_images_fetch.argtypes = [vp, C.c_uint32, vp]
        L.xpnghip_images_first_pixel.restype = C.c_int
        L.xpnghip_images_first_pixel.argtypes = [vp, C.c_uint32, vp]
        L.xpnghip_batch_cuts.restype = C.c_int
        L.xpnghip_batch_cuts.argtypes = [C.c_uint32, C.POINTER(u64), u8p, C.c_uint32, u64, C.POINTER(C.c_uint32), C.c_int]
        L.xpnghip_images_end.restype = None
        L.xpnghip_images_end.argtypes = [vp]
        L.xpnghip_decode_mixed.restype = C.c_int
        L.xpnghip_decode_mixed.argtypes = [C.c_int, C.c_int, C.c_uint32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(vp)]
    return L


def hip_lib():
    """The release library.  XPNG_USE_PROBES_LIB=1 (tools/ only) makes every binding in this module use the probe build."""
    global _hip
    if _hip is None:
        path = PROBES_SO if os.environ.get("XPNG_USE_PROBES_LIB") else HIP_SO
        if not os.path.exists(path):
            raise XpngError(f"{path} is missing: run `make hip` (there is no CPU fallback)")
        _hip = _bind_hip(path)
    return _hip


def probes_lib():
    """libxpng_hip_probes.so (-DXPNG_PROBES) as a second, independent handle: for the tests / tools that need a switch the
    release library does not have (XPNG_FAKE_DEVICES, XPNG_SKIP, pads, the wave probe)."""
    global _probes
    if _probes is None:
        if not os.path.exists(PROBES_SO):
            raise XpngError(f"{PROBES_SO} is missing: run `make probes`")
        _probes = _bind_hip(PROBES_SO)
    return _probes


def shard_ranges(w: int, h: int, D: int):
    """Tile ranges a host-buffer call on D devices uses (xpnghip_shard_ranges; host-only, needs no GPU)."""
    arr = (C.c_uint64 * (2 * max(D, 1)))()
    n = hip_lib().xpnghip_shard_ranges(w, h, D, arr, max(D, 1))
    if n < 0:
        raise XpngError("xpnghip_shard_ranges failed")
    return [(int(arr[2 * k]), int(arr[2 * k + 1])) for k in range(n)]


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_SO):
            raise XpngError(f"{HOST_SO} is missing: run `make host`")
        hip_lib()
        L = C.CDLL(HOST_SO)
        for name in ("xpng_store", "xpng_load", "store_7", "load_7", "xpng_store_T", "xpng_load_T"):
            getattr(L, name).restype = C.c_bool
        L.xpng_store.argtypes = [C.c_uint64, C.POINTER(XpngT), C.c_char_p]
        L.xpng_load.argtypes = [C.c_char_p, C.POINTER(XpngT)]
        L.xpng_store_T.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(XpngT), C.c_char_p]
        L.xpng_load_T.argtypes = [C.c_uint64, C.c_char_p, C.POINTER(XpngT)]
        L.store_7.argtypes = [C.POINTER(XpngT), C.c_char_p]
        L.xpng_load_region.restype = C.c_bool
        L.xpng_load_region.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(XpngT)]
        L.load_7.argtypes = [C.c_char_p, C.POINTER(XpngT)]
        L.xpng_load_batch.restype = C.c_bool
        L.xpng_load_batch.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(XpngT)]
        L.xpng_store_batch.restype = C.c_bool
        L.xpng_store_batch.argtypes = [C.c_uint64, C.POINTER(XpngT), C.POINTER(C.c_char_p), C.c_uint64]
        L.xpng_store_tensors.restype = C.c_bool
        L.xpng_store_tensors.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_uint32,
                                         C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_void_p, C.POINTER(C.c_char_p)]
        _host = L
    return _host


def _err():
    return hip_lib().xpnghip_last_error().decode(errors="replace")


def device_count() -> int:
    return hip_lib().xpnghip_device_count()


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


class MallocedBlobs:
    """The malloc()ed buffer xpnghip_encode_tiles hands back, not yet copied into a Python object (bench.py times the C call
    alone: the copy into `bytes` and the free() are this binding's, not the library's)."""
    def __init__(self, p, n):
        self.p, self.n = p, n

    def bytes(self) -> bytes:
        return C.string_at(self.p, self.n)

    def free(self):
        if self.p:
            _libc.free(self.p)
            self.p = None


def encode_tiles(mode: int, raster: np.ndarray, T: int = 1, lib=None, copy: bool = True):
    """Host raster (h, w, 3|4) uint8 -> concatenated tile blobs (xpnghip_encode_tiles_T; H2D + kernels + D2H) on T devices.
    copy=False returns the library's malloc()ed buffer as a MallocedBlobs (caller frees)."""
    raster = np.ascontiguousarray(raster, dtype=np.uint8)
    h, w, ch = raster.shape
    p, n = C.POINTER(C.c_uint8)(), C.c_uint64()
    lib = lib or hip_lib()
    if lib.xpnghip_encode_tiles_T(T, mode, raster.ctypes.data_as(C.c_void_p), w, h, ch, C.byref(p), C.byref(n)):
        raise XpngError("xpnghip_encode_tiles: " + lib.xpnghip_last_error().decode(errors="replace"))
    if not copy:
        return MallocedBlobs(p, n.value)
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out


def decode_tiles(mode: int, blobs: bytes, w: int, h: int, pxsz: int, T: int = 1, lib=None, out: np.ndarray = None) -> np.ndarray:
    """Tile blobs -> raster (xpnghip_decode_tiles_T).  out: a caller-allocated (h, w, pxsz) uint8 array to fill (what xpng_load's
    malloc is to the C call, libxpng.c:974); default: a fresh zero-filled one."""
    raster = np.zeros((h, w, pxsz), dtype=np.uint8) if out is None else out
    assert raster.shape == (h, w, pxsz) and raster.dtype == np.uint8 and raster.flags["C_CONTIGUOUS"]
    buf = np.frombuffer(blobs, dtype=np.uint8)
    lib = lib or hip_lib()
    if lib.xpnghip_decode_tiles_T(T, mode, buf.ctypes.data_as(C.c_void_p), len(blobs), w, h, pxsz,
                                  raster.ctypes.data_as(C.c_void_p)):
        raise XpngError("xpnghip_decode_tiles: " + lib.xpnghip_last_error().decode(errors="replace"))
    return raster


def staged_encode(mode: int, raster: np.ndarray, T: int = 1, lib=None):
    """The staged-image sequence xpng_store runs (xpnghip_image_begin .. _end): returns (bytes per pixel after
    normalize_RGBA, single-colour?, tile blobs, normalised raster bytes)."""
    raster = np.ascontiguousarray(raster, dtype=np.uint8)
    h, w, ch = raster.shape
    lib = lib or hip_lib()
    img, pxsz = C.c_void_p(), C.c_int(0)
    if lib.xpnghip_image_begin(C.byref(img), raster.ctypes.data_as(C.c_void_p), w, h, ch, C.byref(pxsz)):
        raise XpngError("xpnghip_image_begin: " + lib.xpnghip_last_error().decode(errors="replace"))
    try:
        single = C.c_int(0)
        if lib.xpnghip_image_single_colour(img, C.byref(single)):
            raise XpngError("xpnghip_image_single_colour: " + lib.xpnghip_last_error().decode(errors="replace"))
        norm = np.zeros(h * w * pxsz.value, dtype=np.uint8)
        if lib.xpnghip_image_fetch(img, norm.ctypes.data_as(C.c_void_p)):
            raise XpngError("xpnghip_image_fetch: " + lib.xpnghip_last_error().decode(errors="replace"))
        p, n = C.POINTER(C.c_uint8)(), C.c_uint64()
        if lib.xpnghip_image_encode_T(img, T, mode, C.byref(p), C.byref(n)):
            raise XpngError("xpnghip_image_encode_T: " + lib.xpnghip_last_error().decode(errors="replace"))
        blobs = C.string_at(p, n.value)
        _libc.free(p)
        return pxsz.value, bool(single.value), blobs, norm.tobytes()
    finally:
        lib.xpnghip_image_end(img)


def image_store(mode: int, raster: np.ndarray, T: int = 0, lib=None) -> MallocedBlobs:
    """Exactly the device-side sequence of xpng_store for a raster that reaches the tile codec (host/xpng_api.c store_on_device):
    xpnghip_image_begin -> xpnghip_image_encode_T -> xpnghip_image_end.  Returns the library's malloc()ed blob buffer."""
    raster = np.ascontiguousarray(raster, dtype=np.uint8)
    h, w, ch = raster.shape
    lib = lib or hip_lib()
    img, pxsz = C.c_void_p(), C.c_int(0)
    if lib.xpnghip_image_begin(C.byref(img), raster.ctypes.data_as(C.c_void_p), w, h, ch, C.byref(pxsz)):
        raise XpngError("xpnghip_image_begin: " + lib.xpnghip_last_error().decode(errors="replace"))
    try:
        p, n = C.POINTER(C.c_uint8)(), C.c_uint64()
        if lib.xpnghip_image_encode_T(img, T, mode, C.byref(p), C.byref(n)):
            raise XpngError("xpnghip_image_encode_T: " + lib.xpnghip_last_error().decode(errors="replace"))
        return MallocedBlobs(p, n.value)
    finally:
        lib.xpnghip_image_end(img)


def store(mode: int, raster: np.ndarray, path: str, T: int = None) -> None:
    """xpng_store[_T] (include/xpng.h): full host driver incl. normalisation, fallbacks and file output."""
    raster = np.ascontiguousarray(raster, dtype=np.uint8)
    h, w, ch = raster.shape
    pm = XpngT(raster.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, raster.size, ch == 4)
    rc = host_lib().xpng_store(mode, C.byref(pm), path.encode()) if T is None else host_lib().xpng_store_T(T, mode, C.byref(pm), path.encode())
    if rc:
        raise XpngError("xpng_store failed")


def load(path: str, T: int = None) -> np.ndarray:
    pm = XpngT()
    rc = host_lib().xpng_load(path.encode(), C.byref(pm)) if T is None else host_lib().xpng_load_T(T, path.encode(), C.byref(pm))
    if rc:
        raise XpngError("xpng_load failed")
    out = np.ctypeslib.as_array(pm.p, shape=(pm.h, pm.w, 3 + int(pm.A))).copy()
    _libc.free(pm.p)
    return out


@functools.lru_cache(maxsize=64)
def _tile_count(w: int, h: int) -> int:
    from .shard import tile_table
    return len(tile_table(w, h))


def region_tiles(w: int, h: int, rect) -> list:
    """Tiles of a w x h image that rect = (x, y, w, h) intersects, ascending (xpnghip_region_tiles; host-only, needs no GPU).
    Raises XpngError on an empty or out-of-image rect."""
    cap = _tile_count(w, h) if 0 < w <= 1 << 24 and 0 < h <= 1 << 24 else 1
    arr, r = (C.c_uint32 * cap)(), (C.c_uint64 * 4)(*rect)
    n = hip_lib().xpnghip_region_tiles(w, h, r, arr, cap)
    if n < 0:
        raise XpngError(f"region_tiles: bad rect {tuple(rect)} for a {w} x {h} image")
    return list(arr[:n])


def decode_region(mode: int, blobs: bytes, w: int, h: int, pxsz: int, rect, lib=None) -> np.ndarray:
    """The rect = (x, y, w, h) crop of a tile body (the file after its 8-byte header) -> (rect h, rect w, pxsz) uint8
    (xpnghip_decode_region: only the tiles the rect touches are uploaded and decoded)."""
    out = np.zeros((max(int(rect[3]), 0), max(int(rect[2]), 0), pxsz), dtype=np.uint8)
    buf = np.frombuffer(blobs, dtype=np.uint8)
    lib = lib or hip_lib()
    if lib.xpnghip_decode_region(mode, buf.ctypes.data_as(C.c_void_p), len(blobs), w, h, pxsz, (C.c_uint64 * 4)(*rect),
                                 out.ctypes.data_as(C.c_void_p)):
        raise XpngError("xpnghip_decode_region: " + lib.xpnghip_last_error().decode(errors="replace"))
    return out


def load_region(path: str, x: int, y: int, w: int, h: int) -> np.ndarray:
    """xpng_load_region (include/xpng_region.h): the (h, w, 3|4) crop at (x, y) of an .xpng file."""
    pm = XpngT()
    if host_lib().xpng_load_region(path.encode(), x, y, w, h, C.byref(pm)):
        raise XpngError("xpng_load_region failed")
    out = np.ctypeslib.as_array(pm.p, shape=(pm.h, pm.w, 3 + int(pm.A))).copy()
    _libc.free(pm.p)
    return out


def decode_mixed(mode: int, bodies, dims, pxsz: int, lib=None) -> list:
    """Tile bodies (each file after its 8-byte header) of images of different sizes, dims[i] = (w, h), one tile mode and pixel
    size -> list of (h, w, pxsz) uint8 rasters (xpnghip_decode_mixed: one device call for all of them)."""
    k = len(bodies)
    assert len(dims) == k
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in bodies]
    outs = [np.zeros((max(int(h), 0), max(int(w), 0), pxsz), dtype=np.uint8) for (w, h) in dims]
    ins = (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
    ops = (C.c_void_p * k)(*[o.ctypes.data for o in outs])
    lens = (C.c_uint64 * k)(*[len(b) for b in bodies])
    flat = (C.c_uint64 * (2 * k))(*[int(v) for d in dims for v in d])
    lib = lib or hip_lib()
    if lib.xpnghip_decode_mixed(mode, pxsz, k, ins, lens, flat, ops):
        raise XpngError("xpnghip_decode_mixed: " + lib.xpnghip_last_error().decode(errors="replace"))
    return outs


def load_batch(paths) -> list:
    """xpng_load_batch (include/xpng_batch.h): the (h, w, 3|4) rasters of a list of .xpng files of any sizes; element i equals
    load(paths[i]).  Files of one (level, bytes per pixel) are decoded by one mixed-size device call."""
    k = len(paths)
    arr = (C.c_char_p * k)(*[os.fsencode(p) for p in paths])
    pms = (XpngT * k)()
    if k == 0 or host_lib().xpng_load_batch(arr, k, pms):
        raise XpngError("xpng_load_batch failed")
    out = []
    for pm in pms:
        out.append(np.ctypeslib.as_array(pm.p, shape=(pm.h, pm.w, 3 + int(pm.A))).copy())
        _libc.free(pm.p)
    return out


def batch_cuts(dims, pxsz, max_images: int = 4096, max_bytes: int = 2 << 30) -> list:
    """First image of every staged batch xpng_store_batch makes of a list (xpnghip_batch_cuts; host-only, needs no GPU):
    dims[i] = (w, h), pxsz[i] = bytes per pixel as handed in; the defaults are xpng_store_batch's budgets."""
    k = len(dims)
    flat = (C.c_uint64 * max(2 * k, 1))(*[int(v) for d in dims for v in d])
    px, starts = (C.c_uint8 * max(k, 1))(*pxsz), (C.c_uint32 * max(k, 1))()
    n = hip_lib().xpnghip_batch_cuts(k, flat, px, max_images, max_bytes, starts, k)
    if n < 0:
        raise XpngError("xpnghip_batch_cuts failed")
    return list(starts[:n])


LAYOUT_PLANAR, LAYOUT_BGR = 0x001, 0x002  # include/xpng_hip.h XPNGHIP_LAYOUT_*; the channels of the caller's buffers sit in bits 8..11


def layout(planar: bool = False, bgr: bool = False, channels: int = 0) -> int:
    """The layout word of a device buffer (include/xpng_hip.h XPNGHIP_LAYOUT_*): planar (C, H, W) or interleaved (H, W, C),
    B,G,R or R,G,B colour order, channels 3, 4 or 0 = what the context has."""
    if channels not in (0, 3, 4):
        raise XpngError(f"layout: channels must be 0 (the context's), 3 or 4, not {channels!r}")
    return (LAYOUT_PLANAR if planar else 0) | (LAYOUT_BGR if bgr else 0) | (channels << 8)


def layout_channels(layout: int, pxsz: int) -> int:
    """Channels of a buffer of this layout on a context of pxsz bytes per pixel (xpnghip_layout_channels; host-only)."""
    n = hip_lib().xpnghip_layout_channels(layout, pxsz)
    if n < 0:
        raise XpngError(f"bad layout word {layout:#x} or pxsz {pxsz}")
    return n


DTYPE_F16, DTYPE_BF16, DTYPE_F32 = 1, 2, 3  # include/xpng_hip.h XPNGHIP_DTYPE_*: the element of a float buffer


def dtype_bytes(dtype: int) -> int:
    """Bytes of one element of a float buffer (xpnghip_dtype_bytes; host-only)."""
    n = hip_lib().xpnghip_dtype_bytes(dtype)
    if n < 0:
        raise XpngError(f"bad dtype {dtype!r} (DTYPE_F16 = 1, DTYPE_BF16 = 2, DTYPE_F32 = 3)")
    return n


def _floats(name, values, n=None):
    """a scalar or a sequence of numbers as a C array of floats (None stays None: the call's default)"""
    if values is None:
        return None
    try:
        vals = [float(v) for v in values] if hasattr(values, "__len__") or hasattr(values, "__iter__") else [float(values)] * (n or 1)
    except (TypeError, ValueError):
        raise XpngError(f"{name} must be a number or a sequence of numbers, not {values!r}") from None
    if n is not None and len(vals) != n:
        raise XpngError(f"{name} has {len(vals)} values, the buffers have {n} channels")
    return (C.c_float * len(vals))(*vals)


def _scale_bias(layout, pxsz, scale, bias):
    """scale and bias of a float call, one value per channel of a buffer of this layout (a bad layout is the library's to refuse)"""
    ch = hip_lib().xpnghip_layout_channels(layout, pxsz)
    return _floats("scale", scale, ch if ch > 0 else None), _floats("bias", bias, ch if ch > 0 else None), ch


def float_table(dtype: int, scale, bias) -> bytes:
    """The outputs of the float decode for every byte value: len(scale) * 256 elements of `dtype` as raw bytes, element
    c * 256 + v being the conversion of fmaf(v, scale[c], bias[c]) (xpnghip_float_table; host-only, needs no device).  Bit for
    bit what MixedContext.decode_batch_as_float writes."""
    sc, bi = _floats("scale", scale), _floats("bias", bias)
    if sc is None or bi is None or len(sc) != len(bi):
        raise XpngError("float_table: scale and bias must be sequences of the same length")
    buf = C.create_string_buffer(max(len(sc), 1) * 256 * dtype_bytes(dtype))
    if hip_lib().xpnghip_float_table(dtype, len(sc), sc, bi, buf):
        raise XpngError("xpnghip_float_table: " + _err())
    return buf.raw[:len(sc) * 256 * dtype_bytes(dtype)]


def _rect_array(name, rects, n):
    """n rectangles (x, y, w, h) as a flat C array of uint64 (None stays None: every whole image)"""
    if rects is None:
        return None
    rects = list(rects)
    if len(rects) != n or any(len(r) != 4 for r in rects):
        raise XpngError(f"{name}: rects must be {n} tuples (x, y, w, h)")
    try:
        return (C.c_uint64 * max(4 * n, 1))(*[int(v) for r in rects for v in r])
    except (TypeError, ValueError):
        raise XpngError(f"{name}: a rectangle is four non-negative integers (x, y, w, h)") from None


def _flip_array(name, flips, n, what="images"):
    """n flips as a C array of bytes (None stays None: no flips)"""
    if flips is None:
        return None
    flips = list(flips)
    if len(flips) != n:
        raise XpngError(f"{name}: flips has {len(flips)} entries for {n} {what}")
    return (C.c_uint8 * max(n, 1))(*[int(f) & 0xFF for f in flips])


def resize_host(raster, size, layout: int, dtype: int, scale=None, bias=None, rect=None, flip=False) -> bytes:
    """The rule of MixedContext.decode_batch_resized on the host (xpnghip_resize_host; needs no device): `raster` is an
    (h, w, 3|4) uint8 array in the file's form, size = (OH, OW), rect = (x, y, w, h) or None for the whole raster.  Returns the
    C * OH * OW elements of `dtype` in `layout` as raw bytes, bit for bit what the device call writes for these pixels."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resize_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resize_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    ra = _rect_array("resize_host", None if rect is None else [rect], 1)
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resize_host(px, r.ctypes.data, r.shape[1], r.shape[0], ra, int(flip), ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype, sc, bi,
                                     buf.ctypes.data):
        raise XpngError("xpnghip_resize_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


FILTER_BILINEAR, FILTER_TRIANGLE_AA = 0, 1  # include/xpng_hip.h XPNGHIP_FILTER_*: the filter word of a resampled call


def resample_host(raster, size, layout: int, dtype: int, scale=None, bias=None, rect=None, flip=False, filter: int = FILTER_TRIANGLE_AA) -> bytes:
    """The rule of MixedContext.decode_batch_resampled on the host (xpnghip_resample_host; needs no device): resize_host's
    arguments and `filter`, FILTER_BILINEAR (resize_host itself) or FILTER_TRIANGLE_AA (a triangle filter wherever an axis
    shrinks: an antialiased downscale).  Returns the C * OH * OW elements of `dtype` in `layout` as raw bytes, bit for bit what
    the device call writes for these pixels."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    ra = _rect_array("resample_host", None if rect is None else [rect], 1)
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_host(px, r.ctypes.data, r.shape[1], r.shape[0], ra, int(flip), ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype, sc, bi,
                                       int(filter) & 0xFFFFFFFF, buf.ctypes.data):
        raise XpngError("xpnghip_resample_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


COLOUR_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)  # the matrix a None entry of a `colours` list stands for


def _colour12(name, m):
    """one colour matrix - 12 numbers or a (3, 4) array, row k the output colour k of R, G, B, columns R, G, B, 1 - as 12 floats"""
    try:
        a = np.asarray(m, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.shape not in ((12,), (3, 4)):
        raise XpngError(f"{name}: a colour matrix is 12 numbers or a (3, 4) array, not {m!r}")
    return [float(v) for v in a.reshape(12)]


def _colour_table(name, colours, n):
    """the `colours` of a views call of n views as its table of 12 * n floats; None where colours is None or every entry is"""
    if colours is None:
        return None
    colours = list(colours)
    if len(colours) != n:
        raise XpngError(f"{name}: colours has {len(colours)} entries for {n} views")
    if all(m is None for m in colours):
        return None
    return (C.c_float * (12 * n))(*[x for v, m in enumerate(colours) for x in (COLOUR_IDENTITY if m is None else _colour12(f"{name}: colours[{v}]", m))])


def resample_colour_host(raster, size, layout: int, dtype: int, scale=None, bias=None, rect=None, flip=False, filter: int = FILTER_TRIANGLE_AA,
                         colour=None) -> bytes:
    """The rule of MixedContext.decode_batch_views with a colour matrix on the host (xpnghip_resample_colour_host; needs no
    device): resample_host's arguments and `colour`, 12 numbers or a (3, 4) array - row k the output colour k in the order R, G, B
    whatever the layout's BGR bit says, columns the inputs R, G, B and a constant, in byte units.  Every output pixel's three
    resampled colours go through the matrix (three nested fp32 fmaf) and a clamp to 0 .. 255 before the constants; alpha does not.
    colour None is resample_host itself.  Returns the C * OH * OW elements of `dtype` in `layout` as raw bytes, bit for bit what
    the device call writes for these pixels."""
    if colour is None:
        return resample_host(raster, size, layout, dtype, scale, bias, rect, flip, filter)
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_colour_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_colour_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    ra = _rect_array("resample_colour_host", None if rect is None else [rect], 1)
    cm = (C.c_float * 12)(*_colour12("resample_colour_host", colour))
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_colour_host(px, r.ctypes.data, r.shape[1], r.shape[0], ra, int(flip), ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype,
                                              sc, bi, int(filter) & 0xFFFFFFFF, cm, buf.ctypes.data):
        raise XpngError("xpnghip_resample_colour_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


def resample_cubic_host(raster, size, layout: int, dtype: int, scale=None, bias=None, rect=None, flip=False, colour=None) -> bytes:
    """The rule of MixedContext.decode_batch_views_cubic on the host (xpnghip_resample_cubic_host; needs no device):
    resample_colour_host's arguments without `filter` - the call is always the antialiased bicubic: Keys' cubic with a = -0.5 on
    both axes, stretched by the ratio where an axis shrinks, clamped to the rectangle and renormalised, every resampled value
    clamped to 0 .. 255, then the colour matrix where one is given (None: none), then the constants.  Returns the C * OH * OW
    elements of `dtype` in `layout` as raw bytes, bit for bit what the device call writes for these pixels."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_cubic_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_cubic_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    ra = _rect_array("resample_cubic_host", None if rect is None else [rect], 1)
    cm = None if colour is None else (C.c_float * 12)(*_colour12("resample_cubic_host", colour))
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_cubic_host(px, r.ctypes.data, r.shape[1], r.shape[0], ra, int(flip), ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype,
                                             sc, bi, cm, buf.ctypes.data):
        raise XpngError("xpnghip_resample_cubic_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


_CUBIC = object()  # in place of a filter word: the views call that has none

FILTER_CUBIC_AA = 2  # XPNGHIP_FILTER_CUBIC_AA: the third filter word, which resample_blur_host and decode_batch_views_blur alone take
SOLARISE_OFF = 256.0  # the threshold of a record that does not solarise


def blur_weights(sigma: float, radius: int) -> np.ndarray:
    """The radius + 1 fp32 weights w[0 .. radius] of a Gaussian blur (xpnghip_blur_weights; needs no device), the one statement the
    device call, the host rule and the tests share: in double g[d] = exp(-d^2 / (2 sigma^2)), S = g[0] + 2 (g[1] + .. + g[R]),
    w[d] = float32(g[d] / S).  radius is 0 .. 31; radius 0 needs sigma 0 and gives [1.0]."""
    try:
        sigma, radius = float(sigma), int(radius)
    except (TypeError, ValueError):
        raise XpngError(f"blur_weights: sigma and radius must be numbers, not {sigma!r}, {radius!r}") from None
    w = np.zeros(max(min(radius, 31), 0) + 1, dtype=np.float32)
    if hip_lib().xpnghip_blur_weights(sigma, radius & 0xFFFFFFFF, w.ctypes.data_as(C.POINTER(C.c_float))):
        raise XpngError("xpnghip_blur_weights: " + _err())
    return w


def _blur_record(name, b):
    """None or (sigma, radius, solarise_or_None) as a ViewBlur; the library checks the values"""
    if b is None:
        return ViewBlur(0.0, 0, SOLARISE_OFF, 0)
    if isinstance(b, ViewBlur):
        return b
    try:
        sigma, radius, sol = b
        return ViewBlur(float(sigma), int(radius) & 0xFFFFFFFF, SOLARISE_OFF if sol is None else float(sol), 0)
    except (TypeError, ValueError):
        raise XpngError(f"{name}: a blur is None or (sigma, radius, solarise_or_None), not {b!r}") from None


def resample_blur_host(raster, size, layout: int, dtype: int, scale=None, bias=None, rect=None, flip=False, filter: int = FILTER_TRIANGLE_AA,
                       colour=None, blur=None) -> bytes:
    """The rule of MixedContext.decode_batch_views_blur on the host (xpnghip_resample_blur_host; needs no device):
    resample_colour_host's arguments with filter 0, 1 or FILTER_CUBIC_AA (the rule of resample_cubic_host), plus blur = None or
    (sigma, radius, solarise_or_None).  The resampled and colour-transformed values of the view are blurred with the 2 * radius + 1
    taps of blur_weights(sigma, radius) on each axis over a reflected border (torch's "reflect") and clamped to 0 .. 255 - radius 0:
    no blur, and then sigma must be 0 -, then solarised where a threshold is given (b >= threshold: 255 - b), then the constants;
    alpha passes through untouched.  Returns the C * OH * OW elements of `dtype` in `layout` as raw bytes, bit for bit what the
    device call writes for these pixels."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_blur_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_blur_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    ra = _rect_array("resample_blur_host", None if rect is None else [rect], 1)
    cm = None if colour is None else (C.c_float * 12)(*_colour12("resample_blur_host", colour))
    rec = _blur_record("resample_blur_host", blur)
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_blur_host(px, r.ctypes.data, r.shape[1], r.shape[0], ra, int(flip), ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype,
                                            sc, bi, int(filter) & 0xFFFFFFFF, cm, C.byref(rec), buf.ctypes.data):
        raise XpngError("xpnghip_resample_blur_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


def _view_images(name, view_image, nviews):
    """the image of every view as a C array of uint32 (None stays None: the identity)"""
    if view_image is None:
        return None
    try:
        return (C.c_uint32 * max(nviews, 1))(*[int(i) & 0xFFFFFFFF for i in view_image])
    except (TypeError, ValueError):
        raise XpngError(f"{name}: view_image must be a sequence of image indices") from None


def view_tiles(dims, view_image, rects) -> list:
    """The launch list of MixedContext.decode_batch_views (xpnghip_view_tiles; host-only, needs no device): the tiles of the
    concatenated table of images dims[i] = (w, h) that some view of their image touches, by decreasing pixel count, equal sizes in
    table order.  view_image[v] is the image of view v (None: view v reads image v), rects[v] = (x, y, w, h) inside that image
    (rects None: whole images).  Raises XpngError on a bad index, rectangle or size."""
    dims = [(int(w), int(h)) for (w, h) in dims]
    nviews = len(dims) if view_image is None else len(list(view_image))
    vi = _view_images("view_tiles", None if view_image is None else list(view_image), nviews)
    ra = _rect_array("view_tiles", rects, nviews)
    ok = 0 < len(dims) <= 4096 and all(0 < v <= 1 << 24 for d in dims for v in d)
    cap = sum(_tile_count(w, h) for (w, h) in dims) if ok else 1
    flat, arr = (C.c_uint64 * max(2 * len(dims), 1))(*[v & 0xFFFFFFFFFFFFFFFF for d in dims for v in d]), (C.c_uint32 * max(cap, 1))()
    n = hip_lib().xpnghip_view_tiles(flat, len(dims), nviews, vi, ra, arr, cap)
    if n < 0:
        raise XpngError(f"view_tiles: bad arguments ({len(dims)} images, {nviews} views: an image index outside the batch, a rectangle that is "
                        "empty or leaves its image, or a side outside 1 .. 16777216)")
    return list(arr[:n])


FILTER_NEAREST = 3  # XPNGHIP_FILTER_NEAREST: the fourth filter word, which the affine entry points alone take (beside FILTER_BILINEAR)


def _affine6(name, m):
    """one inverse affine matrix - 6 numbers or a (2, 3) array, output coordinates to source coordinates - as 6 floats"""
    try:
        a = np.asarray(m, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.shape not in ((6,), (2, 3)):
        raise XpngError(f"{name}: an affine matrix is 6 numbers or a (2, 3) array, not {m!r}")
    return [float(np.float32(v)) for v in a.reshape(6)]


def _fill4(name, fill):
    """None (stays None: zeros), one number for every channel, or up to four numbers R, G, B, A (missing ones 0) as 4 floats"""
    if fill is None:
        return None
    try:
        v = [float(fill)] * 4 if not hasattr(fill, "__len__") else [float(x) for x in fill]
    except (TypeError, ValueError):
        v = None
    if v is None or not 1 <= len(v) <= 4:
        raise XpngError(f"{name}: fill is None, a number or up to four numbers R, G, B, A in byte units, not {fill!r}")
    return (C.c_float * 4)(*(v + [0.0] * (4 - len(v))))


def _size_pairs(name, sizes, n):
    """one (OH, OW) for every view or one pair per view as the C array of pairs {out_w, out_h}"""
    try:
        sizes = list(sizes)
        if len(sizes) == 2 and not hasattr(sizes[0], "__len__"):
            sizes = [sizes] * n
        if len(sizes) != n:
            raise XpngError(f"{name}: sizes has {len(sizes)} entries for {n} views")
        return (C.c_uint32 * max(2 * n, 1))(*[int(v) & 0xFFFFFFFF for (oh, ow) in sizes for v in (ow, oh)])
    except (TypeError, ValueError):
        raise XpngError(f"{name}: sizes must be (OH, OW) or one (OH, OW) per view, not {sizes!r}") from None


def affine_footprint(dim, matrix, size):
    """The footprint of one affine view (xpnghip_affine_footprint; host-only, needs no device): dim = (w, h) of the image, matrix
    the inverse 2 x 3 map, size = (OH, OW).  Returns (x, y, w, h), the rectangle of the image outside which every tap is the fill -
    the source coordinates of the four corner output pixels, widened by one pixel and by the second tap, clipped to the image -
    or (0, 0, 0, 0) when it is empty.  Raises XpngError on a matrix outside the entry bounds (include/xpng_hip.h)."""
    m = (C.c_float * 6)(*_affine6("affine_footprint", matrix))
    try:
        oh, ow = (int(v) for v in size)
        w, h = (int(v) for v in dim)
    except (TypeError, ValueError):
        raise XpngError(f"affine_footprint: dim must be (w, h) and size (OH, OW), not {dim!r}, {size!r}") from None
    r = (C.c_uint64 * 4)()
    if hip_lib().xpnghip_affine_footprint(w & 0xFFFFFFFFFFFFFFFF, h & 0xFFFFFFFFFFFFFFFF, m, ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, r):
        raise XpngError("xpnghip_affine_footprint: " + _err())
    return tuple(int(v) for v in r)


def affine_view_tiles(dims, view_image, matrices, sizes) -> list:
    """The launch list of MixedContext.decode_batch_views_affine (xpnghip_affine_view_tiles; host-only, needs no device): view_tiles
    with the footprint of every view (affine_footprint) in place of its rectangle; a view with an empty footprint selects nothing.
    matrices[v] is the inverse 2 x 3 map of view v, sizes one (OH, OW) for every view or one pair per view."""
    dims = [(int(w), int(h)) for (w, h) in dims]
    matrices = list(matrices)
    nviews = len(matrices)
    vi = _view_images("affine_view_tiles", None if view_image is None else list(view_image), nviews)
    if view_image is not None and len(list(view_image)) != nviews:
        raise XpngError(f"affine_view_tiles: view_image has {len(list(view_image))} entries for {nviews} matrices")
    am = (C.c_float * max(6 * nviews, 1))(*[x for v, m in enumerate(matrices) for x in _affine6(f"affine_view_tiles: matrices[{v}]", m)])
    so = _size_pairs("affine_view_tiles", sizes, nviews)
    ok = 0 < len(dims) <= 4096 and all(0 < v <= 1 << 24 for d in dims for v in d)
    cap = sum(_tile_count(w, h) for (w, h) in dims) if ok else 1
    flat, arr = (C.c_uint64 * max(2 * len(dims), 1))(*[v & 0xFFFFFFFFFFFFFFFF for d in dims for v in d]), (C.c_uint32 * max(cap, 1))()
    n = hip_lib().xpnghip_affine_view_tiles(flat, len(dims), nviews, vi, am, so, arr, cap)
    if n < 0:
        raise XpngError(f"affine_view_tiles: bad arguments ({len(dims)} images, {nviews} views: an image index outside the batch, a matrix outside "
                        "the entry bounds, an output size outside 1 .. 16384, or a side outside 1 .. 16777216)")
    return list(arr[:n])


def resample_affine_host(raster, size, matrix, layout: int, dtype: int, scale=None, bias=None, filter: int = FILTER_BILINEAR, fill=None,
                         colour=None) -> bytes:
    """The rule of MixedContext.decode_batch_views_affine on the host (xpnghip_resample_affine_host; needs no device): `raster` is
    an (h, w, 3|4) uint8 array in the file's form, size = (OH, OW), matrix the inverse 2 x 3 map from output to source coordinates
    (pixel centres at + 0.5; tensors.affine_matrix builds one).  filter is FILTER_BILINEAR - four taps, torchvision's affine() on a
    tensor - or FILTER_NEAREST (ties to even).  A tap outside the view's footprint or the image is `fill`: None (zeros), a number,
    or R, G, B, A in byte units.  colour is None or a colour matrix as resample_colour_host takes it.  There is no rect and no
    flip: the matrix carries both.  Returns the C * OH * OW elements of `dtype` in `layout` as raw bytes, bit for bit what the
    device call writes for these pixels."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_affine_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_affine_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    am = (C.c_float * 6)(*_affine6("resample_affine_host", matrix))
    fl = _fill4("resample_affine_host", fill)
    cm = None if colour is None else (C.c_float * 12)(*_colour12("resample_affine_host", colour))
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_affine_host(px, r.ctypes.data, r.shape[1], r.shape[0], am, ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype, sc, bi,
                                              int(filter) & 0xFFFFFFFF, fl, cm, buf.ctypes.data):
        raise XpngError("xpnghip_resample_affine_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


# the ops of a tone record (include/xpng_hip.h XPNGHIP_TONE_*)
TONE_NONE, TONE_AUTOCONTRAST, TONE_EQUALISE, TONE_POSTERISE, TONE_SOLARISE, TONE_INVERT = 0, 1, 2, 3, 4, 5


def _tone_record(name, t):
    """None or up to four (op, arg) pairs - a bare op stands for (op, 0) - as a ViewTone; the library checks the values"""
    if isinstance(t, ViewTone):
        return t
    rec = ViewTone()
    try:
        steps = [] if t is None else list(t)
        if len(steps) > 4:
            raise XpngError(f"{name}: a tone entry has at most four steps, not {len(steps)}")
        for i, st in enumerate(steps):
            op, arg = st if hasattr(st, "__len__") else (st, 0.0)
            rec.op[i], rec.arg[i] = int(op) & 0xFF if 0 <= int(op) <= 255 else 255, float(arg)
    except (TypeError, ValueError):
        raise XpngError(f"{name}: a tone entry is None or up to four (op, arg) pairs, not {t!r}") from None
    return rec


def resample_tone_host(raster, size, layout: int, dtype: int, scale=None, bias=None, rect=None, flip=False, filter: int = FILTER_TRIANGLE_AA,
                       colour=None, blur=None, tone=None) -> bytes:
    """The rule of MixedContext.decode_batch_views_tone on the host (xpnghip_resample_tone_host; needs no device):
    resample_blur_host's arguments plus tone = None or up to four (op, arg) steps, executed in order on the three colour planes of
    the values resample_blur_host would hand to the constants: TONE_AUTOCONTRAST, TONE_EQUALISE, (TONE_POSTERISE, bits),
    (TONE_SOLARISE, threshold), TONE_INVERT.  tone None gives resample_blur_host's bytes.  Returns the C * OH * OW elements of
    `dtype` in `layout` as raw bytes, bit for bit what the device call writes for these pixels."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_tone_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_tone_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    ra = _rect_array("resample_tone_host", None if rect is None else [rect], 1)
    cm = None if colour is None else (C.c_float * 12)(*_colour12("resample_tone_host", colour))
    rec = _blur_record("resample_tone_host", blur)
    tr = _tone_record("resample_tone_host", tone)
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_tone_host(px, r.ctypes.data, r.shape[1], r.shape[0], ra, int(flip), ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype,
                                            sc, bi, int(filter) & 0xFFFFFFFF, cm, C.byref(rec), C.byref(tr), buf.ctypes.data):
        raise XpngError("xpnghip_resample_tone_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


def resample_affine_tone_host(raster, size, matrix, layout: int, dtype: int, scale=None, bias=None, filter: int = FILTER_BILINEAR, fill=None,
                              colour=None, tone=None) -> bytes:
    """The rule of MixedContext.decode_batch_views_affine_tone on the host (xpnghip_resample_affine_tone_host; needs no device):
    resample_affine_host's arguments plus tone as resample_tone_host takes it.  The fill pixels take part in the statistics of
    autocontrast and equalise.  tone None gives resample_affine_host's bytes."""
    r = np.ascontiguousarray(raster, dtype=np.uint8)
    if r.ndim != 3 or r.shape[2] not in (3, 4):
        raise XpngError("resample_affine_tone_host: the raster must be (h, w, 3) or (h, w, 4) uint8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"resample_affine_tone_host: size must be (OH, OW), not {size!r}") from None
    px = r.shape[2]
    sc, bi, ch = _scale_bias(layout, px, scale, bias)
    am = (C.c_float * 6)(*_affine6("resample_affine_tone_host", matrix))
    fl = _fill4("resample_affine_tone_host", fill)
    cm = None if colour is None else (C.c_float * 12)(*_colour12("resample_affine_tone_host", colour))
    tr = _tone_record("resample_affine_tone_host", tone)
    ok = ch > 0 and 1 <= oh <= 16384 and 1 <= ow <= 16384          # (anything else the library refuses, naming the value)
    buf = np.empty(ch * oh * ow if ok else 1, dtype=np.uint32)     # 4-byte aligned, room for the widest element
    if hip_lib().xpnghip_resample_affine_tone_host(px, r.ctypes.data, r.shape[1], r.shape[0], am, ow & 0xFFFFFFFF, oh & 0xFFFFFFFF, layout, dtype, sc,
                                                   bi, int(filter) & 0xFFFFFFFF, fl, cm, C.byref(tr), buf.ctypes.data):
        raise XpngError("xpnghip_resample_affine_tone_host: " + _err())
    return buf.tobytes()[:ch * oh * ow * dtype_bytes(dtype)]


def quantize_host(src, npx: int, channels: int, layout: int, dtype: int, scale=None, bias=None) -> np.ndarray:
    """The quantisation rule of StagedImages.from_device on the host (xpnghip_quantize_host; needs no device): `src` is a tight
    buffer of channels * npx elements of `dtype` (0 = uint8, DTYPE_F16, DTYPE_BF16, DTYPE_F32) in `layout` (LAYOUT_PLANAR and
    LAYOUT_BGR bits only) - a numpy array of any element type of the right size (its bytes are what counts), or a host address.
    Returns the (npx, channels) uint8 array of interleaved R,G,B[,A] bytes, bit for bit what the device call stages for them."""
    if isinstance(src, int):
        addr = src
    else:
        keep = np.ascontiguousarray(src)
        addr = keep.ctypes.data
        es = 1 if dtype == 0 else hip_lib().xpnghip_dtype_bytes(dtype)
        if es > 0 and channels in (3, 4) and keep.nbytes != channels * npx * es:
            raise XpngError(f"quantize_host: the buffer holds {keep.nbytes} bytes, not {channels} * {npx} * {es}")
    sc, bi = _floats("scale", scale, 4), _floats("bias", bias, 4)
    out = np.empty((max(npx, 0), channels if channels in (3, 4) else 1), dtype=np.uint8)
    if hip_lib().xpnghip_quantize_host(layout, dtype, channels, addr, npx, sc, bi, out.ctypes.data):
        raise XpngError("xpnghip_quantize_host: " + _err())
    return out


def _tensor_args(ptrs, dims, channels):
    """the per-image arguments of the two device-buffer calls as C arrays"""
    k = len(ptrs)
    if len(dims) != k or len(channels) != k:
        raise XpngError(f"{k} buffers, {len(dims)} sizes and {len(channels)} channel counts: one of each per image")
    try:
        return ((C.c_void_p * max(k, 1))(*[int(p) for p in ptrs]), (C.c_uint64 * max(2 * k, 1))(*[int(v) for d in dims for v in d]),
                (C.c_uint8 * max(k, 1))(*[int(c) & 0xFF for c in channels]))
    except (TypeError, ValueError):
        raise XpngError("buffers are addresses, sizes are (w, h) and channel counts are integers") from None


def store_tensors(mode: int, ptrs, dims, channels, layout: int, dtype: int, paths, scale=None, bias=None, device: int = 0, stream=0) -> None:
    """xpng_store_tensors (include/xpng_store_tensors.h): file i is what store(mode, raster_i, paths[i]) writes for the quantised
    raster of device buffer ptrs[i] (dims[i] = (w, h), channels[i] = 3 or 4; layout, dtype, scale, bias as in
    StagedImages.from_device).  The pixels stay on the device; the call is ordered behind `stream`."""
    k = len(ptrs)
    if len(paths) != k:
        raise XpngError(f"store_tensors: {k} buffers and {len(paths)} paths")
    p, flat, ch = _tensor_args(ptrs, dims, channels)
    sc, bi = _floats("scale", scale, 4), _floats("bias", bias, 4)
    arr = (C.c_char_p * max(k, 1))(*[os.fsencode(q) for q in paths])
    if host_lib().xpng_store_tensors(mode, k, p, flat, ch, layout, dtype, sc, bi, device, stream, arr):
        raise XpngError("xpng_store_tensors failed: " + _err())


def store_batch(mode: int, rasters, paths) -> None:
    """xpng_store_batch (include/xpng_store_batch.h): file i is what store(mode, rasters[i], paths[i]) writes; the tile stage of
    all images of one (tile mode, bytes per pixel) is one mixed-size device call."""
    k = len(rasters)
    assert len(paths) == k
    rs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rasters]
    pms = (XpngT * max(k, 1))(*[XpngT(r.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[1], r.shape[0], r.size, r.shape[2] == 4) for r in rs])
    arr = (C.c_char_p * max(k, 1))(*[os.fsencode(p) for p in paths])
    if host_lib().xpng_store_batch(mode, pms, arr, k):
        raise XpngError("xpng_store_batch failed")


class StagedImages:
    """The staged batch of xpng_store_batch (xpnghip_images_begin .. _end): a list of (h, w, 3|4) uint8 rasters of any sizes,
    uploaded once and normalised on the device.  pxsz[i] = bytes per pixel of the normalised raster i."""

    def __init__(self, rasters, lib=None):
        self._lib = lib or hip_lib()
        rs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rasters]
        k = self.n = len(rs)
        self.dims = [(r.shape[1], r.shape[0]) for r in rs]
        ptrs = (C.c_void_p * max(k, 1))(*[r.ctypes.data for r in rs])
        flat = (C.c_uint64 * max(2 * k, 1))(*[v for d in self.dims for v in d])
        pin, pout = (C.c_uint8 * max(k, 1))(*[r.shape[2] for r in rs]), (C.c_uint8 * max(k, 1))()
        self._h = C.c_void_p()
        if self._lib.xpnghip_images_begin(C.byref(self._h), k, ptrs, flat, pin, pout):
            raise XpngError("xpnghip_images_begin: " + self._lib.xpnghip_last_error().decode(errors="replace"))
        self.pxsz = list(pout)[:k]

    @classmethod
    def from_device(cls, ptrs, dims, channels, layout: int = 0, dtype: int = 0, scale=None, bias=None, device: int = 0, stream=0, lib=None):
        """The staged batch filled from device buffers (xpnghip_images_begin_device): ptrs[i] is a tight buffer of
        channels[i] * w * h elements (dims[i] = (w, h), channels[i] = 3 or 4) of `dtype` (0 = uint8, DTYPE_F16, DTYPE_BF16,
        DTYPE_F32) in `layout` (LAYOUT_PLANAR and LAYOUT_BGR bits only), aligned to its element.  A float element x is staged as
        round-half-to-even(clamp(fmaf(x, scale[c], bias[c]), 0, 255)) with c the channel's position in the buffer (scale, bias: a
        number or four numbers; None = 1 and 0; not allowed with dtype 0).  The staging kernel is queued on `stream`; when the call
        returns the buffers are free again.  Everything else is StagedImages."""
        self = cls.__new__(cls)
        self._lib = lib or hip_lib()
        self._h = C.c_void_p()
        k = self.n = len(ptrs)
        p, flat, ch = _tensor_args(ptrs, dims, channels)
        self.dims = [(int(w), int(h)) for (w, h) in dims]
        sc, bi = _floats("scale", scale, 4), _floats("bias", bias, 4)
        pout = (C.c_uint8 * max(k, 1))()
        if self._lib.xpnghip_images_begin_device(C.byref(self._h), device, k, p, flat, ch, layout, dtype, sc, bi, stream, pout):
            assert not self._h
            raise XpngError("xpnghip_images_begin_device: " + self._lib.xpnghip_last_error().decode(errors="replace"))
        self.pxsz = list(pout)[:k]
        return self

    def _fail(self, what):
        raise XpngError(what + ": " + self._lib.xpnghip_last_error().decode(errors="replace"))

    def single_colour(self) -> list:
        out = (C.c_uint8 * self.n)()
        if self._lib.xpnghip_images_single_colour(self._h, out):
            self._fail("xpnghip_images_single_colour")
        return [bool(v) for v in out]

    def first_pixel(self, i: int) -> bytes:
        """After single_colour(): the first pixel of normalised raster i."""
        out = (C.c_uint8 * 4)()
        if self._lib.xpnghip_images_first_pixel(self._h, i, out):
            self._fail("xpnghip_images_first_pixel")
        return bytes(out[: self.pxsz[i]])

    def fetch(self, i: int) -> np.ndarray:
        w, h = self.dims[i]
        out = np.zeros((h, w, self.pxsz[i]), dtype=np.uint8)
        if self._lib.xpnghip_images_fetch(self._h, i, out.ctypes.data_as(C.c_void_p)):
            self._fail("xpnghip_images_fetch")
        return out

    def encode(self, modes) -> list:
        """modes[i] = 0 (skip), 1 or 2 -> list of tile blobs (bytes), None for the skipped images."""
        assert len(modes) == self.n
        m, blobs, lens = (C.c_uint8 * self.n)(*modes), (C.POINTER(C.c_uint8) * self.n)(), (C.c_uint64 * self.n)()
        if self._lib.xpnghip_images_encode(self._h, m, blobs, lens):
            assert not any(bool(b) for b in blobs)
            self._fail("xpnghip_images_encode")
        out = []
        for b, n in zip(blobs, lens):
            out.append(C.string_at(b, n) if b else None)
            if b:
                _libc.free(b)
        return out

    def end(self):
        if self._h:
            self._lib.xpnghip_images_end(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


def normalize_device(d_rgba: int, npx: int, d_out: int, stream=0):
    """normalize_RGBA (libxpng.c:688-721) on a device-resident RGBA raster -> (bytes per pixel, rewritten into d_out?)."""
    pxsz, rew = C.c_int(0), C.c_int(0)
    if hip_lib().xpnghip_normalize_device(d_rgba, npx, d_out, C.byref(pxsz), C.byref(rew), stream):
        raise XpngError("xpnghip_normalize_device: " + _err())
    return pxsz.value, bool(rew.value)


class _Handle:
    """What both kinds of context do with their xpnghip_ctx handle (self._h)."""

    def close(self):
        if self._h:
            hip_lib().xpnghip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tile(self, i: int):
        a = (C.c_uint64 * 4)()
        if hip_lib().xpnghip_ctx_tile(self._h, i, a):
            raise IndexError(i)
        return tuple(a)

    def workspace_bytes(self) -> int:
        return hip_lib().xpnghip_ctx_workspace_bytes(self._h)

    def decode_status(self, stream=0) -> int:
        """Synchronise and report whether the last decode accepted every tile header (0) or rejected some (1)."""
        return hip_lib().xpnghip_ctx_decode_status(self._h, stream)


class Context(_Handle):
    """xpnghip_ctx: tile table + device workspace for one raster geometry on one GPU.  Device pointers are
    plain integers (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t handle or 0."""

    FETCH = {"pr": 0, "nl": 1, "r": 2, "g": 3, "b": 4, "a": 5, "k": 19, "sums": 30}

    def __init__(self, w: int, h: int, pxsz: int, device: int = 0, batch: int = 1, tile_range=None):
        self.w, self.h, self.pxsz, self.device, self.batch = w, h, pxsz, device, batch
        self._h = C.c_void_p()
        r0, r1 = tile_range if tile_range else (0, (1 << 64) - 1)
        if hip_lib().xpnghip_ctx_create_range(C.byref(self._h), device, w, h, pxsz, batch, r0, r1):
            raise XpngError("xpnghip_ctx_create_range: " + _err())
        self.n_tiles = hip_lib().xpnghip_ctx_tile_count(self._h)

    def tiles(self):
        return [self.tile(i) for i in range(self.n_tiles)]

    def blob_bound(self, t0=0, t1=None) -> int:
        return hip_lib().xpnghip_ctx_blob_bound(self._h, t0, self.n_tiles if t1 is None else t1)

    def encode_device(self, mode, d_raster: int, d_blobs: int, t0=0, t1=None, stream=0, sync=True) -> int:
        n = C.c_uint64()
        rc = hip_lib().xpnghip_encode_device(self._h, mode, d_raster, t0, self.n_tiles if t1 is None else t1, d_blobs,
                                             C.byref(n) if sync else None, stream)
        if rc:
            raise XpngError("xpnghip_encode_device: " + _err())
        return n.value

    def encode_device_batch(self, mode, d_rasters, d_blobs, t0=0, t1=None, stream=0, sync=True):
        """d_rasters / d_blobs: sequences of device pointers (one per image, <= batch).  Returns the list of blob lengths
        (sync=True) or None."""
        k = len(d_rasters)
        ins, outs, lens = (C.c_void_p * k)(*d_rasters), (C.c_void_p * k)(*d_blobs), (C.c_uint64 * k)()
        rc = hip_lib().xpnghip_encode_device_batch(self._h, mode, ins, k, t0, self.n_tiles if t1 is None else t1, outs,
                                                   lens if sync else None, stream)
        if rc:
            raise XpngError("xpnghip_encode_device_batch: " + _err())
        return list(lens) if sync else None

    def decode_device_batch(self, mode, d_blobs, blob_lens, tile_offs, d_rasters, t0=0, t1=None, stream=0):
        """blob_lens: bytes of each blob buffer; tile_offs: per image, the blob start offsets of tiles [t0, t1)."""
        k = len(d_blobs)
        t1 = self.n_tiles if t1 is None else t1
        off_arr = None   # tile_offs None: the size walk (libxpng.c:982) runs on the device
        if tile_offs is not None:
            flat = [o for offs in tile_offs for o in offs]
            assert len(flat) == k * (t1 - t0)
            key = (tuple(flat), t0, t1)
            if getattr(self, "_off_key", None) != key:
                self._off_key, self._off_arr = key, (C.c_uint64 * len(flat))(*flat)
            off_arr = self._off_arr
        ins, outs, lens = (C.c_void_p * k)(*d_blobs), (C.c_void_p * k)(*d_rasters), (C.c_uint64 * k)(*blob_lens)
        if hip_lib().xpnghip_decode_device_batch(self._h, mode, ins, lens, k, off_arr, t0, t1, outs, stream):
            raise XpngError("xpnghip_decode_device_batch: " + _err())

    def decode_region_batch(self, mode, d_blobs, blob_lens, rects, d_outs, out_bpr, tile_offs=None, stream=0):
        """One region decode launch (xpnghip_decode_region_device_batch): image i's rects[i] = (x, y, w, h) crop goes to
        d_outs[i] at row pitch out_bpr.  tile_offs None: the size walk runs on the device; else per image the blob offsets of
        ALL its tiles."""
        k = len(d_blobs)
        assert len(blob_lens) == k and len(rects) == k and len(d_outs) == k
        off_arr = None
        if tile_offs is not None:
            flat = [o for offs in tile_offs for o in offs]
            assert len(flat) == k * self.n_tiles
            off_arr = (C.c_uint64 * len(flat))(*flat)
        flat_r = [int(v) for r in rects for v in r]
        ins, outs, lens = (C.c_void_p * k)(*d_blobs), (C.c_void_p * k)(*d_outs), (C.c_uint64 * k)(*blob_lens)
        if hip_lib().xpnghip_decode_region_device_batch(self._h, mode, ins, lens, k, off_arr, (C.c_uint64 * (4 * k))(*flat_r),
                                                        outs, out_bpr, stream):
            raise XpngError("xpnghip_decode_region_device_batch: " + _err())

    def last_blobs_len(self) -> int:
        return hip_lib().xpnghip_ctx_last_blobs_len(self._h)

    def decode_device(self, mode, d_blobs: int, blobs_len: int, tile_off, d_raster: int, t0=0, t1=None, stream=0):
        t1 = self.n_tiles if t1 is None else t1
        arr = (C.c_uint64 * (t1 - t0))(*tile_off) if tile_off is not None else None
        if hip_lib().xpnghip_decode_device(self._h, mode, d_blobs, blobs_len, arr, t0, t1, d_raster, stream):
            raise XpngError("xpnghip_decode_device: " + _err())

    def transform_device(self, d_raster: int, t0=0, t1=None, stream=0):
        if hip_lib().xpnghip_m1_transform_device(self._h, d_raster, t0, self.n_tiles if t1 is None else t1, stream):
            raise XpngError("xpnghip_m1_transform_device: " + _err())

    def transform_device_batch(self, d_rasters, t0=0, t1=None, stream=0):
        k = len(d_rasters)
        ins = (C.c_void_p * k)(*d_rasters)
        if hip_lib().xpnghip_m1_transform_device_batch(self._h, ins, k, t0, self.n_tiles if t1 is None else t1, stream):
            raise XpngError("xpnghip_m1_transform_device_batch: " + _err())

    def fetch(self, what, tile: int, cap: int = 1 << 22) -> np.ndarray:
        code = self.FETCH[what] if isinstance(what, str) else what
        buf = np.zeros(cap, dtype=np.uint8)
        n = hip_lib().xpnghip_debug_fetch(self._h, code, tile, buf.ctypes.data_as(C.c_void_p), cap)
        if n < 0:
            raise XpngError(f"debug_fetch({what}, {tile}) failed")
        return buf[:n].copy()


class MixedContext(_Handle):
    """A mixed-size context (xpnghip_ctx_create_mixed): images of different sizes, dims[i] = (w, h), one pixel size, decoded or
    encoded by ONE device call.  Device pointers are plain integers; `stream` is a hipStream_t handle or 0."""

    def __init__(self, dims, pxsz: int, device: int = 0):
        self.dims, self.pxsz, self.device = [(int(w), int(h)) for (w, h) in dims], pxsz, device
        self.nimg = len(self.dims)
        self._h = C.c_void_p()
        flat = (C.c_uint64 * max(2 * self.nimg, 1))(*[v for d in self.dims for v in d])
        if hip_lib().xpnghip_ctx_create_mixed(C.byref(self._h), device, flat, self.nimg, pxsz):
            raise XpngError("xpnghip_ctx_create_mixed: " + _err())
        self.n_tiles = hip_lib().xpnghip_ctx_tile_count(self._h)
        self.first_tile = [hip_lib().xpnghip_ctx_mixed_first_tile(self._h, i) for i in range(self.nimg + 1)]

    def blob_bound(self, i: int) -> int:
        """Capacity the blob buffer of image i needs (xpnghip_ctx_blob_bound over the image's span of the concatenated table)."""
        return hip_lib().xpnghip_ctx_blob_bound(self._h, self.first_tile[i], self.first_tile[i + 1])

    def encode_batch(self, mode, d_rasters, d_blobs, in_bpr=0, stream=0, sync=True):
        """One launch sequence over every tile of every image (xpnghip_encode_varsize_device_batch).  in_bpr != 0: every
        d_rasters[i] holds its rows at this pitch; 0: tight rasters.  Returns the list of blob lengths (sync=True) or None (read
        them with last_blobs_len_at after synchronising)."""
        return self._encode("xpnghip_encode_varsize_device_batch", mode, d_rasters, in_bpr, d_blobs, stream, sync)

    def _encode(self, symbol, mode, d_rasters, form, d_blobs, stream, sync):
        """the marshalling of both encode calls; form = the row pitch or the layout word, the argument in which they differ"""
        k = len(d_rasters)
        ins, outs, lens = (C.c_void_p * k)(*d_rasters), (C.c_void_p * len(d_blobs))(*d_blobs), (C.c_uint64 * max(k, 1))()
        if getattr(hip_lib(), symbol)(self._h, mode, ins, form, k, outs, lens if sync else None, stream):
            raise XpngError(symbol + ": " + _err())
        return list(lens)[:k] if sync else None

    def last_blobs_len_at(self, i: int) -> int:
        return hip_lib().xpnghip_ctx_last_blobs_len_at(self._h, i)

    def decode_batch(self, mode, d_blobs, lens, d_outs, out_bpr=0, tile_offs=None, stream=0):
        """One launch over every tile of every image (xpnghip_decode_mixed_device_batch).  out_bpr != 0: every d_outs[i] is
        written at this row pitch; 0: tight rasters.  tile_offs None: the size walk runs on the device; else per image the blob
        offsets of its tiles."""
        self._decode("xpnghip_decode_mixed_device_batch", mode, d_blobs, lens, d_outs, tile_offs, stream, out_bpr)

    def _decode(self, symbol, mode, d_blobs, lens, d_outs, tile_offs, stream, *between, before=()):
        """the marshalling of every decode call; between = the arguments of this form, which sit between d_outs and stream (before:
        those of the views call in front of d_outs)"""
        k = len(d_blobs)
        off_arr = None
        if tile_offs is not None:
            flat = [o for offs in tile_offs for o in offs]
            assert len(flat) == self.n_tiles
            off_arr = (C.c_uint64 * len(flat))(*flat)
        ins, outs, ln = (C.c_void_p * k)(*d_blobs), (C.c_void_p * len(d_outs))(*d_outs), (C.c_uint64 * len(lens))(*lens)
        if getattr(hip_lib(), symbol)(self._h, mode, ins, ln, k, off_arr, *before, outs, *between, stream):
            raise XpngError(symbol + ": " + _err())

    def decode_batch_as(self, mode, d_blobs, lens, d_outs, layout, tile_offs=None, stream=0):
        """decode_batch in its tight form, with every d_outs[i] written in `layout` (api.layout(); C * w * h bytes at any
        alignment): xpnghip_decode_varsize_device_batch_as."""
        self._decode("xpnghip_decode_varsize_device_batch_as", mode, d_blobs, lens, d_outs, tile_offs, stream, layout)

    def decode_batch_as_float(self, mode, d_blobs, lens, d_outs, layout, dtype, scale=None, bias=None, tile_offs=None, stream=0):
        """decode_batch_as with every d_outs[i] written as C * w * h elements of `dtype` (DTYPE_F16, DTYPE_BF16, DTYPE_F32), aligned
        to the element: element = fmaf(byte, scale[c], bias[c]) rounded to nearest even, c the channel's position in the buffer.
        scale / bias: one number per channel of the buffers or None (ones / zeros): xpnghip_decode_varsize_device_batch_as_float."""
        sc, bi, _ = _scale_bias(layout, self.pxsz, scale, bias)
        self._decode("xpnghip_decode_varsize_device_batch_as_float", mode, d_blobs, lens, d_outs, tile_offs, stream, layout, dtype, sc, bi)

    def decode_batch_resized(self, mode, d_blobs, lens, d_outs, layout, dtype, size, scale=None, bias=None, rects=None, flips=None,
                             tile_offs=None, stream=0):
        """decode_batch_as_float with a crop, a bilinear resize and a left-right flip in the copy-out: every d_outs[i] is
        C * OH * OW elements of `dtype`, size = (OH, OW), the resampling of rects[i] = (x, y, w, h) of image i (None: every whole
        image), mirrored where flips[i] is true (None: none): xpnghip_decode_varsize_device_batch_resized."""
        k = len(d_blobs)
        try:
            oh, ow = (int(v) & 0xFFFFFFFF for v in size)
        except (TypeError, ValueError):
            raise XpngError(f"decode_batch_resized: size must be (OH, OW), not {size!r}") from None
        sc, bi, _ = _scale_bias(layout, self.pxsz, scale, bias)
        ra = _rect_array("decode_batch_resized", rects, k)
        fl = _flip_array("decode_batch_resized", flips, k)
        self._decode("xpnghip_decode_varsize_device_batch_resized", mode, d_blobs, lens, d_outs, tile_offs, stream, layout, dtype, sc, bi, ra, fl, ow, oh)

    def decode_batch_resampled(self, mode, d_blobs, lens, d_outs, layout, dtype, size, scale=None, bias=None, rects=None, flips=None,
                               filter: int = FILTER_TRIANGLE_AA, tile_offs=None, stream=0):
        """decode_batch_resized with a filter word: FILTER_BILINEAR is that call itself, the same kernel and the same bytes;
        FILTER_TRIANGLE_AA resamples every axis that shrinks with a triangle filter of the ratio's half-width, clamped to the
        rectangle and renormalised - an antialiased downscale, F.interpolate(mode="bilinear", antialias=True) of the cropped
        rectangle up to the order of summation: xpnghip_decode_varsize_device_batch_resampled (the rule is in include/xpng_hip.h)."""
        k = len(d_blobs)
        try:
            oh, ow = (int(v) & 0xFFFFFFFF for v in size)
        except (TypeError, ValueError):
            raise XpngError(f"decode_batch_resampled: size must be (OH, OW), not {size!r}") from None
        sc, bi, _ = _scale_bias(layout, self.pxsz, scale, bias)
        ra = _rect_array("decode_batch_resampled", rects, k)
        fl = _flip_array("decode_batch_resampled", flips, k)
        self._decode("xpnghip_decode_varsize_device_batch_resampled", mode, d_blobs, lens, d_outs, tile_offs, stream, layout, dtype, sc, bi, ra, fl, ow, oh,
                     int(filter) & 0xFFFFFFFF)

    def _view_args(self, name, view_image, sizes, layout, scale, bias, n):
        """what every views call of n views marshals alike: view_image, the size pairs and the constants"""
        vi = _view_images(name, None if view_image is None else list(view_image), n)
        if view_image is not None and len(list(view_image)) != n:
            raise XpngError(f"{name}: view_image has {len(list(view_image))} entries for {n} output buffers")
        so = None if sizes is None else _size_pairs(name, sizes, n)
        sc, bi, _ = _scale_bias(layout, self.pxsz, scale, bias)
        return vi, so, sc, bi

    def _views(self, name, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale, bias, rects, flips, tile_offs, stream, colours, filter,
               blurs=None):
        """the marshalling of the views calls; filter _CUBIC: the cubic call, which has no filter word and always takes `colours`;
        blurs not None: the blur call, which takes a filter word, `colours` and the records"""
        n = len(d_outs)
        br = None
        if blurs is not None:
            blurs = list(blurs)
            if len(blurs) != n:
                raise XpngError(f"{name}: blurs has {len(blurs)} entries for {n} views")
            br = (ViewBlur * max(n, 1))(*[_blur_record(f"{name}: blurs[{v}]", b) for v, b in enumerate(blurs)])
        cm = _colour_table(name, colours, n)
        vi, so, sc, bi = self._view_args(name, view_image, sizes, layout, scale, bias, n)
        ra = _rect_array(name, rects, n)
        fl = _flip_array(name, flips, n, "views")
        if name == "decode_batch_views_blur":
            self._decode("xpnghip_decode_varsize_device_batch_views_blur", mode, d_blobs, lens, d_outs, tile_offs, stream, so, ra, fl, layout, dtype,
                         sc, bi, int(filter) & 0xFFFFFFFF, cm, br, before=(n, vi))
            return
        if filter is _CUBIC:
            self._decode("xpnghip_decode_varsize_device_batch_views_cubic", mode, d_blobs, lens, d_outs, tile_offs, stream, so, ra, fl, layout, dtype,
                         sc, bi, cm, before=(n, vi))
            return
        if cm is not None:
            self._decode("xpnghip_decode_varsize_device_batch_views_colour", mode, d_blobs, lens, d_outs, tile_offs, stream, so, ra, fl, layout, dtype,
                         sc, bi, int(filter) & 0xFFFFFFFF, cm, before=(n, vi))
            return
        self._decode("xpnghip_decode_varsize_device_batch_views", mode, d_blobs, lens, d_outs, tile_offs, stream, so, ra, fl, layout, dtype, sc, bi,
                     int(filter) & 0xFFFFFFFF, before=(n, vi))

    def decode_batch_views(self, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale=None, bias=None, rects=None, flips=None,
                           filter: int = FILTER_TRIANGLE_AA, tile_offs=None, stream=0, colours=None):
        """decode_batch_resampled with any number of outputs per image, and only the tiles they touch decoded: view v reads image
        view_image[v] (None: view v reads image v), its rectangle rects[v] = (x, y, w, h) (None: whole images), mirrored where
        flips[v] is true, resampled to its own size: `sizes` is one (OH, OW) for every view or one pair per view.  d_outs[v] is
        C * OH_v * OW_v elements of `dtype`: xpnghip_decode_varsize_device_batch_views (the rule is in include/xpng_hip.h).
        colours is None or one entry per view, each None (the identity matrix) or a colour matrix of 12 numbers or a (3, 4) array as
        resample_colour_host takes it: the copy-out then puts every pixel of view v through matrix v and a clamp to 0 .. 255
        before the constants (xpnghip_decode_varsize_device_batch_views_colour).  colours None, or every entry None, is the
        plain call."""
        self._views("decode_batch_views", mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale, bias, rects, flips, tile_offs, stream,
                    colours, filter)

    def decode_batch_views_cubic(self, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale=None, bias=None, rects=None, flips=None,
                                 tile_offs=None, stream=0, colours=None):
        """decode_batch_views without `filter`: every view is resampled with the antialiased bicubic of resample_cubic_host - Keys'
        cubic, a = -0.5, stretched where an axis shrinks, clamped to the rectangle, the values clamped to 0 .. 255 - and view v
        equals that function's bytes.  The selection of tiles, sizes, rects, flips and colours (a None entry beside a matrix is the
        identity matrix, which here gives the bits of no matrix) are decode_batch_views':
        xpnghip_decode_varsize_device_batch_views_cubic (the rule is in include/xpng_hip.h)."""
        self._views("decode_batch_views_cubic", mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale, bias, rects, flips, tile_offs,
                    stream, colours, _CUBIC)

    def decode_batch_views_blur(self, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale=None, bias=None, rects=None, flips=None,
                                filter: int = FILTER_TRIANGLE_AA, tile_offs=None, stream=0, colours=None, blurs=None):
        """decode_batch_views plus a Gaussian blur and a solarise per view: blurs is None or one entry per view, each None (neither)
        or (sigma, radius, solarise_or_None) as resample_blur_host takes it, and view v equals that function's bytes.  filter is
        0, 1 or FILTER_CUBIC_AA (the rule of decode_batch_views_cubic).  Views with a None entry are written by the copy-out
        kernel of the underlying call; the others take a second kernel over fp32 planes in the context's workspace
        (C * OH * OW floats per such view).  blurs None is the underlying call itself:
        xpnghip_decode_varsize_device_batch_views_blur (the rule is in include/xpng_hip.h)."""
        self._views("decode_batch_views_blur", mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale, bias, rects, flips, tile_offs,
                    stream, colours, filter, blurs)

    def decode_batch_views_affine(self, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, matrices, scale=None, bias=None,
                                  filter: int = FILTER_BILINEAR, fill=None, tile_offs=None, stream=0, colours=None):
        """decode_batch_views under an affine map per view: matrices[v] is the inverse 2 x 3 map of view v, from its output
        coordinates to source coordinates of its whole image (tensors.affine_matrix builds one from a rectangle, a size, an angle,
        a translation, a scale, a shear and a flip), in place of rects and flips.  filter is FILTER_BILINEAR or FILTER_NEAREST;
        a tap outside the view's footprint is `fill` (None, a number, or R, G, B, A in byte units; one for the call).  Only the
        tiles that some view's footprint touches are decoded (affine_view_tiles), and view v equals resample_affine_host's bytes.
        sizes, view_image and colours are decode_batch_views': xpnghip_decode_varsize_device_batch_views_affine (the rule is in
        include/xpng_hip.h)."""
        name = "decode_batch_views_affine"
        n = len(d_outs)
        matrices = list(matrices)
        if len(matrices) != n:
            raise XpngError(f"{name}: matrices has {len(matrices)} entries for {n} views")
        am = (C.c_float * max(6 * n, 1))(*[x for v, m in enumerate(matrices) for x in _affine6(f"{name}: matrices[{v}]", m)])
        cm = _colour_table(name, colours, n)
        vi, so, sc, bi = self._view_args(name, view_image, sizes, layout, scale, bias, n)
        self._decode("xpnghip_decode_varsize_device_batch_views_affine", mode, d_blobs, lens, d_outs, tile_offs, stream, so, am, _fill4(name, fill), layout,
                     dtype, sc, bi, int(filter) & 0xFFFFFFFF, cm, before=(n, vi))

    def _tone_table(self, name, tones, n):
        """tones (None stays None) as the C array of n records"""
        if tones is None:
            return None
        tones = list(tones)
        if len(tones) != n:
            raise XpngError(f"{name}: tones has {len(tones)} entries for {n} views")
        return (ViewTone * max(n, 1))(*[_tone_record(f"{name}: tones[{v}]", t) for v, t in enumerate(tones)])

    def decode_batch_views_tone(self, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, scale=None, bias=None, rects=None, flips=None,
                                filter: int = FILTER_TRIANGLE_AA, tile_offs=None, stream=0, colours=None, blurs=None, tones=None):
        """decode_batch_views_blur plus tone steps per view: tones is None or one entry per view, each None or a list of up to four
        (op, arg) pairs as resample_tone_host takes them, and view v equals that function's bytes.  A view with a step takes the
        second pass over fp32 planes in the context's workspace, where its statistics are reduced and its steps applied in place.
        tones None, or every entry None, is decode_batch_views_blur itself:
        xpnghip_decode_varsize_device_batch_views_tone (the rule is in include/xpng_hip.h)."""
        name = "decode_batch_views_tone"
        n = len(d_outs)
        br = None
        if blurs is not None:
            blurs = list(blurs)
            if len(blurs) != n:
                raise XpngError(f"{name}: blurs has {len(blurs)} entries for {n} views")
            br = (ViewBlur * max(n, 1))(*[_blur_record(f"{name}: blurs[{v}]", b) for v, b in enumerate(blurs)])
        tr = self._tone_table(name, tones, n)
        cm = _colour_table(name, colours, n)
        vi, so, sc, bi = self._view_args(name, view_image, sizes, layout, scale, bias, n)
        ra = _rect_array(name, rects, n)
        fl = _flip_array(name, flips, n, "views")
        self._decode("xpnghip_decode_varsize_device_batch_views_tone", mode, d_blobs, lens, d_outs, tile_offs, stream, so, ra, fl, layout, dtype,
                     sc, bi, int(filter) & 0xFFFFFFFF, cm, br, tr, before=(n, vi))

    def decode_batch_views_affine_tone(self, mode, d_blobs, lens, view_image, d_outs, layout, dtype, sizes, matrices, scale=None, bias=None,
                                       filter: int = FILTER_BILINEAR, fill=None, tile_offs=None, stream=0, colours=None, tones=None):
        """decode_batch_views_affine plus tone steps per view, as decode_batch_views_tone takes them; the fill pixels take part in
        the statistics.  View v equals resample_affine_tone_host's bytes; tones None is decode_batch_views_affine itself:
        xpnghip_decode_varsize_device_batch_views_affine_tone (the rule is in include/xpng_hip.h)."""
        name = "decode_batch_views_affine_tone"
        n = len(d_outs)
        matrices = list(matrices)
        if len(matrices) != n:
            raise XpngError(f"{name}: matrices has {len(matrices)} entries for {n} views")
        am = (C.c_float * max(6 * n, 1))(*[x for v, m in enumerate(matrices) for x in _affine6(f"{name}: matrices[{v}]", m)])
        tr = self._tone_table(name, tones, n)
        cm = _colour_table(name, colours, n)
        vi, so, sc, bi = self._view_args(name, view_image, sizes, layout, scale, bias, n)
        self._decode("xpnghip_decode_varsize_device_batch_views_affine_tone", mode, d_blobs, lens, d_outs, tile_offs, stream, so, am,
                     _fill4(name, fill), layout, dtype, sc, bi, int(filter) & 0xFFFFFFFF, cm, tr, before=(n, vi))

    def last_decode_tiles(self) -> int:
        """tile work items of the context's most recent decode launch (xpnghip_ctx_last_decode_tiles): n_tiles after the other
        decode calls, len(view_tiles(...)) after decode_batch_views, 0 before any decode"""
        return hip_lib().xpnghip_ctx_last_decode_tiles(self._h)

    def encode_batch_from(self, mode, d_rasters, layout, d_blobs, stream=0, sync=True):
        """encode_batch in its tight form, with every d_rasters[i] read in `layout` (api.layout(); its channels must be the
        context's): xpnghip_encode_varsize_device_batch_from.  Returns the list of blob lengths (sync=True) or None."""
        return self._encode("xpnghip_encode_varsize_device_batch_from", mode, d_rasters, layout, d_blobs, stream, sync)


def walk_tile_offsets(blobs: bytes, n_tiles: int):
    """Serial size walk of the reference decoder (libxpng.c:982): blob start offsets of every tile."""
    off, o = [], 0
    for _ in range(n_tiles):
        off.append(o)
        o += int.from_bytes(blobs[o:o + 4], "little") & 0xFFFFFF
    return off, o
