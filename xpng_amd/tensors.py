"""torch front end: .xpng files -> device tensors in the layout and the data type a model reads, the pixels never leaving HBM
(load_files), and device tensors -> .xpng files the same way back (store_files).

`load_files` is what `api.load_batch` is for host arrays.  The files that reach the tile codec are grouped by (tile mode, bytes per
pixel) and every group is decoded by mixed-size device calls straight into tensors of the final layout
(MixedContext.decode_batch_as: the layout is written by the copy-out pass of the decode, include/xpng_hip.h XPNGHIP_LAYOUT_*;
MixedContext.decode_batch_as_float when a float dtype is asked for: the same pass converts and normalises, XPNGHIP_DTYPE_*;
MixedContext.decode_batch_resized when an output size is asked for: the same pass also crops, resizes and flips;
MixedContext.decode_batch_resampled when that resize is to antialias).
`load_views` gives any number of crops per file from ONE decode of it, and decodes only the tiles they touch
(MixedContext.decode_batch_views); with colour= every view also gets a colour matrix of its own in the same pass (colour_matrix,
random_colour_jitter), and with blur= and solarise= a Gaussian blur and a solarise of its own in a second kernel of that call
(MixedContext.decode_batch_views_blur; random_gaussian_blur, random_solarise); with affine= every view is rotated, sheared, scaled
and translated in the copy-out instead (MixedContext.decode_batch_views_affine; affine_matrix, random_affine); with tone= a view is
autocontrasted, equalised, posterised, solarised and inverted, up to four steps in any order, behind either
(MixedContext.decode_batch_views_tone, decode_batch_views_affine_tone; random_tone).
api.py stays free of torch; this module is the only one of the package that imports it at load time."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import api
from .api import XpngError

BATCH_MAX, BATCH_BYTES = 4096, 2 << 30  # the budget of one device call: xpng_load_batch's (csrc/host/xpng_api.c)


def _arrange(t: torch.Tensor, layout: str, channels, bgr: bool) -> torch.Tensor:
    """(h, w, 3|4) uint8 in the file's form -> the requested layout, with torch ops"""
    px = t.shape[2]
    if channels == 4 and px == 3:
        t = torch.cat([t, torch.full_like(t[..., :1], 255)], dim=2)
    elif channels == 3 and px == 4:
        t = t[..., :3]
    if bgr:
        t = t[..., [2, 1, 0] + ([3] if t.shape[2] == 4 else [])]
    return (t.permute(2, 0, 1) if layout == "chw" else t).contiguous()


_DTYPES = {torch.float16: api.DTYPE_F16, torch.bfloat16: api.DTYPE_BF16, torch.float32: api.DTYPE_F32}


def _per_channel(name, value, default, C):
    """mean / std as C Python floats: None -> the default, a scalar -> repeated, a sequence -> one per channel position"""
    if value is None:
        return [default] * C
    if isinstance(value, torch.Tensor):
        value = value.tolist()
    vals = [float(v) for v in value] if isinstance(value, (list, tuple)) else [float(value)] * C
    if len(vals) != C:
        raise XpngError(f"load_files: {name} has {len(vals)} values, the tensors have {C} channels")
    return vals


def _scale_bias(mean, std, C):
    """y = (v / 255 - mean) / std as y = v * scale + bias: computed in Python doubles, rounded once to fp32"""
    m, s = _per_channel("mean", mean, 0.0, C), _per_channel("std", std, 1.0, C)
    if any(x == 0 for x in s):
        raise XpngError("load_files: std must not be 0")
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).to(torch.float32).item()   # noqa: E731  (round to nearest fp32)
    return [f32(1.0 / (255.0 * x)) for x in s], [f32(-a / x) for a, x in zip(m, s)]


def _lookup(t: torch.Tensor, layout: str, dtype, dt: int, scale, bias) -> torch.Tensor:
    """an arranged uint8 tensor through api.float_table: bit for bit what the device call writes for these bytes"""
    C = t.shape[0] if layout == "chw" else t.shape[2]
    raw = api.float_table(dt, scale[:C], bias[:C])
    table = torch.frombuffer(bytearray(raw), dtype=dtype).view(C, 256)
    idx = t.to(torch.int64)
    if layout == "chw":
        return torch.stack([table[c][idx[c]] for c in range(C)], dim=0).contiguous()
    return torch.stack([table[c][idx[..., c]] for c in range(C)], dim=2).contiguous()


def random_resized_crops(dims, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """One rectangle (x, y, w, h) per image of dims = [(w, h), ...], drawn as torchvision's RandomResizedCrop.get_params draws it:
    up to ten tries of an area in `scale` times the image's and an aspect ratio log-uniform in `ratio`, the first that fits placed
    uniformly; then the centre crop of the whole image clamped to `ratio`.  A pure host function; with a seeded torch.Generator
    the list is reproducible.  What load_files(..., size=..., crops=...) takes."""
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    out = []
    for (width, height) in dims:
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise XpngError(f"random_resized_crops: bad image size {width} x {height}")
        area, rect = width * height, None
        for _ in range(10):
            target = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
            aspect = math.exp(torch.empty(1).uniform_(log_lo, log_hi, generator=generator).item())
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                y = int(torch.randint(0, height - h + 1, (1,), generator=generator).item())
                x = int(torch.randint(0, width - w + 1, (1,), generator=generator).item())
                rect = (x, y, w, h)
                break
        if rect is None:
            rect = centre_crop(width, height, ratio)
        out.append(rect)
    return out


def centre_crop(width, height, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """the fallback of random_resized_crops: the largest centred rectangle of the image whose aspect ratio lies in `ratio`"""
    in_ratio = width / height
    if in_ratio < min(ratio):
        w, h = width, min(height, max(1, int(round(width / min(ratio)))))
    elif in_ratio > max(ratio):
        w, h = min(width, max(1, int(round(height * max(ratio))))), height
    else:
        w, h = width, height
    return ((width - w) // 2, (height - h) // 2, w, h)


def _read_xpng(fn, p):
    """the bytes of a .xpng file and (level, w, h, bytes per pixel) from its 8-byte header; fn names the caller in the errors"""
    try:
        with open(p, "rb") as f:
            buf = f.read()
    except OSError as e:
        raise XpngError(f"{fn}: cannot read {os.fspath(p)!r}: {e}") from None
    if len(buf) < 8:
        raise XpngError(f"{fn}: {os.fspath(p)!r} is shorter than a header")
    h0, h1 = int.from_bytes(buf[0:4], "little"), int.from_bytes(buf[4:8], "little")
    mode, w, h, alpha = h0 >> 24, (h0 & 0xFFFFFF) + 1, (h1 & 0xFFFFFF) + 1, (h1 >> 24) & 1
    if mode not in (1, 2, 7):
        raise XpngError(f"{fn}: {os.fspath(p)!r} has level {mode}")
    return buf, (mode, w, h, 3 + alpha)


def _host_raster(fn, p, buf, head):
    """the (h, w, px) uint8 tensor of a file that is answered from its host bytes - level 7, or a whole-image single colour - or
    None for a file that needs the tile codec"""
    mode, w, h, px = head
    if mode == 7:
        if len(buf) < 8 + w * h * px:
            raise XpngError(f"{fn}: {os.fspath(p)!r} is shorter than its raster")
        return torch.frombuffer(bytearray(buf[8:8 + w * h * px]), dtype=torch.uint8).view(h, w, px)
    if len(buf) == 8 + px and buf[7] & 2:                      # whole-image single colour: the file holds one pixel
        return torch.frombuffer(bytearray(buf[8:8 + px]), dtype=torch.uint8).view(1, 1, px).expand(h, w, px)
    return None


def _pack_bodies(part):
    """the tile bodies of the files of one device call, (index, w, h, bytes) each, in one host buffer: each 16-byte aligned, 64
    readable bytes behind the last -> (buffer, offsets)"""
    offs, total = [], 0
    for (_, _, _, buf) in part:
        offs.append(total)
        total += -(-(len(buf) - 8) // 16) * 16
    host = bytearray(total + 64)
    for o, (_, _, _, buf) in zip(offs, part):
        host[o:o + len(buf) - 8] = buf[8:]
    return host, offs


def _cubic(name, interpolation, antialias):
    """True for interpolation "bicubic" (which needs antialias=True), False for "bilinear"; anything else is an error"""
    if interpolation not in ("bilinear", "bicubic"):
        raise XpngError(f"{name}: interpolation must be 'bilinear' or 'bicubic', not {interpolation!r}")
    if interpolation == "bicubic" and not antialias:
        raise XpngError(f"{name}: interpolation='bicubic' needs antialias=True: the rule is the antialiased bicubic (a = -0.5, PIL's BICUBIC); "
                        "torch's bicubic without antialias is another kernel (a = -0.75) and is not offered")
    return interpolation == "bicubic"


def load_files(paths, layout: str = "chw", channels=None, bgr: bool = False, device=None, dtype=torch.uint8, mean=None, std=None,
               stack: bool = False, size=None, crops=None, flips=None, antialias: bool = False, interpolation: str = "bilinear"):
    """The images of a list of .xpng files of any sizes as tensors on `device` (default: the current cuda device), each of
    shape (C, h, w) for layout "chw" or (h, w, C) for "hwc".  channels None keeps each file's own count (3 or 4); 3 drops the
    alpha of an RGBA file, 4 gives an RGB file alpha 255; bgr=True orders the colours B, G, R (alpha stays last).
    load_files(p, "hwc")[i] equals api.load(p[i]).  Level-7 and whole-image single-colour files are answered from the host bytes
    without a codec call, so a list of only those also loads with device="cpu"; any other list needs a GPU.  Any failure raises
    XpngError and nothing is returned.

    dtype torch.uint8 (the default) gives the file's bytes; mean or std with it is an error.  dtype torch.float16, torch.bfloat16
    or torch.float32 gives y = (v / 255 - mean[c]) / std[c], torchvision's ToTensor + Normalize: mean and std are a number or one
    number per channel position of the RETURNED tensor (with bgr=True the first belongs to blue; alpha is last), default 0 and 1.
    The conversion is done by the decode's own copy-out pass (MixedContext.decode_batch_as_float) as ONE fp32 fused multiply-add
    y = fmaf(v, scale[c], bias[c]), rounded to nearest even to the dtype, with scale[c] = float32(1 / (255 * std[c])) and
    bias[c] = float32(-mean[c] / std[c]) computed here in Python doubles and rounded once to fp32.  A caller who needs another
    affine map, or other constants bit for bit, calls decode_batch_as_float directly.  Host-answered files go through
    api.float_table, the same arithmetic on the host, so they are bit-identical to what the kernel writes.

    stack=True returns ONE tensor (N, C, h, w) or (N, h, w, C) instead of the list: every image must have the same (C, h, w) after
    `channels` is applied (XpngError names the first that differs); the device calls write straight into its slices.

    size=(OH, OW) makes every returned tensor (C, OH, OW) or (OH, OW, C): the same pass of the decode crops, resizes with plain
    2 x 2-tap bilinear interpolation (half-pixel centres as F.interpolate(mode="bilinear", align_corners=False, antialias=False);
    NOT an antialiased resize: see antialias below) and flips (MixedContext.decode_batch_resized; the rule is in include/xpng_hip.h).  It needs a float
    dtype.  crops is one rectangle (x, y, w, h) per path (random_resized_crops makes them) or None for the whole images; flips one
    bool per path (True mirrors left to right) or None.  stack=True then works for files of ANY sizes - only C must agree.
    Host-answered files go through api.resize_host and are bit-identical.  Without size the function runs exactly the path above;
    crops or flips without size is an error.

    antialias=True with size resamples every axis that SHRINKS with a triangle filter as wide as the ratio, clamped to the crop
    rectangle and renormalised, and leaves an axis that grows to the two taps above (MixedContext.decode_batch_resampled with
    FILTER_TRIANGLE_AA; the rule is in include/xpng_hip.h).  Before the normalisation this is
    F.interpolate(mode="bilinear", align_corners=False, antialias=True) of the cropped rectangle as fp32, torchvision's default for
    resize and RandomResizedCrop, up to the order of summation: the largest difference measured against torch's CPU kernel was
    1.22e-4 of one byte step (tests/test_resample.py asserts 2^-10).  Host-answered files go through api.resample_host and are
    bit-identical, so such files still load with device="cpu".  antialias=False (the default) runs today's path, call for call;
    antialias=True without size is an error.

    interpolation="bicubic" with size and antialias=True resamples with the antialiased bicubic of load_views - PIL's BICUBIC,
    F.interpolate(mode="bicubic", antialias=True) with its result clamped to 0 .. 255 - through the same device call
    (MixedContext.decode_batch_views_cubic, one view per file); host-answered files go through api.resample_cubic_host.
    "bilinear" (the default) runs the paths above, call for call."""
    if layout not in ("chw", "hwc"):
        raise XpngError(f"load_files: layout must be 'chw' or 'hwc', not {layout!r}")
    if channels not in (None, 3, 4):
        raise XpngError(f"load_files: channels must be None, 3 or 4, not {channels!r}")
    if dtype != torch.uint8 and dtype not in _DTYPES:
        raise XpngError(f"load_files: dtype must be torch.uint8, float16, bfloat16 or float32, not {dtype!r}")
    if dtype == torch.uint8 and (mean is not None or std is not None):
        raise XpngError("load_files: mean and std need a float dtype (dtype=torch.uint8 returns the file's bytes)")
    if size is None and (crops is not None or flips is not None):
        raise XpngError("load_files: crops and flips need size=(OH, OW)")
    if antialias and size is None:
        raise XpngError("load_files: antialias=True needs size=(OH, OW): without a resize there is nothing to filter")
    cubic = _cubic("load_files", interpolation, antialias)
    if cubic and size is None:
        raise XpngError("load_files: interpolation='bicubic' needs size=(OH, OW): without a resize there is nothing to interpolate")
    if size is not None:
        if dtype == torch.uint8:
            raise XpngError("load_files: size needs a float dtype (torch.float16, bfloat16 or float32): the resize interpolates")
        try:
            OH, OW = (int(v) for v in size)
        except (TypeError, ValueError):
            raise XpngError(f"load_files: size must be (OH, OW), not {size!r}") from None
        if not (1 <= OH <= 16384 and 1 <= OW <= 16384):
            raise XpngError(f"load_files: size {(OH, OW)} is outside 1 .. 16384")
    mean, std = (x.tolist() if isinstance(x, torch.Tensor) else x for x in (mean, std))
    dt = _DTYPES.get(dtype)                                        # None: the uint8 path, exactly as without the argument
    cache = {}

    def consts(C):
        """(scale, bias) of a C-channel tensor; a per-channel mean or std of another length is an error"""
        if C not in cache:
            cache[C] = _scale_bias(mean, std, C)
        return cache[C]

    if dt:
        _scale_bias(None, std, len(std) if isinstance(std, (list, tuple)) else 1)   # std == 0 is refused whatever the files hold
        if channels:
            consts(channels)
    paths = list(paths)
    if not paths:
        raise XpngError("load_files: empty list")
    if size is not None:
        crops = [None] * len(paths) if crops is None else [None if r is None else tuple(int(v) for v in r) for r in crops]
        flips = [False] * len(paths) if flips is None else [bool(f) for f in flips]
        if len(crops) != len(paths) or len(flips) != len(paths):
            raise XpngError(f"load_files: {len(paths)} paths, {len(crops)} crops and {len(flips)} flips: one of each per path")
        if any(r is not None and len(r) != 4 for r in crops):
            raise XpngError("load_files: a crop is (x, y, w, h)")
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise XpngError("load_files: no GPU is visible (device='cpu' answers level-7 and single-colour files without one)")
    heads, bufs = [], []
    for p in paths:
        buf, head = _read_xpng("load_files", p)
        heads.append(head)
        bufs.append(buf)
    if dt:
        for (_, _, _, px) in heads:
            consts(channels or px)
    def shape(C, h, w):
        if size is not None:                                           # every tensor has the output's size, whatever the file's
            h, w = OH, OW
        return (C, h, w) if layout == "chw" else (h, w, C)

    whole = None
    if stack:
        first = (channels or heads[0][3], heads[0][2], heads[0][1])
        if size is not None:
            first = (first[0], OH, OW)
        for p, (_, w, h, px) in zip(paths, heads):
            if size is not None:
                w, h = OW, OH
            if (channels or px, h, w) != first:
                raise XpngError(f"load_files: stack=True needs images of one shape, but {os.fspath(p)!r} is (C, h, w) = "
                                f"{(channels or px, h, w)} and the first is {first}")
        whole = torch.empty((len(paths),) + shape(*first), dtype=dtype, device=dev)
    out, groups = [None] * len(paths), {}
    for i, (p, buf, (mode, w, h, px)) in enumerate(zip(paths, bufs, heads)):
        t = _host_raster("load_files", p, buf, (mode, w, h, px))
        if t is None:
            groups.setdefault((mode, px), []).append((i, w, h, buf))
            continue
        if size is not None:
            C = channels or px
            word = api.layout(planar=layout == "chw", bgr=bgr, channels=C)
            if cubic:
                raw = api.resample_cubic_host(t.numpy(), (OH, OW), word, dt, *consts(C), rect=crops[i], flip=flips[i])
            elif antialias:
                raw = api.resample_host(t.numpy(), (OH, OW), word, dt, *consts(C), rect=crops[i], flip=flips[i], filter=api.FILTER_TRIANGLE_AA)
            else:
                raw = api.resize_host(t.numpy(), (OH, OW), word, dt, *consts(C), rect=crops[i], flip=flips[i])
            t = torch.frombuffer(bytearray(raw), dtype=dtype).view(shape(C, h, w))
        else:
            t = _arrange(t, layout, channels, bgr)
            if dt:
                t = _lookup(t, layout, dtype, dt, *consts(channels or px))
        if whole is not None:
            whole[i].copy_(t)
        else:
            out[i] = t.to(dev)
    if groups and dev.type != "cuda":
        raise XpngError("load_files: these files need the tile codec, which runs on a GPU only (there is no CPU fallback)")
    for (mode, px), members in sorted(groups.items()):
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        C = channels or px
        word = api.layout(planar=layout == "chw", bgr=bgr, channels=C)
        starts = api.batch_cuts([(w, h) for (_, w, h, _) in members], [px] * len(members), BATCH_MAX, BATCH_BYTES) + [len(members)]
        for a, b in zip(starts, starts[1:]):
            part = members[a:b]
            host, offs = _pack_bodies(part)                       # the tile bodies of the call in one upload
            with torch.cuda.device(index):
                d_in = torch.frombuffer(host, dtype=torch.uint8).to(dev)
                if whole is not None:                             # (the kernels take any pointers: the slices are the buffers)
                    outs = [whole[i] for (i, _, _, _) in part]
                else:
                    outs = [torch.empty(shape(C, h, w), dtype=dtype, device=dev) for (_, w, h, _) in part]
                torch.cuda.current_stream().synchronize()          # the upload is there before the context's stream reads it
                ctx = api.MixedContext([(w, h) for (_, w, h, _) in part], px, device=index)
                try:
                    ins, lens = [d_in.data_ptr() + o for o in offs], [len(buf) - 8 for (_, _, _, buf) in part]
                    if cubic:                                    # (the views call with the identity view_image: one view per file)
                        ctx.decode_batch_views_cubic(mode, ins, lens, None, [t.data_ptr() for t in outs], word, dt, (OH, OW), *consts(C),
                                                     rects=[crops[i] or (0, 0, w, h) for (i, w, h, _) in part], flips=[flips[i] for (i, _, _, _) in part])
                    elif size is not None and antialias:
                        ctx.decode_batch_resampled(mode, ins, lens, [t.data_ptr() for t in outs], word, dt, (OH, OW), *consts(C),
                                                   rects=[crops[i] or (0, 0, w, h) for (i, w, h, _) in part], flips=[flips[i] for (i, _, _, _) in part],
                                                   filter=api.FILTER_TRIANGLE_AA)
                    elif size is not None:
                        ctx.decode_batch_resized(mode, ins, lens, [t.data_ptr() for t in outs], word, dt, (OH, OW), *consts(C),
                                                 rects=[crops[i] or (0, 0, w, h) for (i, w, h, _) in part], flips=[flips[i] for (i, _, _, _) in part])
                    elif dt:
                        ctx.decode_batch_as_float(mode, ins, lens, [t.data_ptr() for t in outs], word, dt, *consts(C))
                    else:
                        ctx.decode_batch_as(mode, ins, lens, [t.data_ptr() for t in outs], word)
                    status = ctx.decode_status()                  # (synchronises the context's stream: the tensors are complete)
                finally:
                    ctx.close()
            if status != 0:
                raise XpngError("load_files: a tile of a level-%d file was rejected or the device call failed (status %d)" % (mode, status))
            for (i, _, _, _), t in zip(part, outs):
                out[i] = t
    return whole if whole is not None else out


def load_views(paths, views, size, layout: str = "chw", channels=None, bgr: bool = False, device=None, dtype=torch.float16, mean=None,
               std=None, antialias: bool = True, stack: bool = False, out=None, colour=None, interpolation: str = "bilinear", blur=None,
               solarise=None, affine=None, fill=None, tone=None):
    """Any number of views per file, each decoded once: views is a list of (path_index, rect_or_None, flip) - rect = (x, y, w, h)
    inside file path_index, None for the whole image; flip True mirrors left to right - and view v comes back as a tensor
    (C, OH_v, OW_v) for layout "chw" or (OH_v, OW_v, C) for "hwc", in view order.  size is one (OH, OW) for every view or one pair
    per view.  layout, channels, bgr, device, mean and std are load_files'; dtype must be a float dtype (the resize interpolates).
    antialias=True (the default, torchvision's) resamples a shrinking axis with the triangle filter of load_files(antialias=True);
    False gives plain bilinear taps.  View v equals, bit for bit, api.resample_host of api.load(paths[path_index]).

    The files that reach the tile codec are grouped and cut into device calls as load_files does, and every call is ONE
    MixedContext.decode_batch_views: each file is entropy-decoded once however many views read it, and only the tiles that some
    view of the file touches are decoded at all.  A path that no view names is not read.  Level-7 and single-colour files go
    through api.resample_host per view, so a list of only those also works with device="cpu".

    stack=True returns ONE tensor (V, C, OH, OW) or (V, OH, OW, C): it needs one size and one C.  out is a list of preallocated
    tensors, one per view, written in place and returned: each must have the view's shape, `dtype`, the device and be contiguous
    (slices along the first dimension of a stacked tensor are) - this is how a multi-crop caller fills its two stacked tensors of
    different sizes from one call.  Any failure raises XpngError.

    colour is None or one entry per view, each None (the identity matrix) or a colour matrix - 12 numbers or a (3, 4) array as
    colour_matrix, compose_colour and random_colour_jitter return them: row k the output colour k of R, G, B whatever bgr says,
    columns the inputs R, G, B and a constant in byte units.  The copy-out pass of the decode puts every pixel of the view through
    its matrix and a clamp to 0 .. 255 before the normalisation, so a colour jitter and a grayscale per view cost no further pass
    (the rule is in include/xpng_hip.h; alpha does not pass through the matrix).  View v then equals, bit for bit,
    api.resample_colour_host with its matrix, which is also what answers level-7 and single-colour files.  Without colour, or
    with every entry None, the function runs exactly the calls it runs without the argument; beside a matrix a None entry is the
    identity matrix, whose clamp can differ from no matrix in the last bits where the antialiased quotient rounds past 255.

    interpolation="bicubic" resamples every view with the ANTIALIASED BICUBIC that DINO, BYOL, MAE and timm's ViT recipes use:
    Keys' cubic with a = -0.5 on both axes, stretched by the ratio where an axis shrinks, clamped to the view's rectangle and
    renormalised, and every resampled value clamped to 0 .. 255 before the matrix and the normalisation - PIL's BICUBIC, and
    F.interpolate(mode="bicubic", align_corners=False, antialias=True) of the cropped rectangle followed by that clamp, up to the
    order of summation (tests/test_cubic.py states the measured difference).  It needs antialias=True: torch's bicubic without
    antialias is another kernel (a = -0.75) with another border rule, and is not offered.  Every device call is then ONE
    MixedContext.decode_batch_views_cubic and view v equals, bit for bit, api.resample_cubic_host with its matrix, which also
    answers level-7 and single-colour files; here an identity matrix and no matrix give the same bits.  "bilinear" (the
    default) runs exactly the calls the function ran without the argument.

    blur and solarise are the two augmentations of SimCLR, BYOL and DINO that are not linear per pixel; both sit between the colour
    matrix and the normalisation.  blur is None or one entry per view, each None or (sigma, kernel_size) with kernel_size odd, 3 ..
    63 and below twice the view's smaller side: a Gaussian blur of kernel_size taps per axis over a reflected border, on the colour
    channels (alpha is not blurred), clamped to 0 .. 255 - torchvision's GaussianBlur on tensors up to the order of summation
    (tests/test_views_blur.py states the measured difference), not PIL's ImageFilter.GaussianBlur, which is a box-blur
    approximation.  solarise is None or one entry per view, each None or a threshold in 0 .. 255: a colour value b at or above it
    becomes 255 - b (torchvision's solarize in byte units).  random_gaussian_blur and random_solarise draw such lists.  With either
    list given - with both interpolations - every device call is ONE MixedContext.decode_batch_views_blur: views that ask for
    neither are written as before, the others take a second kernel over fp32 planes in the context's workspace; view v equals,
    bit for bit, api.resample_blur_host, which also answers level-7 and single-colour files.  With both None the function runs
    exactly the calls it ran without the arguments.

    affine gives views a rotation, a shear, a scale and a translation - RandomRotation, RandomAffine, the geometric operations of
    RandAugment - in the same pass.  It is None or one entry per view, each None or an inverse 2 x 3 matrix from the view's output
    coordinates to source coordinates of its whole image, as affine_matrix and random_affine return them.  A view that has a matrix
    must have rect None and flip False - the matrix carries both; a None entry takes affine_matrix(rect or the whole image, size,
    flip=flip).  The call needs antialias=False and interpolation "bilinear" (four taps, torchvision's affine() on tensors) or
    "nearest" (for label maps; accepted only here).  What a tap finds outside the image is fill: None (zeros), a number, or R, G,
    B, A in byte units, one for the call.  Every device call is then ONE MixedContext.decode_batch_views_affine, which decodes only
    the tiles that a view's warped footprint touches, and view v equals, bit for bit, api.resample_affine_host with its matrix,
    which also answers level-7 and single-colour files.  blur= or solarise= together with affine= is an error.  With affine None
    the function runs exactly the calls it ran without the argument.

    tone gives views the tone operations of AutoAugment, RandAugment and TrivialAugment, in any order.  It is None or one entry per
    view, each None or a sequence of up to four steps executed in order: "autocontrast", "equalise", ("posterise", bits) with bits
    an integer 0 .. 8, ("solarise", threshold) with a threshold in 0 .. 255, and "invert" (the rule is in include/xpng_hip.h; on
    whole byte values equalise, posterise, solarise and invert are PIL's ImageOps, autocontrast is torchvision's on a float tensor).
    The steps run on the three colour planes of the finished view - behind the resampling, the colour matrix, the blur and the
    solarise= list, which stays the blur record's - and before the normalisation; autocontrast and equalise take their statistics
    over the whole view, fill pixels of a warp included.  tone= works with every interpolation, with colour=, blur= and solarise=,
    and with affine=.  Every device call is then ONE MixedContext.decode_batch_views_tone, or with affine= ONE
    decode_batch_views_affine_tone, and view v equals, bit for bit, api.resample_tone_host or api.resample_affine_tone_host, which
    also answer level-7 and single-colour files.  random_tone draws such lists.  With tone None the function runs exactly the
    calls it ran without the argument."""
    if layout not in ("chw", "hwc"):
        raise XpngError(f"load_views: layout must be 'chw' or 'hwc', not {layout!r}")
    if channels not in (None, 3, 4):
        raise XpngError(f"load_views: channels must be None, 3 or 4, not {channels!r}")
    if dtype not in _DTYPES:
        raise XpngError(f"load_views: dtype must be torch.float16, bfloat16 or float32, not {dtype!r}: the resize interpolates")
    if stack and out is not None:
        raise XpngError("load_views: stack=True allocates the result, out= is the caller's: give one of them")
    dt = _DTYPES[dtype]
    mean, std = (x.tolist() if isinstance(x, torch.Tensor) else x for x in (mean, std))
    paths = list(paths)
    try:
        views = [(int(i), None if r is None else tuple(int(v) for v in r), bool(f)) for (i, r, f) in views]
    except (TypeError, ValueError):
        raise XpngError("load_views: a view is (path_index, (x, y, w, h) or None, flip)") from None
    V = len(views)
    if not V:
        raise XpngError("load_views: empty list of views")
    for v, (i, r, _) in enumerate(views):
        if not 0 <= i < len(paths):
            raise XpngError(f"load_views: view {v} names path {i}, the list has {len(paths)}")
        if r is not None and len(r) != 4:
            raise XpngError(f"load_views: the rectangle of view {v} is {r!r}, not (x, y, w, h)")
    try:
        sizes = list(size)
        if len(sizes) == 2 and not hasattr(sizes[0], "__len__"):
            sizes = [sizes] * V
        sizes = [tuple(int(x) for x in s) for s in sizes]
        if any(len(s) != 2 for s in sizes):
            raise ValueError
    except (TypeError, ValueError):
        raise XpngError(f"load_views: size must be (OH, OW) or one (OH, OW) per view, not {size!r}") from None
    if len(sizes) != V:
        raise XpngError(f"load_views: {len(sizes)} sizes for {V} views: one (OH, OW), or one per view")
    for v, (oh, ow) in enumerate(sizes):
        if not (1 <= oh <= 16384 and 1 <= ow <= 16384):
            raise XpngError(f"load_views: size {(oh, ow)} of view {v} is outside 1 .. 16384")
    cols = [None] * V
    if colour is not None:
        cols = list(colour)
        if len(cols) != V:
            raise XpngError(f"load_views: colour has {len(cols)} entries for {V} views: one matrix (or None) per view")
        cols = [None if m is None else api._colour12(f"load_views: colour[{v}]", m) for v, m in enumerate(cols)]
        if any(m is not None for m in cols):                           # beside a matrix, None is the identity MATRIX: every view is clamped
            cols = [list(api.COLOUR_IDENTITY) if m is None else m for m in cols]
    blurs = None
    if blur is not None or solarise is not None:
        bl, so = ([None] * V if x is None else list(x) for x in (blur, solarise))
        for name, x in (("blur", bl), ("solarise", so)):
            if len(x) != V:
                raise XpngError(f"load_views: {name} has {len(x)} entries for {V} views: one entry (or None) per view")
        blurs = []
        for v, (b, t) in enumerate(zip(bl, so)):
            sigma, radius = 0.0, 0
            if b is not None:
                try:
                    sigma, ks = float(b[0]), int(b[1])
                    if len(b) != 2 or ks != b[1]:
                        raise ValueError
                except (TypeError, ValueError, IndexError):
                    raise XpngError(f"load_views: blur[{v}] is {b!r}, not None or (sigma, kernel_size)") from None
                if ks < 3 or ks > 63 or ks % 2 == 0:
                    raise XpngError(f"load_views: the kernel_size of blur[{v}] is {ks}: it must be odd and 3 .. 63")
                radius = ks // 2
            if t is not None:
                try:
                    t = float(t)
                except (TypeError, ValueError):
                    raise XpngError(f"load_views: solarise[{v}] is {t!r}, not None or a threshold in 0 .. 255") from None
                if not 0.0 <= t <= 255.0:
                    raise XpngError(f"load_views: solarise[{v}] is {t!r}, not None or a threshold in 0 .. 255")
            blurs.append(None if b is None and t is None else (sigma, radius, t))
    tones = None
    if tone is not None:
        tones = list(tone)
        if len(tones) != V:
            raise XpngError(f"load_views: tone has {len(tones)} entries for {V} views: one list of steps (or None) per view")
        tones = [_tone_steps(f"load_views: tone[{v}]", t) for v, t in enumerate(tones)]
    mats, afilt = None, api.FILTER_BILINEAR
    if affine is not None:
        mats = list(affine)
        if len(mats) != V:
            raise XpngError(f"load_views: affine has {len(mats)} entries for {V} views: one matrix (or None) per view")
        if antialias or interpolation not in ("bilinear", "nearest"):
            raise XpngError("load_views: affine= needs antialias=False and interpolation 'bilinear' or 'nearest': a warp is sampled with four taps "
                            f"or one, not {interpolation!r} with antialias={antialias!r}")
        if blurs is not None:
            raise XpngError("load_views: blur= or solarise= together with affine= is not offered")
        for v, m in enumerate(mats):
            if m is not None and (views[v][1] is not None or views[v][2]):
                raise XpngError(f"load_views: view {v} has a matrix, so its rectangle must be None and its flip False: the matrix carries both")
        mats = [None if m is None else api._affine6(f"load_views: affine[{v}]", m) for v, m in enumerate(mats)]
        fill = api._fill4("load_views", fill)
        fill = None if fill is None else list(fill)
        afilt = api.FILTER_NEAREST if interpolation == "nearest" else api.FILTER_BILINEAR
        interpolation = "bilinear"
    elif interpolation == "nearest":
        raise XpngError("load_views: interpolation='nearest' is offered with affine= only")
    elif fill is not None:
        raise XpngError("load_views: fill= is the value outside an affine view: it needs affine=")
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise XpngError("load_views: no GPU is visible (device='cpu' answers level-7 and single-colour files without one)")
    cubic = _cubic("load_views", interpolation, antialias)
    filt = api.FILTER_TRIANGLE_AA if antialias else api.FILTER_BILINEAR
    # only the files that a view names are read
    heads, bufs = {}, {}
    for i in sorted({i for (i, _, _) in views}):
        bufs[i], heads[i] = _read_xpng("load_views", paths[i])
    for v, (i, r, _) in enumerate(views):
        _, w, h, _ = heads[i]
        if r is not None and not (r[2] > 0 and r[3] > 0 and 0 <= r[0] <= w - r[2] and 0 <= r[1] <= h - r[3]):
            raise XpngError(f"load_views: the rectangle {r} of view {v} is empty or leaves the {w} x {h} image {os.fspath(paths[i])!r}")
    if mats is not None:                                               # a view without a matrix: its crop, its resize and its flip as one
        mats = [m if m is not None else affine_matrix(views[v][1] or (0, 0, heads[views[v][0]][1], heads[views[v][0]][2]), sizes[v], flip=views[v][2]).reshape(6).tolist()
                for v, m in enumerate(mats)]
        # what the library would refuse of a matrix or of the fill is refused here, before any view is written
        for v, m in enumerate(mats):
            try:
                api.affine_footprint(heads[views[v][0]][1:3], m, sizes[v])
            except XpngError as e:
                raise XpngError(f"load_views: view {v}: {e}") from None
        for k, x in enumerate(fill or ()):
            if not 0.0 <= x <= 255.0:                                  # (NaN included)
                raise XpngError(f"load_views: bad fill: entry {k} is {x!r} (R, G, B, A in byte units: each must be finite and lie in 0 .. 255)")
    chans = [channels or heads[i][3] for (i, _, _) in views]
    cache = {}
    for C in set(chans):
        cache[C] = _scale_bias(mean, std, C)

    def shape(v):
        (oh, ow), C = sizes[v], chans[v]
        return (C, oh, ow) if layout == "chw" else (oh, ow, C)

    whole = None
    if stack:
        for v in range(V):
            if shape(v) != shape(0):
                raise XpngError(f"load_views: stack=True needs one size and one channel count, but view {v} is {shape(v)} and view 0 is {shape(0)}")
        whole = torch.empty((V,) + shape(0), dtype=dtype, device=dev)
        res = list(whole.unbind(0))
    elif out is not None:
        res = list(out)
        if len(res) != V:
            raise XpngError(f"load_views: out has {len(res)} tensors for {V} views")
        for v, t in enumerate(res):
            if not isinstance(t, torch.Tensor):
                raise XpngError(f"load_views: out[{v}] is not a tensor")
            if tuple(t.shape) != shape(v):
                raise XpngError(f"load_views: out[{v}] has shape {tuple(t.shape)}, view {v} is {shape(v)}")
            if t.dtype != dtype:
                raise XpngError(f"load_views: out[{v}] has dtype {t.dtype}, not {dtype}")
            if t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index):
                raise XpngError(f"load_views: out[{v}] is on {t.device}, not on {dev}")
            if not t.is_contiguous():
                raise XpngError(f"load_views: out[{v}] is not contiguous")
    else:
        res = [None] * V
    groups = {}
    for i, (mode, w, h, px) in heads.items():
        t = _host_raster("load_views", paths[i], bufs[i], (mode, w, h, px))
        if t is None:
            groups.setdefault((mode, px), []).append((i, w, h, bufs[i]))
            continue
        ras = t.contiguous().numpy()
        for v, (vi, r, f) in enumerate(views):
            if vi != i:
                continue
            word = api.layout(planar=layout == "chw", bgr=bgr, channels=chans[v])
            if tones is not None and mats is not None:
                raw = api.resample_affine_tone_host(ras, sizes[v], mats[v], word, dt, *cache[chans[v]], filter=afilt, fill=fill, colour=cols[v],
                                                    tone=tones[v])
            elif tones is not None:
                raw = api.resample_tone_host(ras, sizes[v], word, dt, *cache[chans[v]], rect=r, flip=f, filter=api.FILTER_CUBIC_AA if cubic else filt,
                                             colour=cols[v], blur=None if blurs is None else blurs[v], tone=tones[v])
            elif mats is not None:
                raw = api.resample_affine_host(ras, sizes[v], mats[v], word, dt, *cache[chans[v]], filter=afilt, fill=fill, colour=cols[v])
            elif blurs is not None:
                raw = api.resample_blur_host(ras, sizes[v], word, dt, *cache[chans[v]], rect=r, flip=f, filter=api.FILTER_CUBIC_AA if cubic else filt,
                                             colour=cols[v], blur=blurs[v])
            elif cubic:
                raw = api.resample_cubic_host(ras, sizes[v], word, dt, *cache[chans[v]], rect=r, flip=f, colour=cols[v])
            else:
                raw = api.resample_colour_host(ras, sizes[v], word, dt, *cache[chans[v]], rect=r, flip=f, filter=filt, colour=cols[v])
            tv = torch.frombuffer(bytearray(raw), dtype=dtype).view(shape(v))
            if res[v] is None:
                res[v] = tv.to(dev)
            else:
                res[v].copy_(tv)
    if groups and dev.type != "cuda":
        raise XpngError("load_views: these files need the tile codec, which runs on a GPU only (there is no CPU fallback)")
    for (mode, px), members in sorted(groups.items()):
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        C = channels or px
        word = api.layout(planar=layout == "chw", bgr=bgr, channels=C)
        starts = api.batch_cuts([(w, h) for (_, w, h, _) in members], [px] * len(members), BATCH_MAX, BATCH_BYTES) + [len(members)]
        for a, b in zip(starts, starts[1:]):
            part = members[a:b]
            local = {i: k for k, (i, _, _, _) in enumerate(part)}
            mine = [v for v, (i, _, _) in enumerate(views) if i in local]
            host, offs = _pack_bodies(part)                       # the tile bodies of the call in one upload
            with torch.cuda.device(index):
                d_in = torch.frombuffer(host, dtype=torch.uint8).to(dev)
                for v in mine:
                    if res[v] is None:
                        res[v] = torch.empty(shape(v), dtype=dtype, device=dev)
                torch.cuda.current_stream().synchronize()          # the upload is there before the context's stream reads it
                ctx = api.MixedContext([(w, h) for (_, w, h, _) in part], px, device=index)
                try:
                    ins, lens = [d_in.data_ptr() + o for o in offs], [len(buf) - 8 for (_, _, _, buf) in part]
                    args = (mode, ins, lens, [local[views[v][0]] for v in mine], [res[v].data_ptr() for v in mine], word, dt,
                            [sizes[v] for v in mine], *cache[C])
                    kw = dict(rects=[views[v][1] or (0, 0, heads[views[v][0]][1], heads[views[v][0]][2]) for v in mine],
                              flips=[views[v][2] for v in mine],
                              colours=[cols[v] for v in mine] if cols[mine[0]] is not None else None)
                    if tones is not None and mats is not None:
                        ctx.decode_batch_views_affine_tone(*args[:8], [mats[v] for v in mine], *cache[C], filter=afilt, fill=fill, colours=kw["colours"],
                                                           tones=[tones[v] for v in mine])
                    elif tones is not None:
                        ctx.decode_batch_views_tone(*args, filter=api.FILTER_CUBIC_AA if cubic else filt,
                                                    blurs=None if blurs is None else [blurs[v] for v in mine], tones=[tones[v] for v in mine], **kw)
                    elif mats is not None:
                        ctx.decode_batch_views_affine(*args[:8], [mats[v] for v in mine], *cache[C], filter=afilt, fill=fill, colours=kw["colours"])
                    elif blurs is not None:
                        ctx.decode_batch_views_blur(*args, filter=api.FILTER_CUBIC_AA if cubic else filt, blurs=[blurs[v] for v in mine], **kw)
                    elif cubic:
                        ctx.decode_batch_views_cubic(*args, **kw)
                    else:
                        ctx.decode_batch_views(*args, filter=filt, **kw)
                    status = ctx.decode_status()                  # (synchronises the context's stream: the tensors are complete)
                finally:
                    ctx.close()
            if status != 0:
                raise XpngError("load_views: a tile of a level-%d file was rejected or the device call failed (status %d)" % (mode, status))
    return whole if whole is not None else res


_LUMA = (0.299, 0.587, 0.114)


def _colour64(brightness, contrast, saturation, hue):
    """colour_matrix in float64, before the one rounding"""
    b, c, s, h = float(brightness), float(contrast), float(saturation), float(hue)
    M = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    M = b * M
    M = c * M
    M[:, 3] += (1.0 - c) * 127.5
    S = s * np.eye(3) + (1.0 - s) * np.ones((3, 1)) * np.array([_LUMA])
    M = S @ M
    co, si = (1.0, 0.0) if h == 0.0 else (math.cos(2.0 * math.pi * h), math.sin(2.0 * math.pi * h))
    K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    R = co * np.eye(3) + (1.0 - co) / 3.0 * np.ones((3, 3)) + si / math.sqrt(3.0) * K
    return R @ M


def _compose64(a, b):
    a, b = (np.asarray(api._colour12("compose_colour", m), dtype=np.float64).reshape(3, 4) for m in (a, b))
    out = b[:, :3] @ a
    out[:, 3] += b[:, 3]
    return out


def colour_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0):
    """The (3, 4) float32 colour matrix of a brightness, a contrast, a saturation and a hue step, as load_views(colour=...) and
    MixedContext.decode_batch_views(colours=...) take it: row k the output colour k of R, G, B, columns the inputs R, G, B and a
    constant, in byte units (0 .. 255).  Composed in float64 in this fixed order, each step left-multiplied onto the 3 x 4 with
    its constant column, then rounded once to fp32:
      brightness b   b * M
      contrast c     about the fixed centre 127.5: c * M, constant += (1 - c) * 127.5
      saturation s   S = s * I + (1 - s) * 1 * [0.299, 0.587, 0.114]: 0 is the luma in every colour, 1 the identity
      hue h          a fraction of a turn: the rotation by 2 pi h about the gray axis,
                     cos * I + (1 - cos) / 3 * J + sin / sqrt(3) * K with J all ones and K = [[0, -1, 1], [1, 0, -1], [-1, 1, 0]]
    All ones and hue 0 give exactly the identity.  This is NOT torchvision's ColorJitter value for value: there the contrast
    blends with the image's own mean gray level and not with a fixed centre, the hue shift goes through HSV and not through a
    rotation in RGB, every step clamps to the value range before the next one, and the order of the four steps is drawn at random.
    Here the steps are linear and fixed, so that a whole jitter is ONE matrix and one clamp at its end.  The call itself takes any
    matrix: a caller who wants another order or another step composes it with compose_colour."""
    return _colour64(brightness, contrast, saturation, hue).astype(np.float32)


def compose_colour(a, b):
    """The (3, 4) float32 matrix that applies colour matrix b AFTER colour matrix a (without a's clamp in between): b's 3 x 3 times
    a, plus b's constant column; computed in float64, rounded once."""
    return _compose64(a, b).astype(np.float32)


def random_colour_jitter(n, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, gray_p=0.2, generator=None):
    """n colour matrices, one per view, drawn as SimCLR's and BYOL's colour augmentation draws its parameters: with probability p a
    jitter colour_matrix(b, c, s, h) with b uniform in [max(0, 1 - brightness), 1 + brightness], c and s alike and h uniform in
    [-hue, hue]; with probability gray_p a grayscale (saturation 0) on top of it; otherwise the identity.  A pure host function;
    with a seeded torch.Generator the list is reproducible.  What load_views(..., colour=...) takes."""
    n = int(n)
    if n < 0:
        raise XpngError(f"random_colour_jitter: n is {n}")
    for name, x in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        if not 0.0 <= float(x) <= 16.0:
            raise XpngError(f"random_colour_jitter: {name} must be within 0 .. 16, not {x!r}")
    if not 0.0 <= float(hue) <= 0.5:
        raise XpngError(f"random_colour_jitter: hue must be within 0 .. 0.5, not {hue!r}")
    u = torch.rand((n, 6), dtype=torch.float64, generator=generator).tolist()   # one draw whatever the outcomes: entry k depends on row k alone

    def span(x, r):
        lo, hi = max(0.0, 1.0 - float(r)), 1.0 + float(r)
        return lo + (hi - lo) * x

    out = []
    for (jit, ub, uc, us, uh, gray) in u:
        M = _colour64(1.0, 1.0, 1.0, 0.0)
        if jit < p:
            M = _colour64(span(ub, brightness), span(uc, contrast), span(us, saturation), (2.0 * uh - 1.0) * float(hue))
        if gray < gray_p:
            M = _compose64(M, _colour64(1.0, 1.0, 0.0, 0.0))
        out.append(M.astype(np.float32))
    return out


def random_gaussian_blur(n, kernel_size=23, sigma=(0.1, 2.0), p=0.5, generator=None):
    """n entries for load_views(blur=...), one per view, drawn as SimCLR's, BYOL's and DINO's GaussianBlur draws its parameter: with
    probability p the pair (sigma, kernel_size) with sigma uniform in [sigma[0], sigma[1]], otherwise None.  kernel_size is odd and
    3 .. 63 (23 is BYOL's and DINO's for 224 x 224; SimCLR takes a tenth of the side, made odd); a multi-crop caller draws one
    list per view size with its own kernel_size and p (DINO: p = 1.0 and 0.1 for the two global views, 0.5 for the local ones).
    A pure host function; with a seeded torch.Generator the list is reproducible."""
    n, ks = int(n), int(kernel_size)
    if n < 0:
        raise XpngError(f"random_gaussian_blur: n is {n}")
    if ks != kernel_size or ks < 3 or ks > 63 or ks % 2 == 0:
        raise XpngError(f"random_gaussian_blur: kernel_size must be odd and 3 .. 63, not {kernel_size!r}")
    try:
        lo, hi = (float(x) for x in sigma)
    except (TypeError, ValueError):
        raise XpngError(f"random_gaussian_blur: sigma must be (low, high), not {sigma!r}") from None
    if not 2.0 ** -10 <= lo <= hi <= 1024.0:
        raise XpngError(f"random_gaussian_blur: sigma must satisfy 2^-10 <= low <= high <= 1024, not {sigma!r}")
    if not 0.0 <= float(p) <= 1.0:
        raise XpngError(f"random_gaussian_blur: p must be within 0 .. 1, not {p!r}")
    u = torch.rand((n, 2), dtype=torch.float64, generator=generator).tolist()   # one draw whatever the outcomes: entry k depends on row k alone
    return [(lo + (hi - lo) * us, ks) if coin < p else None for (coin, us) in u]


def random_solarise(n, threshold=128, p=0.2, generator=None):
    """n entries for load_views(solarise=...), one per view: with probability p the threshold (0 .. 255, in byte units; 128 is
    BYOL's and DINO's), otherwise None.  A pure host function; with a seeded torch.Generator the list is reproducible."""
    n = int(n)
    if n < 0:
        raise XpngError(f"random_solarise: n is {n}")
    if not 0.0 <= float(threshold) <= 255.0:
        raise XpngError(f"random_solarise: threshold must be within 0 .. 255, not {threshold!r}")
    if not 0.0 <= float(p) <= 1.0:
        raise XpngError(f"random_solarise: p must be within 0 .. 1, not {p!r}")
    u = torch.rand((n,), dtype=torch.float64, generator=generator).tolist()
    return [float(threshold) if coin < p else None for coin in u]


_TONE_OPS = {"autocontrast": api.TONE_AUTOCONTRAST, "equalise": api.TONE_EQUALISE, "posterise": api.TONE_POSTERISE,
             "solarise": api.TONE_SOLARISE, "invert": api.TONE_INVERT}


def _tone_steps(name, entry):
    """one entry of load_views(tone=...) - None or up to four steps - as the list of (op, arg) pairs of api.resample_tone_host, checked"""
    if entry is None:
        return None
    if isinstance(entry, str):
        raise XpngError(f"{name} is {entry!r}: an entry is None or a sequence of steps, not one step")
    try:
        steps = list(entry)
    except TypeError:
        raise XpngError(f"{name} is {entry!r}, not None or a sequence of up to four steps") from None
    if len(steps) > 4:
        raise XpngError(f"{name} has {len(steps)} steps: at most four")
    out = []
    for k, st in enumerate(steps):
        op, arg = (st, None) if isinstance(st, str) else (tuple(st) + (None, None))[:2] if hasattr(st, "__len__") and 1 <= len(st) <= 2 else (None, None)
        if op not in _TONE_OPS:
            raise XpngError(f"{name}, step {k} is {st!r}: a step is 'autocontrast', 'equalise', ('posterise', bits), ('solarise', threshold) or 'invert'")
        if op in ("posterise", "solarise"):
            try:
                arg = float(arg)
            except (TypeError, ValueError):
                raise XpngError(f"{name}, step {k}: {op!r} needs a number, as ({op!r}, value), not {st!r}") from None
            if op == "posterise" and not (0.0 <= arg <= 8.0 and arg == int(arg)):
                raise XpngError(f"{name}, step {k}: posterise bits are {arg!r}, not an integer in 0 .. 8")
            if op == "solarise" and not 0.0 <= arg <= 255.0:
                raise XpngError(f"{name}, step {k}: the solarise threshold is {arg!r}, not within 0 .. 255")
        elif arg is not None:
            raise XpngError(f"{name}, step {k}: {op!r} takes no argument, not {st!r}")
        out.append((_TONE_OPS[op], 0.0 if arg is None else arg))
    return out or None


def random_tone(n, num_ops=2, ops=("autocontrast", "equalise", "posterise", "solarise"), magnitude=9, num_magnitude_bins=31, p=1.0,
                generator=None):
    """n entries for load_views(tone=...), one per view, drawn as RandAugment draws its operations: num_ops steps (0 .. 4), each
    uniform out of `ops` (names out of "autocontrast", "equalise", "posterise", "solarise", "invert") and kept with probability p.
    The magnitude is RandAugment's table: posterise keeps 8 - round(magnitude * 4 / (num_magnitude_bins - 1)) bits, solarise takes
    the threshold 255 * (1 - magnitude / (num_magnitude_bins - 1)).  A pure host function: one torch.rand draw of shape
    (n, num_ops, 2), so entry k depends on row k alone; with a seeded torch.Generator the list is reproducible."""
    n, num_ops, bins = int(n), int(num_ops), int(num_magnitude_bins)
    if n < 0:
        raise XpngError(f"random_tone: n is {n}")
    if not 0 <= num_ops <= 4:
        raise XpngError(f"random_tone: num_ops must be 0 .. 4, not {num_ops!r}")
    ops = list(ops)
    if not ops or any(o not in _TONE_OPS for o in ops):
        raise XpngError(f"random_tone: ops must be names out of {sorted(_TONE_OPS)}, not {ops!r}")
    if bins < 2 or not 0 <= float(magnitude) <= bins - 1:
        raise XpngError(f"random_tone: magnitude must be within 0 .. num_magnitude_bins - 1 = {bins - 1}, not {magnitude!r}")
    if not 0.0 <= float(p) <= 1.0:
        raise XpngError(f"random_tone: p must be within 0 .. 1, not {p!r}")
    bits = 8 - int(round(float(magnitude) * 4.0 / (bins - 1)))
    thr = 255.0 * (1.0 - float(magnitude) / (bins - 1))
    u = torch.rand((n, num_ops, 2), dtype=torch.float64, generator=generator).tolist()   # one draw whatever the outcomes
    out = []
    for row in u:
        steps = []
        for (pick, coin) in row:
            op = ops[min(int(pick * len(ops)), len(ops) - 1)]
            if coin < p:
                steps.append((op, bits) if op == "posterise" else (op, thr) if op == "solarise" else op)
        out.append(steps or None)
    return out


def _size_pair(name, size):
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise XpngError(f"{name}: size must be (OH, OW), not {size!r}") from None
    if not (1 <= oh <= 16384 and 1 <= ow <= 16384):
        raise XpngError(f"{name}: size {(oh, ow)} is outside 1 .. 16384")
    return oh, ow


def affine_matrix(rect, size, angle=0.0, translate=(0, 0), scale=1.0, shear=(0.0, 0.0), flip=False):
    """The (2, 3) float32 INVERSE matrix of a view, as load_views(affine=...) and MixedContext.decode_batch_views_affine take it:
    from continuous output coordinates (x to the right, y down, pixel (j, i) centred at (j + 0.5, i + 0.5)) to continuous source
    coordinates of the whole image.  The view shows rect = (x, y, w, h) of the image resized to size = (OH, OW) - mirrored left to
    right first where flip is true - and then rotated, sheared, scaled and translated about the OUTPUT's centre, with the
    parameter meanings of torchvision's RandomAffine / F.affine: angle in degrees, clockwise; translate = (tx, ty) in output pixels;
    scale > 0; shear = (sx, sy) in degrees (a number is (sx, 0)).

    Composed in float64 and rounded once.  The order, from an output pixel back to the source:
      1. P = (X - OW / 2, Y - OH / 2)                               coordinates about the output's centre
      2. P' = A^-1 P, A^-1 = (R(angle) Sh(shear) S(scale))^-1 (P - translate)  torchvision's _get_inverse_affine_matrix with centre 0
      3. Q = P' + (OW / 2, OH / 2)                                  back into the frame of the resized rectangle
      4. sx = x + Qx * w / OW  (flip: x + w - Qx * w / OW),  sy = y + Qy * h / OH     the crop and the resize
    All defaults give exactly the crop-resize matrix [[w / OW, 0, x], [0, h / OH, y]], and an angle that is a multiple of 90 without
    shear takes cos and sin as exactly 0 and +-1, so a quarter turn of a square view of its own size is exact on the bits.  Where this differs from torchvision: there
    the image is cropped and resized (RandomResizedCrop) in a pass of its own, which interpolates once more and cuts the corners
    that the rotation then turns into the frame to `fill`; here step 4 is part of the one map, so a rotated view shows the source
    pixels around its rectangle where the image has them, and `fill` only outside the image.  The flip comes before the warp."""
    oh, ow = _size_pair("affine_matrix", size)
    try:
        x, y, w, h = (float(v) for v in rect)
        tx, ty = (float(v) for v in translate)
        shx, shy = (float(shear), 0.0) if not hasattr(shear, "__len__") else (float(v) for v in shear)
        rot, sc = math.radians(float(angle)), float(scale)
    except (TypeError, ValueError):
        raise XpngError(f"affine_matrix: rect is (x, y, w, h), translate (tx, ty), shear a number or (sx, sy); got {rect!r}, {translate!r}, {shear!r}") from None
    if not (w > 0 and h > 0 and sc > 0.0 and math.isfinite(sc)):
        raise XpngError(f"affine_matrix: the rectangle must not be empty and scale must be positive, not {rect!r}, {scale!r}")
    shx, shy = math.radians(shx), math.radians(shy)
    a = math.cos(rot - shy) / math.cos(shy)
    b = -math.cos(rot - shy) * math.tan(shx) / math.cos(shy) - math.sin(rot)
    c = math.sin(rot - shy) / math.cos(shy)
    d = -math.sin(rot - shy) * math.tan(shx) / math.cos(shy) + math.cos(rot)
    inv = np.array([[d / sc, -b / sc, 0.0], [-c / sc, a / sc, 0.0], [0.0, 0.0, 1.0]])
    if shx == 0.0 and shy == 0.0 and float(angle) % 90.0 == 0.0:      # whole quarter turns exactly: cos and sin are 0 and +-1, not 6e-17
        co, si = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(float(angle) // 90.0) % 4]
        inv = np.array([[co / sc, si / sc, 0.0], [-si / sc, co / sc, 0.0], [0.0, 0.0, 1.0]]) + 0.0   # (+ 0.0: no -0.0)
    move = lambda px, py: np.array([[1.0, 0.0, px], [0.0, 1.0, py], [0.0, 0.0, 1.0]])
    crop = np.array([[-w / ow if flip else w / ow, 0.0, x + w if flip else x], [0.0, h / oh, y], [0.0, 0.0, 1.0]])
    M = crop @ move(ow / 2.0, oh / 2.0) @ inv @ move(-tx, -ty) @ move(-ow / 2.0, -oh / 2.0)
    return M[:2].astype(np.float32)


def random_affine(n, rects, size, degrees, translate=None, scale=None, shear=None, generator=None):
    """n matrices for load_views(affine=...), one per view, with parameters drawn as torchvision's RandomAffine.get_params draws
    them: the angle uniform in degrees = (lo, hi) (a number d is (-d, d)); with translate = (a, b), tx and ty uniform in
    +-a * OW and +-b * OH, rounded to whole output pixels; with scale = (lo, hi) the scale uniform in it; with shear = (lo, hi) or
    (xlo, xhi, ylo, yhi) (a number s is (-s, s)) the shears uniform in them.  rects is one (x, y, w, h) per view - what
    random_resized_crops returns, or the whole images - and size one (OH, OW) for every view or one pair per view; view k is
    affine_matrix(rects[k], size_k, angle, (tx, ty), scale, (sx, sy)).  A pure host function; with a seeded torch.Generator the list
    is reproducible."""
    n = int(n)
    rects = list(rects)
    if n < 0 or len(rects) != n:
        raise XpngError(f"random_affine: n is {n} and rects has {len(rects)} entries")
    sizes = list(size)
    if len(sizes) == 2 and not hasattr(sizes[0], "__len__"):
        sizes = [sizes] * n
    if len(sizes) != n:
        raise XpngError(f"random_affine: {len(sizes)} sizes for {n} views: one (OH, OW), or one per view")

    def span(name, x, k):
        if x is None:
            return None
        try:
            v = [-float(x), float(x)] if not hasattr(x, "__len__") else [float(t) for t in x]
        except (TypeError, ValueError):
            v = []
        if len(v) not in k or any(lo > hi for lo, hi in zip(v[::2], v[1::2])):
            raise XpngError(f"random_affine: {name} must be a number or (low, high) with low <= high, not {x!r}")
        return v

    deg, sc, sh = span("degrees", degrees, (2,)), span("scale", scale, (2,)), span("shear", shear, (2, 4))
    if deg is None:
        raise XpngError("random_affine: degrees is required (0 for no rotation)")
    if sc is not None and not sc[0] > 0.0:
        raise XpngError(f"random_affine: scale must be positive, not {scale!r}")
    if translate is not None:
        try:
            ta, tb = (float(t) for t in translate)
        except (TypeError, ValueError):
            ta = -1.0
        if not (0.0 <= ta <= 1.0 and 0.0 <= tb <= 1.0):
            raise XpngError(f"random_affine: translate must be two fractions within 0 .. 1, not {translate!r}")
    u = torch.rand((n, 6), dtype=torch.float64, generator=generator).tolist()   # one draw whatever the outcomes: entry k depends on row k alone
    out = []
    for k, (ua, ux, uy, us, uhx, uhy) in enumerate(u):
        oh, ow = _size_pair("random_affine", sizes[k])
        angle = deg[0] + (deg[1] - deg[0]) * ua
        tx = ty = 0
        if translate is not None:
            tx, ty = int(round((2.0 * ux - 1.0) * ta * ow)), int(round((2.0 * uy - 1.0) * tb * oh))
        s = 1.0 if sc is None else sc[0] + (sc[1] - sc[0]) * us
        shx = 0.0 if sh is None else sh[0] + (sh[1] - sh[0]) * uhx
        shy = 0.0 if sh is None or len(sh) == 2 else sh[2] + (sh[3] - sh[2]) * uhy
        out.append(affine_matrix(rects[k], (oh, ow), angle, (tx, ty), s, (shx, shy)))
    return out


def _inverse_scale_bias(mean, std, present):
    """load_files' y = (v / 255 - mean) / std inverted: v = y * (255 std) + 255 mean, as four (scale, bias) values computed in
    Python doubles and rounded once to fp32.  `present` = the channel counts among the tensors: a per-channel mean or std must have
    exactly that many values, so it cannot serve a list that mixes 3 and 4 channels."""
    def four(name, value, default):
        if value is None:
            return [default] * 4
        if isinstance(value, torch.Tensor):
            value = value.tolist()
        if not isinstance(value, (list, tuple)):
            return [float(value)] * 4
        vals = [float(v) for v in value]
        for C in sorted(present):
            if len(vals) != C:
                raise XpngError(f"store_files: {name} has {len(vals)} values, a tensor has {C} channels")
        return vals + [default] * (4 - len(vals))
    m, s = four("mean", mean, 0.0), four("std", std, 1.0)
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).to(torch.float32).item()   # noqa: E731  (round to nearest fp32)
    return [f32(255.0 * x) for x in s], [f32(255.0 * x) for x in m]


def store_files(tensors, paths, level: int = 1, layout: str = "chw", bgr: bool = False, mean=None, std=None):
    """Writes one .xpng file per tensor at `level` (1, 2 or 7): the inverse of load_files.  `tensors` is a list of tensors of any
    sizes, each (C, h, w) for layout "chw" or (h, w, C) for "hwc" with C = 3 or 4 per tensor, or one stacked (N, ...) tensor; all
    on ONE cuda device, contiguous, of ONE dtype among torch.uint8, float16, bfloat16 and float32.  bgr=True reads the colours as
    B, G, R (alpha stays last).  Anything else raises XpngError naming the first offender; nothing is ever copied or converted
    silently, and no file is written unless all can be.

    A uint8 tensor holds the bytes to store; mean or std with it is an error.  A float tensor holds what load_files returns for the
    same mean and std, y = (v / 255 - mean[c]) / std[c], and is stored as v = fmaf(y, scale[c], bias[c]) rounded half to even and
    clamped to 0 .. 255 (NaN gives 0), with scale[c] = float32(255 * std[c]) and bias[c] = float32(255 * mean[c]) computed here in
    Python doubles and rounded once; mean and std are a number or one number per channel position of the tensors, default 0 and 1
    (a model that writes 0 .. 1 needs neither).  The rule is written down in include/xpng_hip.h (xpnghip_images_begin_device).

    The pixels stay on the device: one staging kernel, queued behind the current torch stream, quantises and rearranges every
    tensor of the list into a staged batch, and file i is byte for byte what api.store(level, raster_i, paths[i]) writes for the
    quantised (h, w, C) raster - normalisation of RGBA, the single colour of level 2 and the raw fallbacks included
    (api.store_tensors, include/xpng_store_tensors.h).  When the call returns the tensors are free again.

    CPU tensors are accepted with level=7 only: they are quantised by api.quantize_host, the same arithmetic on the host, and
    written through api.store_batch, which needs no device at that level."""
    if layout not in ("chw", "hwc"):
        raise XpngError(f"store_files: layout must be 'chw' or 'hwc', not {layout!r}")
    if level not in (1, 2, 7):
        raise XpngError(f"store_files: level must be 1, 2 or 7, not {level!r}")
    if isinstance(tensors, torch.Tensor):
        if tensors.dim() != 4:
            raise XpngError(f"store_files: a stacked tensor is (N, ...) with four dimensions, not {tuple(tensors.shape)}")
        if not tensors.is_contiguous():
            raise XpngError("store_files: the stacked tensor is not contiguous")
        tensors = list(tensors.unbind(0))
    else:
        tensors = list(tensors)
    paths = [os.fspath(p) for p in paths]
    if len(tensors) != len(paths):
        raise XpngError(f"store_files: {len(tensors)} tensors and {len(paths)} paths")
    if not tensors:
        raise XpngError("store_files: empty list")
    first = tensors[0]
    dims, chans = [], []
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise XpngError(f"store_files: tensor {i} is not a tensor of three dimensions")
        if t.dtype != torch.uint8 and t.dtype not in _DTYPES:
            raise XpngError(f"store_files: tensor {i} has dtype {t.dtype}; torch.uint8, float16, bfloat16 or float32 are stored")
        if t.dtype != first.dtype:
            raise XpngError(f"store_files: tensor {i} has dtype {t.dtype}, the first has {first.dtype}: one dtype per call")
        if t.device != first.device:
            raise XpngError(f"store_files: tensor {i} is on {t.device}, the first on {first.device}: one device per call")
        if not t.is_contiguous():
            raise XpngError(f"store_files: tensor {i} is not contiguous (call .contiguous() yourself: nothing is copied silently)")
        C, h, w = (t.shape[0], t.shape[1], t.shape[2]) if layout == "chw" else (t.shape[2], t.shape[0], t.shape[1])
        if C not in (3, 4):
            raise XpngError(f"store_files: tensor {i} has {C} channels in layout {layout!r}, not 3 or 4")
        if not (1 <= w <= 1 << 24 and 1 <= h <= 1 << 24):
            raise XpngError(f"store_files: tensor {i} is {w} x {h}; each side must be 1 .. 16777216")
        dims.append((w, h))
        chans.append(C)
    dt = _DTYPES.get(first.dtype, 0)
    if not dt and (mean is not None or std is not None):
        raise XpngError("store_files: mean and std need a float dtype (a torch.uint8 tensor holds the bytes to store)")
    scale = bias = None
    if dt:
        scale, bias = _inverse_scale_bias(mean, std, set(chans))
        if not all(math.isfinite(v) for v in scale + bias):
            raise XpngError("store_files: mean and std must be finite")
    word = api.layout(planar=layout == "chw", bgr=bgr)
    if first.device.type == "cpu":
        if level != 7:
            raise XpngError("store_files: CPU tensors are stored at level 7 only; levels 1 and 2 run on a GPU (there is no CPU fallback)")
        rasters = [api.quantize_host(t.data_ptr(), w * h, C, word, dt, scale, bias).reshape(h, w, C) for t, (w, h), C in zip(tensors, dims, chans)]
        api.store_batch(7, rasters, paths)
        return
    if first.device.type != "cuda":
        raise XpngError(f"store_files: tensors on {first.device} cannot be stored (cuda, or cpu with level=7)")
    index = first.device.index if first.device.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(index).cuda_stream      # the staging kernel runs behind whatever produced the tensors there
    api.store_tensors(level, [t.data_ptr() for t in tensors], dims, chans, word, dt, paths, scale, bias, device=index, stream=stream)
