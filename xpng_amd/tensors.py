"""torch front end: .xpng files -> uint8 device tensors in the layout a model reads, the pixels never leaving HBM.

`load_files` is what `api.load_batch` is for host arrays.  The files that reach the tile codec are grouped by (tile mode, bytes per
pixel) and every group is decoded by mixed-size device calls straight into tensors of the final layout
(MixedContext.decode_batch_as: the layout is written by the copy-out pass of the decode, include/xpng_hip.h XPNGHIP_LAYOUT_*).
api.py stays free of torch; this module is the only one of the package that imports it at load time."""
from __future__ import annotations

import os

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


def load_files(paths, layout: str = "chw", channels=None, bgr: bool = False, device=None) -> list:
    """The images of a list of .xpng files of any sizes as uint8 tensors on `device` (default: the current cuda device), each of
    shape (C, h, w) for layout "chw" or (h, w, C) for "hwc".  channels None keeps each file's own count (3 or 4); 3 drops the
    alpha of an RGBA file, 4 gives an RGB file alpha 255; bgr=True orders the colours B, G, R (alpha stays last).
    load_files(p, "hwc")[i] equals api.load(p[i]).  Level-7 and whole-image single-colour files are answered from the host bytes
    without a codec call, so a list of only those also loads with device="cpu"; any other list needs a GPU.  Any failure raises
    XpngError and nothing is returned."""
    if layout not in ("chw", "hwc"):
        raise XpngError(f"load_files: layout must be 'chw' or 'hwc', not {layout!r}")
    if channels not in (None, 3, 4):
        raise XpngError(f"load_files: channels must be None, 3 or 4, not {channels!r}")
    paths = list(paths)
    if not paths:
        raise XpngError("load_files: empty list")
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise XpngError("load_files: no GPU is visible (device='cpu' answers level-7 and single-colour files without one)")
    out, groups = [None] * len(paths), {}
    for i, p in enumerate(paths):
        try:
            with open(p, "rb") as f:
                buf = f.read()
        except OSError as e:
            raise XpngError(f"load_files: cannot read {os.fspath(p)!r}: {e}") from None
        if len(buf) < 8:
            raise XpngError(f"load_files: {os.fspath(p)!r} is shorter than a header")
        h0, h1 = int.from_bytes(buf[0:4], "little"), int.from_bytes(buf[4:8], "little")
        mode, w, h, alpha = h0 >> 24, (h0 & 0xFFFFFF) + 1, (h1 & 0xFFFFFF) + 1, (h1 >> 24) & 1
        px = 3 + alpha
        if mode not in (1, 2, 7):
            raise XpngError(f"load_files: {os.fspath(p)!r} has level {mode}")
        if mode == 7:
            if len(buf) < 8 + w * h * px:
                raise XpngError(f"load_files: {os.fspath(p)!r} is shorter than its raster")
            t = torch.frombuffer(bytearray(buf[8:8 + w * h * px]), dtype=torch.uint8).view(h, w, px)
            out[i] = _arrange(t, layout, channels, bgr).to(dev)
        elif len(buf) == 11 + alpha and buf[7] & 2:              # whole-image single colour: the file holds one pixel
            t = torch.frombuffer(bytearray(buf[8:8 + px]), dtype=torch.uint8).view(1, 1, px).expand(h, w, px)
            out[i] = _arrange(t, layout, channels, bgr).to(dev)
        else:
            groups.setdefault((mode, px), []).append((i, w, h, buf))
    if groups and dev.type != "cuda":
        raise XpngError("load_files: these files need the tile codec, which runs on a GPU only (there is no CPU fallback)")
    for (mode, px), members in sorted(groups.items()):
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        C = channels or px
        word = api.layout(planar=layout == "chw", bgr=bgr, channels=C)
        starts = api.batch_cuts([(w, h) for (_, w, h, _) in members], [px] * len(members), BATCH_MAX, BATCH_BYTES) + [len(members)]
        for a, b in zip(starts, starts[1:]):
            part = members[a:b]
            # the tile bodies of the call in one upload: each 16-byte aligned, 64 readable bytes behind the last
            offs, total = [], 0
            for (_, _, _, buf) in part:
                offs.append(total)
                total += -(-(len(buf) - 8) // 16) * 16
            host = bytearray(total + 64)
            for o, (_, _, _, buf) in zip(offs, part):
                host[o:o + len(buf) - 8] = buf[8:]
            with torch.cuda.device(index):
                d_in = torch.frombuffer(host, dtype=torch.uint8).to(dev)
                outs = [torch.empty((C, h, w) if layout == "chw" else (h, w, C), dtype=torch.uint8, device=dev) for (_, w, h, _) in part]
                torch.cuda.current_stream().synchronize()          # the upload is there before the context's stream reads it
                ctx = api.MixedContext([(w, h) for (_, w, h, _) in part], px, device=index)
                try:
                    ctx.decode_batch_as(mode, [d_in.data_ptr() + o for o in offs], [len(buf) - 8 for (_, _, _, buf) in part],
                                        [t.data_ptr() for t in outs], word)
                    status = ctx.decode_status()                  # (synchronises the context's stream: the tensors are complete)
                finally:
                    ctx.close()
            if status != 0:
                raise XpngError("load_files: a tile of a level-%d file was rejected or the device call failed (status %d)" % (mode, status))
            for (i, _, _, _), t in zip(part, outs):
                out[i] = t
    return out
