#!/usr/bin/env python3
"""Pin the level-2 colour catalogue of tests/_m2_colour.py to the GENUINE reference (oracle/_ref/xpng, compiled by oracle/Makefile).

  python oracle/make_m2_colour_golden.py

Writes tests/golden/m2_colour.json: name -> {w, h, seven_md5 (the raster as a .7 file), L2: {size, md5} of the file the reference
wrote at level 2}.  Only the table is committed; the rasters come out of the generator again, and tests/test_m2_colour_streams.py
checks that the generator and the oracle still agree with it.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _m2_colour as mc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from xpng_amd.synth import to_seven_bytes  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    assert po.have_ref(), "make -C oracle ref first"
    rasters = {name: np.ascontiguousarray(mc.raster(name)) for name in mc.names()}
    rasters["gray_cluster"] = mc.gray_cluster_raster()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for name, r in rasters.items():
            h, w, _ = r.shape
            seven = to_seven_bytes(r)
            data, _ = po.ref_encode(2, seven, td)
            back, _ = po.ref_decode(data, td)
            assert back == seven, name                                       # the reference round-trips its own file
            out[name] = {"w": w, "h": h, "seven_md5": md5(seven), "L2": {"size": len(data), "md5": md5(data)}}
            print(name, len(data), flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "m2_colour.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("entries:", len(out))


if __name__ == "__main__":
    main()
