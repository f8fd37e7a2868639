#!/usr/bin/env python3
"""Pin the steered rasters of tests/_steered.py to the GENUINE reference (oracle/_ref/xpng, compiled by oracle/Makefile).

  python oracle/make_steered_golden.py

Writes tests/golden/steered.json: name -> {w, h, ch, seven_md5 (the raster as a .7 file), L1 / L2: {size, md5} of the file the
reference wrote at that level}.  Only the table is committed; the rasters come out of the generator again, and
tests/test_steered.py checks that the generator and the oracle still agree with it.
"""
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _steered as S  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from xpng_amd.synth import to_seven_bytes  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    assert po.have_ref(), "make -C oracle ref first"
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for name in S.named():
            r = S.raster(name)
            h, w, ch = r.shape
            seven = to_seven_bytes(r)
            ent = {"w": w, "h": h, "ch": ch, "seven_md5": md5(seven)}
            for level in (1, 2):
                data, _ = po.ref_encode(level, seven, td)
                back, _ = po.ref_decode(data, td)
                assert back == to_seven_bytes(po.normalize_rgba(r)), (name, level)   # the reference round-trips its own file
                ent[f"L{level}"] = {"size": len(data), "md5": md5(data)}
            out[name] = ent
            print(name, ent["L1"]["size"], ent["L2"]["size"], flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "steered.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("entries:", len(out))


if __name__ == "__main__":
    main()
