"""CPU: the cut rule of the batched level-1 form (xpng_amd/csrc/top_class_cut.hpp) compiled into a stand-alone program with g++.

The rule says how many of a launch's biggest tiles get a wavefront of their own for the alpha chain: the tiles as large as the
largest, when there are at most 128 / B of them, when other tiles remain and when the launch then models at least a tenth shorter
(a wavefront with one stream steps 3 : 2 against one with 32).

1. The table of the rule, row for row, with the pixel counts taken from xpng_amd.shard.tile_table:
       4096^2    B = 64, 128   all tiles   k = 1   (one tile of 295 936, 16 of 241 536, 64 of 197 136)
       16384^2   B = 4         all tiles   k = 0   (1225 equal largest tiles: more than the budget)
       888^2     any B         all tiles   k = 0   (4 equal tiles)
       988^2     B <= 64       all tiles   k = 1   (295 936 / 241 536 x 2 / 197 136)
       988^2     B <= 64       tiles 1..3  k = 2   (two equal top tiles)
2. 200 000 random size-sorted inputs: k * B <= 128, k < T, k = 0 when all tiles are equal, a cut takes exactly the top class and
   models a gain of at least a tenth."""
import _kit as K

from xpng_amd.shard import tile_table


def _sorted_sizes(W, H, t0=0, t1=None):
    sizes = [w * h for (_, _, w, h) in tile_table(W, H)][t0:t1]
    return sorted(sizes, reverse=True)


def test_cut_rule_table_and_bounds_on_the_host(tmp_path):
    big = _sorted_sizes(4096, 4096)
    assert (big.count(295936), big.count(241536), big.count(197136), len(big)) == (1, 16, 64, 81)
    huge = _sorted_sizes(16384, 16384)
    assert huge.count(huge[0]) == 1225
    assert _sorted_sizes(888, 888) == [197136] * 4
    assert _sorted_sizes(988, 988) == [295936, 241536, 241536, 197136]
    assert _sorted_sizes(988, 988, 1, 4) == [241536, 241536, 197136]
    rows = [("4096^2 all", 64, 1, big), ("4096^2 all", 128, 1, big), ("16384^2 all", 4, 0, huge)]
    rows += [("888^2 all", B, 0, _sorted_sizes(888, 888)) for B in (1, 2, 3, 32, 64, 128, 200)]
    rows += [("988^2 all", B, 1, _sorted_sizes(988, 988)) for B in (1, 2, 3, 32, 64)]
    rows += [("988^2 tiles (1, 4)", B, 2, _sorted_sizes(988, 988, 1, 4)) for B in (1, 2, 3, 32, 64)]
    cases = "".join('{"%s", %d, %d, {%s}},\n' % (name, B, k, ", ".join(map(str, n))) for name, B, k, n in rows)
    header = K.cut("top_class_cut.hpp", "#pragma once", "}  // namespace xpng") + "}\n"
    assert "hip" not in header and "asm" not in header
    r = K.run_kernels_on_host(tmp_path, "top_class_cut_host", {"CUT_TEXT": header, "CASES_TEXT": cases},
                              sanitize=("-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"), timeout=120)
    print(r.stdout)
    assert "table rows: %d" % len(rows) in r.stdout
    assert "cases: 200000" in r.stdout and int(r.stdout.split("cases: 200000 (")[1].split()[0]) > 1000
