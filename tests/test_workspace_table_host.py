"""CPU: the workspace table of a context (xpng_amd/csrc/common.hpp WsTable) run on the host.

Its text is cut out of common.hpp and compiled into tests/workspace_table_host.cpp, a stand-alone program that supplies hipMalloc and
hipFree on top of malloc and free, with a switch that makes the n-th allocation fail, built with a statically linked
AddressSanitizer where the toolchain has one.  It checks that a second get on a filled slot allocates nothing and leaves the total
alone, that drop subtracts exactly what get added and nulls the member, that a group of four whose third allocation fails keeps two
filled slots and the sum of their sizes and is completed - exactly the missing two - by the next call, that free_all frees every
live block exactly once and leaves every member null and the total at 0, and that drop of a null member is harmless."""
import _kit as K


def test_workspace_table_on_the_host(tmp_path):
    text = K.cut("common.hpp", "// ---- workspace table")
    assert "struct WsTable" in text and "__device__" not in text and text.count("hipMalloc(") == 1 and text.count("hipFree(") == 2
    r = K.run_kernels_on_host(tmp_path, "workspace_table_host", {"TABLE_TEXT": text})
    assert "mallocs 7, frees 7" in r.stdout
