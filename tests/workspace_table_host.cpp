// Host run of the workspace table (xpng_amd/csrc/common.hpp WsTable): its text, cut out of the header by the test, on top of an
// allocator of this file's own - hipMalloc / hipFree as malloc / free that keep the set of live blocks, count their calls and can be
// told to fail the n-th allocation from now.  AddressSanitizer sees a block freed twice or never; the set of live blocks says the same
// without it.
// Built and run by tests/test_workspace_table_host.py: g++ -fsanitize=address -static-libasan -DTABLE_TEXT=\"...\".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
static std::set<void *> g_live;
static long g_mallocs = 0, g_frees = 0, g_fail_in = 0, g_errors = 0;  // g_fail_in = n > 0: the n-th allocation from now fails
static void bad(const char *what, long a = 0, long b = 0) { printf("FAIL %s (%ld, %ld)\n", what, a, b); g_errors++; }
#define CHECK(cond) do { if (!(cond)) bad(#cond, __LINE__); } while (0)
static hipError_t hipMalloc(void **p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) return hipErrorOutOfMemory;  // (like the runtime: *p is left as it was)
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    g_mallocs++;
    return hipSuccess;
}
static hipError_t hipFree(void *p) {
    if (!g_live.erase(p)) bad("hipFree of a block that is not live");
    else free(p);
    g_frees++;
    return hipSuccess;
}

#include TABLE_TEXT  // struct WsTable, cut out of xpng_amd/csrc/common.hpp by the test

// pointer members of different types, as a context has them
struct Holder { uint8_t *a = nullptr; uint32_t *b = nullptr; uint64_t *c = nullptr; uint16_t *d = nullptr; const uint8_t **e = nullptr; };
static const uint64_t SZ[4] = {1000, 24, 4096, 7};
static hipError_t group(WsTable &t, Holder &h) {  // a lazy group: four tables, the first failure ends it
    hipError_t e;
    if ((e = t.get((void **)&h.a, SZ[0])) || (e = t.get((void **)&h.b, SZ[1])) || (e = t.get((void **)&h.c, SZ[2])) || (e = t.get((void **)&h.d, SZ[3]))) return e;
    return hipSuccess;
}

int main() {
    {   // get on a filled slot; drop; drop of a null member
        WsTable t;
        Holder h;
        CHECK(t.get((void **)&h.a, 100) == hipSuccess && h.a && t.total == 100 && g_mallocs == 1);
        uint8_t *first = h.a;
        h.a[99] = 1;
        CHECK(t.get((void **)&h.a, 5000) == hipSuccess && h.a == first && t.total == 100 && g_mallocs == 1);  // nothing allocated, the total left alone
        CHECK(t.get((void **)&h.e, 64) == hipSuccess && t.total == 164);
        t.drop((void **)&h.a);
        CHECK(!h.a && t.total == 64 && g_frees == 1 && t.live.size() == 1);  // exactly what get added
        t.drop((void **)&h.a);                                               // a null member: harmless
        t.drop((void **)&h.b);                                               // ... one that never held anything too
        CHECK(t.total == 64 && g_frees == 1 && t.live.size() == 1 && h.e);
        CHECK(t.get((void **)&h.a, 300) == hipSuccess && h.a && t.total == 364);  // a grow path: drop, then get
        h.a[299] = 1;
        t.free_all();
        CHECK(!h.a && !h.e && t.total == 0 && t.live.empty() && g_live.empty() && g_frees == 3 && g_mallocs == 3);
        t.free_all();                                                        // nothing recorded: nothing freed
        CHECK(g_frees == 3);
    }
    {   // a group whose third allocation fails, repeated with the failure switched off
        WsTable t;
        Holder h;
        const long m0 = g_mallocs, f0 = g_frees;
        g_fail_in = 3;
        CHECK(group(t, h) == hipErrorOutOfMemory);
        CHECK(h.a && h.b && !h.c && !h.d && t.total == SZ[0] + SZ[1] && g_mallocs == m0 + 2 && t.live.size() == 2);
        uint8_t *a = h.a;
        uint32_t *b = h.b;
        CHECK(group(t, h) == hipSuccess);
        CHECK(h.a == a && h.b == b && h.c && h.d && g_mallocs == m0 + 4);  // exactly the missing two
        CHECK(t.total == SZ[0] + SZ[1] + SZ[2] + SZ[3] && t.live.size() == 4 && g_live.size() == 4);
        h.c[SZ[2] / 8 - 1] = 1;
        CHECK(group(t, h) == hipSuccess && g_mallocs == m0 + 4);           // complete: a further call allocates nothing
        t.drop((void **)&h.b);                                             // one from the middle, then the rest at once
        CHECK(!h.b && t.total == SZ[0] + SZ[2] + SZ[3] && g_frees == f0 + 1);
        t.free_all();
        CHECK(!h.a && !h.b && !h.c && !h.d && t.total == 0 && t.live.empty() && g_live.empty());
        CHECK(g_frees == f0 + 4 && g_mallocs - g_frees == 0);              // every live block freed exactly once
    }
    {   // a failure leaves the slot null and the table as it was
        WsTable t;
        Holder h;
        g_fail_in = 1;
        CHECK(t.get((void **)&h.c, 8) == hipErrorOutOfMemory && !h.c && t.total == 0 && t.live.empty());
        t.free_all();
    }
    CHECK(g_live.empty());
    printf("mallocs %ld, frees %ld\nerrors: %ld\n", g_mallocs, g_frees, g_errors);
    return g_errors ? 1 : 0;
}
