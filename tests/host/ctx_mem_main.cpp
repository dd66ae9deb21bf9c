// ctx_mem_main.cpp — csrc/ctx_mem.cpp against the stubbed allocation calls (hip_stub.cpp).  usage: ctx_mem_test <case>;
// exit status 0 when every check of the case held.  The stub's books are the assertion: what is live, of which kind, and
// how many calls were made.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../bsc-nav_amd/csrc/ctx_mem.h"
#include "hip_stub.h"

static char g_err[512] = "";
void bsc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static long live() { return stub_live(STUB_DEVICE) + stub_live(STUB_PINNED); }

static void case_alloc_free_grow()
{
    BscMem *m = mem_create();
    CHECK(m);
    void *a = nullptr, *z = nullptr;
    CHECK(mem_alloc(m, &a, 100, "a") == BSC_OK && stub_is_live(a, STUB_DEVICE));
    memset(a, 1, 100);
    CHECK(mem_alloc(m, &z, 0, "zero bytes") == BSC_OK && stub_is_live(z, STUB_DEVICE));   // the stub aborts on a 0-byte request
    void *was = a;
    mem_free(m, &a);
    CHECK(a == nullptr && !stub_is_live(was, STUB_DEVICE) && live() == 1);
    void *g = nullptr;
    int64_t cap = 0;
    long calls = stub_calls();
    CHECK(mem_grow(m, &g, &cap, 0, false, "g") == BSC_OK && g == nullptr && cap == 0 && stub_calls() == calls);   // 0 >= 0: nothing
    CHECK(mem_grow(m, &g, &cap, 64, false, "g") == BSC_OK && cap == 64 && stub_is_live(g, STUB_DEVICE));
    memset(g, 2, 64);                                             // exactly 64 bytes: the sanitizer sees one more
    void *g0 = g;
    calls = stub_calls();
    CHECK(mem_grow(m, &g, &cap, 64, false, "g") == BSC_OK && mem_grow(m, &g, &cap, 10, false, "g") == BSC_OK);
    CHECK(g == g0 && cap == 64 && stub_calls() == calls);         // the fast path makes no call
    CHECK(mem_grow(m, &g, &cap, 65, false, "g") == BSC_OK && cap == 65 && !stub_is_live(g0, STUB_DEVICE) && stub_is_live(g, STUB_DEVICE));
    CHECK(stub_calls() == calls + 2 && live() == 2);              // one free, one allocation
    void *hp = nullptr;
    int64_t hcap = 0;
    CHECK(mem_grow(m, &hp, &hcap, 32, true, "hp") == BSC_OK && stub_is_live(hp, STUB_PINNED) && stub_last_flags() == hipHostMallocDefault);
    CHECK(mem_grow(m, &hp, &hcap, 48, true, "hp") == BSC_OK && hcap == 48 && stub_live(STUB_PINNED) == 1);
    mem_release_all(m);
    CHECK(live() == 0);
}

static void case_pinned_flags()
{
    BscMem *m = mem_create();
    void *p = nullptr, *q = nullptr;
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;
    CHECK(mem_alloc_pinned(m, &p, 152, flags, "mailbox") == BSC_OK && stub_is_live(p, STUB_PINNED) && stub_last_flags() == flags);
    CHECK(mem_alloc_pinned(m, &q, 8, hipHostMallocDefault, "q") == BSC_OK && stub_last_flags() == hipHostMallocDefault);
    CHECK(stub_live(STUB_PINNED) == 2 && stub_live(STUB_DEVICE) == 0);
    mem_free(m, &p);                                              // through hipHostFree, or the stub aborts
    CHECK(p == nullptr && stub_live(STUB_PINNED) == 1);
    mem_release_all(m);
    CHECK(live() == 0);
}

static void case_free_null_and_released()
{
    BscMem *m = mem_create();
    void *p = nullptr;
    const long calls = stub_calls();
    mem_free(m, &p);
    CHECK(p == nullptr && stub_calls() == calls);
    CHECK(mem_alloc(m, &p, 8, "p") == BSC_OK);
    mem_free(m, &p);
    const long after = stub_calls();
    mem_free(m, &p);                                              // released: the slot is null, nothing is freed twice
    CHECK(p == nullptr && stub_calls() == after && live() == 0);
    mem_release_all(m);
    mem_release_all(nullptr);
    CHECK(live() == 0);
}

static void case_mark_release_to()
{
    BscMem *m = mem_create();
    void *keep[3] = {}, *tmp[4] = {};
    CHECK(mem_alloc(m, &keep[0], 8, "k0") == BSC_OK && mem_alloc_pinned(m, &keep[1], 8, 0, "k1") == BSC_OK);
    const uint64_t mark = mem_mark(m);
    mem_release_to(m, mark);                                      // nothing since the mark
    CHECK(live() == 2);
    CHECK(mem_alloc(m, &tmp[0], 8, "t0") == BSC_OK && mem_alloc_pinned(m, &tmp[1], 8, 0, "t1") == BSC_OK);
    mem_free(m, &keep[0]);                                        // an older entry leaves in between: the mark still holds
    CHECK(mem_alloc(m, &tmp[2], 8, "t2") == BSC_OK);
    mem_free(m, &tmp[0]);                                         // a newer one released early is not released again
    const uint64_t inner = mem_mark(m);
    CHECK(mem_alloc(m, &tmp[3], 8, "t3") == BSC_OK);
    mem_release_to(m, inner);
    CHECK(!stub_is_live(tmp[3], STUB_DEVICE) && stub_is_live(tmp[2], STUB_DEVICE) && stub_is_live(tmp[1], STUB_PINNED));
    mem_release_to(m, mark);
    CHECK(live() == 1 && stub_is_live(keep[1], STUB_PINNED));
    CHECK(mem_alloc(m, &keep[2], 8, "k2") == BSC_OK);             // the ledger goes on working
    mem_release_all(m);
    CHECK(live() == 0);
}

// N mixed allocations (device, pinned, grown), the k-th failing, for every k: the failed slot is null, the earlier ones are
// intact, the later ones succeed, and nothing is left after mem_release_all.  More than 256 so that the ledger itself grows.
static void case_fail_each()
{
    const int N = 300;
    for (int k = 0; k < N; ++k) {
        BscMem *m = mem_create();
        static void *slot[N];
        static int64_t cap[N];
        memset(slot, 0, sizeof slot);
        memset(cap, 0, sizeof cap);
        stub_fail_in(k);
        g_err[0] = 0;
        for (int i = 0; i < N; ++i) {
            const size_t bytes = 16 + 8 * (size_t)i;
            bsc_status st;
            if (i % 3 == 0) st = mem_alloc(m, &slot[i], bytes, "dev");
            else if (i % 3 == 1) st = mem_alloc_pinned(m, &slot[i], bytes, hipHostMallocDefault, "pin");
            else st = mem_grow(m, &slot[i], &cap[i], (int64_t)bytes, i % 2 == 0, "grown");
            if (i == k) {
                CHECK(st == BSC_E_HIP && slot[i] == nullptr && cap[i] == 0);
                CHECK(strstr(g_err, i % 3 == 0 ? "dev" : (i % 3 == 1 ? "pin" : "grown")) && strstr(g_err, "bytes"));
            } else {
                CHECK(st == BSC_OK && slot[i] != nullptr);
                memset(slot[i], 0x5a, bytes);
            }
        }
        for (int i = 0; i < N; ++i) {
            if (i == k) continue;
            const bool pinned = i % 3 == 1 || (i % 3 == 2 && i % 2 == 0);
            CHECK(stub_is_live(slot[i], pinned ? STUB_PINNED : STUB_DEVICE));
            CHECK(((unsigned char *)slot[i])[0] == 0x5a && ((unsigned char *)slot[i])[16 + 8 * i - 1] == 0x5a);
        }
        CHECK(live() == N - 1);
        mem_release_all(m);
        CHECK(live() == 0);
    }
}

// the all-or-nothing pattern of the library's workspaces: mark, allocate, on failure release to the mark
static void case_all_or_nothing()
{
    const int N = 6;
    for (int k = 0; k <= N; ++k) {                                // k == N: nothing fails
        BscMem *m = mem_create();
        void *before = nullptr, *ws[N] = {};
        CHECK(mem_alloc(m, &before, 8, "before") == BSC_OK);
        stub_fail_in(k < N ? k : -1);
        const uint64_t mark = mem_mark(m);
        bsc_status st = BSC_OK;
        for (int i = 0; i < N && st == BSC_OK; ++i)
            st = i & 1 ? mem_alloc_pinned(m, &ws[i], 24, 0, "ws") : mem_alloc(m, &ws[i], 24, "ws");
        if (st != BSC_OK) mem_release_to(m, mark);
        CHECK((st == BSC_OK) == (k == N));
        CHECK(live() == (k == N ? N + 1 : 1) && stub_is_live(before, STUB_DEVICE));
        stub_fail_in(-1);
        mem_release_all(m);
        CHECK(live() == 0);
    }
}

static void case_failed_grow_retries()
{
    BscMem *m = mem_create();
    void *g = nullptr;
    int64_t cap = 0;
    CHECK(mem_grow(m, &g, &cap, 40, false, "g") == BSC_OK);
    stub_fail_in(0);
    CHECK(mem_grow(m, &g, &cap, 80, false, "g") == BSC_E_HIP && g == nullptr && cap == 0 && live() == 0);
    CHECK(strstr(g_err, "80 bytes") && strstr(g_err, "g"));
    CHECK(mem_grow(m, &g, &cap, 80, false, "g") == BSC_OK && cap == 80 && stub_is_live(g, STUB_DEVICE));
    memset(g, 3, 80);
    stub_fail_in(0);
    void *hp = nullptr;
    int64_t hcap = 0;
    CHECK(mem_grow(m, &hp, &hcap, 8, true, "hp") == BSC_E_HIP && hp == nullptr && hcap == 0);
    CHECK(mem_grow(m, &hp, &hcap, 8, true, "hp") == BSC_OK && stub_is_live(hp, STUB_PINNED));
    mem_release_all(m);
    CHECK(live() == 0);
}

int main(int argc, char **argv)
{
    static const struct { const char *name; void (*run)(); } cases[] = {
        {"alloc_free_grow", case_alloc_free_grow},   {"pinned_flags", case_pinned_flags},
        {"free_null_and_released", case_free_null_and_released}, {"mark_release_to", case_mark_release_to},
        {"fail_each", case_fail_each},               {"all_or_nothing", case_all_or_nothing},
        {"failed_grow_retries", case_failed_grow_retries},
    };
    for (auto &c : cases)
        if (argc == 2 && !strcmp(argv[1], c.name)) {
            c.run();
            printf("ok %s\n", c.name);
            return 0;
        }
    fprintf(stderr, "usage: %s <case>\n", argv[0]);
    return 2;
}
