// ctx_mem.cpp — the ledger of ctx_mem.h: the only place of the library that allocates or frees device / pinned-host memory for
// a context.  Entries are found by pointer value (linear search: a context has about 200, and no timed call comes here).
#include "ctx_mem.h"

#include <stdlib.h>

struct MemEntry { void *p; uint64_t serial; bool pinned; };   // serial: order of allocation, what a mark refers to
struct BscMem { MemEntry *e; size_t n, cap; uint64_t next_serial; };

BscMem *mem_create() { return (BscMem *)calloc(1, sizeof(BscMem)); }

static void release_entry(BscMem *m, size_t i)
{
    (void)(m->e[i].pinned ? hipHostFree(m->e[i].p) : hipFree(m->e[i].p));
    m->e[i] = m->e[--m->n];
}

void mem_release_all(BscMem *m)
{
    if (!m) return;
    while (m->n) release_entry(m, m->n - 1);
    free(m->e);
    free(m);
}

static bsc_status alloc_entry(BscMem *m, void **slot, size_t bytes, bool pinned, unsigned flags, const char *what)
{
    *slot = nullptr;
    if (m->n == m->cap) {                        // room in the ledger first: no allocation is made that cannot be entered
        const size_t cap = m->cap ? 2 * m->cap : 256;
        MemEntry *e = (MemEntry *)realloc(m->e, cap * sizeof(MemEntry));
        if (!e) { bsc_set_error("%s: out of host memory", what); return BSC_E_HIP; }
        m->e = e; m->cap = cap;
    }
    const size_t b = bytes ? bytes : 16;
    const hipError_t err = pinned ? hipHostMalloc(slot, b, flags) : hipMalloc(slot, b);
    if (err != hipSuccess) {
        *slot = nullptr;
        bsc_set_error("%s(%zu bytes) for %s: %s", pinned ? "hipHostMalloc" : "hipMalloc", bytes, what, hipGetErrorString(err));
        return BSC_E_HIP;
    }
    m->e[m->n++] = MemEntry{*slot, m->next_serial++, pinned};
    return BSC_OK;
}

bsc_status mem_alloc(BscMem *m, void **slot, size_t bytes, const char *what) { return alloc_entry(m, slot, bytes, false, 0, what); }
bsc_status mem_alloc_pinned(BscMem *m, void **slot, size_t bytes, unsigned flags, const char *what) { return alloc_entry(m, slot, bytes, true, flags, what); }

void mem_free(BscMem *m, void **slot)
{
    for (size_t i = 0; *slot && i < m->n; ++i)
        if (m->e[i].p == *slot) { release_entry(m, i); break; }
    *slot = nullptr;
}

bsc_status mem_grow(BscMem *m, void **slot, int64_t *cap, int64_t need_bytes, bool pinned, const char *what)
{
    if (*cap >= need_bytes) return BSC_OK;
    mem_free(m, slot);
    *cap = 0;
    const bsc_status st = alloc_entry(m, slot, (size_t)need_bytes, pinned, MEM_PIN_DEFAULT, what);
    if (st == BSC_OK) *cap = need_bytes;
    return st;
}

uint64_t mem_mark(const BscMem *m) { return m->next_serial; }

void mem_release_to(BscMem *m, uint64_t mark)
{
    for (size_t i = m->n; i-- > 0;)              // downwards: the entry that takes a released one's place has been seen
        if (m->e[i].serial >= mark) release_entry(m, i);
}
