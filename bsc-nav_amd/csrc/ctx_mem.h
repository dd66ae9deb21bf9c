// ctx_mem.h — the ledger of a context's device and pinned-host memory (ctx_mem.cpp; host-only, knows nothing of bsc_ctx).
// Every allocation a context owns is entered there as {pointer, device | pinned}; bsc_destroy frees whatever is entered.  A
// function that builds several buffers takes a mark first and releases everything since the mark when one allocation fails.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bscnav.h"

// a function shared between translation units that stays out of the library's dynamic symbol table
#define BSC_LOCAL __attribute__((visibility("hidden")))

void bsc_set_error(const char *fmt, ...);

struct BscMem;
BSC_LOCAL BscMem *mem_create();                  // nullptr: out of host memory
BSC_LOCAL void mem_release_all(BscMem *m);       // frees every entry with the call that matches its kind, then the ledger
// device memory; 0 bytes are rounded up to a small allocation.  On failure *slot is null, the error names `what` and the size
BSC_LOCAL bsc_status mem_alloc(BscMem *m, void **slot, size_t bytes, const char *what);
// pinned host memory with the runtime's allocation flags: these, or any other of hipHostMalloc's
static const unsigned MEM_PIN_DEFAULT = hipHostMallocDefault, MEM_PIN_MAPPED_COHERENT = hipHostMallocMapped | hipHostMallocCoherent;
BSC_LOCAL bsc_status mem_alloc_pinned(BscMem *m, void **slot, size_t bytes, unsigned flags, const char *what);
BSC_LOCAL void mem_free(BscMem *m, void **slot);   // one entry, early; nulls the slot; nothing to do for a null slot
// *slot holds at least need_bytes afterwards: nothing happens while *cap >= need_bytes, otherwise the old block is freed and exactly
// need_bytes are allocated (contents are not kept; callers add their own slack).  On failure *slot is null and *cap is 0.
BSC_LOCAL bsc_status mem_grow(BscMem *m, void **slot, int64_t *cap, int64_t need_bytes, bool pinned, const char *what);
BSC_LOCAL uint64_t mem_mark(const BscMem *m);
BSC_LOCAL void mem_release_to(BscMem *m, uint64_t mark);   // frees every entry made since mem_mark returned `mark`
// the temporaries of one call: whatever is allocated while it lives is released when it goes out of scope
struct MemScope {
    BscMem *m; uint64_t mark;
    explicit MemScope(BscMem *mem) : m(mem), mark(mem_mark(mem)) {}
    ~MemScope() { mem_release_to(m, mark); }
};
