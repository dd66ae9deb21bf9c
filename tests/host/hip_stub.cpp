// hip_stub.cpp — the four HIP allocation calls of csrc/ctx_mem.cpp on the host, malloc-backed, with the books a test needs:
// every live pointer with its kind, a counter of calls, "fail the k-th allocation from now", and abort() on a free of an
// unknown pointer or through the wrong call.
#include "hip_stub.h"

#include <stdio.h>
#include <stdlib.h>

#include <map>

static std::map<void *, StubKind> g_live;
static long g_calls = 0, g_fail_in = -1;
static unsigned g_last_flags = 0;

long stub_live(StubKind kind)
{
    long n = 0;
    for (auto &kv : g_live) n += kv.second == kind;
    return n;
}
long stub_calls() { return g_calls; }
unsigned stub_last_flags() { return g_last_flags; }
void stub_fail_in(long k) { g_fail_in = k; }
bool stub_is_live(const void *p, StubKind kind)
{
    auto it = g_live.find((void *)p);
    return it != g_live.end() && it->second == kind;
}

static hipError_t stub_alloc(void **p, size_t bytes, StubKind kind)
{
    ++g_calls;
    if (bytes == 0) { fprintf(stderr, "stub: allocation of 0 bytes\n"); abort(); }
    if (g_fail_in == 0) { g_fail_in = -1; return hipErrorOutOfMemory; }      // *p is left as it was, like the runtime
    if (g_fail_in > 0) --g_fail_in;
    *p = malloc(bytes);
    g_live[*p] = kind;
    return hipSuccess;
}

static hipError_t stub_release(void *p, StubKind kind)
{
    ++g_calls;
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) {
        fprintf(stderr, "stub: %s of %p, which is %s\n", kind == STUB_DEVICE ? "hipFree" : "hipHostFree", p,
                it == g_live.end() ? "not live" : "of the other kind");
        abort();
    }
    g_live.erase(it);
    free(p);
    return hipSuccess;
}

extern "C" hipError_t hipMalloc(void **p, size_t bytes) { return stub_alloc(p, bytes, STUB_DEVICE); }
extern "C" hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int flags)
{
    g_last_flags = flags;
    return stub_alloc(p, bytes, STUB_PINNED);
}
extern "C" hipError_t hipFree(void *p) { return stub_release(p, STUB_DEVICE); }
extern "C" hipError_t hipHostFree(void *p) { return stub_release(p, STUB_PINNED); }
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (stub)" : "stub error"; }
