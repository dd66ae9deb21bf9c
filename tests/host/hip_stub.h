// hip_stub.h — what the ledger test asks of the stubbed HIP allocation calls (hip_stub.cpp)
#pragma once
#include <hip/hip_runtime_api.h>

enum StubKind { STUB_DEVICE = 0, STUB_PINNED = 1 };
long stub_live(StubKind kind);                       // live pointers of that kind
bool stub_is_live(const void *p, StubKind kind);
long stub_calls();                                   // allocation + free calls so far
unsigned stub_last_flags();                          // flags of the last hipHostMalloc
void stub_fail_in(long k);                           // the k-th allocation from now (0 = the next) fails once; -1: none
