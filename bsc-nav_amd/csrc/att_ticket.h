// att_ticket.h — how the persistent attention workgroups (k_attention, k_attention32: encoder_ops.hip; k_attention_split:
// encoder_gemm.hip) hand out their (image, head) items.
//
// Items are handed out by a ticket counter (work[0]; work[1] counts finished workgroups, the last one re-arms both), not by a static
// stride: a workgroup whose CU is shared with another stream's kernel simply takes fewer items.  With the static stride one slow or
// late workgroup stretched the whole launch — the rgb chain of libbscnav's own side stream, resident on one or two CUs for
// milliseconds, cost the 12 attention launches of a ViT-B forward 2.4 ms (bench pipeline 24.7 -> 22.x ms per step).
// work == nullptr keeps the static stride.  s_ticket: one int of the workgroup's LDS.
#pragma once
#include "bsc_internal.h"

// the workgroup's first item (a workgroup barrier inside when there is a counter)
__device__ __forceinline__ int att_first_item(int *work, int &s_ticket, int tid)
{
    if (!work) return blockIdx.x;
    if (tid == 0) s_ticket = atomicAdd(&work[0], 1);
    __syncthreads();
    return s_ticket;
}

// The item after `item`, in two steps round the barrier that ends the staging of `item`: att_take_ticket before it (everyone has
// read the previous ticket: the barrier that opens the staging lies in between), att_next_item after it.
__device__ __forceinline__ void att_take_ticket(int *work, int &s_ticket, int tid)
{
    if (work && tid == 0) s_ticket = atomicAdd(&work[0], 1);
}
__device__ __forceinline__ int att_next_item(const int *work, const int &s_ticket, int item)
{
    return work ? s_ticket : item + (int)gridDim.x;
}

// the last workgroup to leave re-arms the counters for the next launch on this stream
__device__ __forceinline__ void att_rearm(int *work, int tid)
{
    if (work && tid == 0) {
        __threadfence();
        if (atomicAdd(&work[1], 1) == (int)gridDim.x - 1) {
            work[0] = 0;
            work[1] = 0;
            __threadfence();
        }
    }
}
