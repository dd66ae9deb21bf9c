// score_map.hip — bsc_score_map: the second way out of the cosine scan's similarities.  bsc_localize_regions ranks a query's
// candidates and keeps K of them; this call keeps, for every cell (r, c) of the top-down grid, the best score among the candidates
// standing on it and the height of the voxel that has it — a field over the floor plan instead of a list (memory_2.py:623-671 for
// the scores and the region rules).
//
//   region_scan        (localize.hip) the front half of bsc_localize_regions, unchanged: the same rows, the same scan kernels,
//                      the same candidate list — a candidate's score here has the bits it has in the ranking
//   k_score_scatter    one thread per list entry, looping over the queries of a chunk: 64-bit atomicMax of
//                      (ascending image of the f32 score) << 32 | (descending image of h) into map[q][r * gs + c].  Integer max
//                      does not care about arrival order: the result is the same from run to run, and of two voxels with equal
//                      score the smaller h wins.  0 = nobody wrote: below the key of any score, -inf included.
//   k_score_decode     one thread per (query, cell): key -> score / height in the caller's buffers
// The map of keys is scratch of the context, bounded by working through the queries in chunks (BSC_SCORE_MAP_CHUNK_MB, read per
// call; 256 MiB unless set).
#include "bsc_internal.h"
#include "localize_cand.h"

#include <stdlib.h>

#define TPB 256
#define SCORE_MAP_CHUNK_MB 256.0

__device__ __forceinline__ u64 score_key(float score, int h)
{
    uint32_t u = __float_as_uint(score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);             // ascending: -inf -> 0x007fffff, so no key of a candidate is 0
    return ((u64)u << 32) | (u64)(~(uint32_t)h);                // smaller h, larger key
}

__global__ __launch_bounds__(TPB) void k_score_scatter(RegionCandArgs a, int q0, int nqc, const float *__restrict__ sims,
                                                       int64_t sims_stride, int gs, u64 *__restrict__ map)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= a.n_cand) return;
    int r, cc, h;
    a.position((int)cand_val(a, i), r, cc, h);
    if (r < 0 || r >= gs || cc < 0 || cc >= gs) return;         // (an imported position outside the grid has no cell)
    const int64_t cells = (int64_t)gs * gs;
    u64 *cell = map + (int64_t)r * gs + cc;
    for (int k = 0; k < nqc; ++k) {
        const int q = q0 + k;
        float best;
        if (cand_score(a, i, q, sims + (int64_t)q * sims_stride, best)) atomicMax(cell + (int64_t)k * cells, score_key(best, h));
    }
}

// grid (cells / TPB, queries of the chunk): consecutive threads read consecutive keys and write consecutive outputs
__global__ __launch_bounds__(TPB) void k_score_decode(const u64 *__restrict__ map, int64_t cells, float *__restrict__ score,
                                                      int32_t *__restrict__ height)
{
    const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (c >= cells) return;
    const int64_t o = (int64_t)blockIdx.y * cells + c;
    const u64 key = map[o];
    float s = -INFINITY;
    int32_t h = -1;
    if (key != 0ull) {
        const uint32_t u = (uint32_t)(key >> 32);
        s = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
        h = (int32_t)~(uint32_t)key;
    }
    score[o] = s;
    if (height) height[o] = h;
}

bsc_status score_map_impl(bsc_ctx *x, const float *q_dev, int32_t nq, const bsc_region *regions, float *score_dev, int32_t *height_dev)
{
    hipStream_t s = x->stream;
    RegionScan rg;
    BSC_TRY(region_scan(x, q_dev, nq, regions, &rg));
    const int gs = x->c.grid_size;
    const int64_t cells = (int64_t)gs * gs, per_q = cells * (int64_t)sizeof(u64);
    double mb = SCORE_MAP_CHUNK_MB;
    if (const char *e = getenv("BSC_SCORE_MAP_CHUNK_MB")) {
        const double v = atof(e);
        if (v > 0) mb = v;
    }
    int64_t qc = (int64_t)(mb * 1048576.0) / per_q;             // queries per chunk: at least one, whatever the bound
    qc = qc < 1 ? 1 : (qc > nq ? nq : qc);
    BSC_TRY(mem_grow(x->mem, (void **)&x->sm_map, &x->sm_cap, per_q * qc, false, "score map scratch"));
    const unsigned cblocks = (unsigned)((cells + TPB - 1) / TPB);
    for (int q0 = 0; q0 < nq; q0 += (int)qc) {
        const int n = (int)(nq - q0 < qc ? nq - q0 : qc);
        BSC_HIP(hipMemsetAsync(x->sm_map, 0, (size_t)(per_q * n), s));
        if (!rg.nothing && rg.ca.n_cand > 0)
            hipLaunchKernelGGL(k_score_scatter, dim3((unsigned)((rg.ca.n_cand + TPB - 1) / TPB)), dim3(TPB), 0, s, rg.ca, q0, n,
                               (const float *)x->l_sims, rg.sstride, gs, x->sm_map);
        hipLaunchKernelGGL(k_score_decode, dim3(cblocks, (unsigned)n), dim3(TPB), 0, s, (const u64 *)x->sm_map, cells,
                           score_dev + (int64_t)q0 * cells, height_dev ? height_dev + (int64_t)q0 * cells : nullptr);
    }
    BSC_HIP(hipGetLastError());
    BSC_HIP(hipStreamSynchronize(s));
    return BSC_OK;
}
