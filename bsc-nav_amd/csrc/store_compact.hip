// store_compact.hip — reclaiming the dead rows of the token pool (exact mode).
//
// update_memory_surp_base merges the tokens of a group (memory_2.py:386-446): the mean goes into the pool row of the component's
// smallest slot, the other rows of the component stay allocated and nothing refers to them any more (surprise.hip).  DS_POOL_N
// therefore grows by up to iter_size rows per surprise flush while the live store is bounded by voxels x cache_size, and the
// exact-mode scan of bsc_localize streams every row below DS_POOL_N.  Compaction moves the live rows to pool rows [0, L), L =
// their number, in place and with the fewest copies:
//   k_compact_mark   a byte per pool row: some store_rows[e][k], k < store_cnt[e], names it (entry vcap, grid_0_0_0, included)
//   k_compact_count  per 256 rows: holes (dead rows below L) and movers (live rows at or above L); both lists have M entries
//   k_compact_lists  the two lists in index order (block scan + the exclusive prefix of the block totals)
//   k_compact_move   one wavefront per pair (mover k -> hole k): token row as float4 per lane, its distance, its cached scale /
//                    inverse norm of the fp16-piece scan when that cache is current; remap[mover - L] = hole
//   k_compact_remap  store_rows entries >= L through the remap table
// Sources (>= L) and destinations (< L, dead) are disjoint: no second pool, no row read after it was overwritten.  The order of
// the rows inside the pool is not observable (exports, candidates and the gathered scan go through store_rows).
#include "bsc_internal.h"

#include <stdlib.h>
#include <chrono>

#define TPB 256

bool store_compact_auto()
{
    const char *e = getenv("BSC_STORE_COMPACT");      // never | auto (default), read per call like BSC_REGION_PRUNE
    return !(e && !strcmp(e, "never"));
}

__global__ __launch_bounds__(TPB) void k_compact_mark(int64_t n_slots, int cs, const int32_t *__restrict__ store_cnt,
                                                      const int32_t *__restrict__ store_rows, int64_t pool_n,
                                                      uint8_t *__restrict__ mark)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_slots) return;
    const int64_t e = i / cs;
    if ((int)(i - e * cs) >= store_cnt[e]) return;
    const int32_t r = store_rows[i];
    if (r >= 0 && r < pool_n) mark[r] = 1;
}

__device__ __forceinline__ void compact_flags(int64_t i, int64_t pool_n, int64_t L, const uint8_t *__restrict__ mark, int &hole,
                                              int &mover)
{
    const bool in = i < pool_n, live = in && mark[i] != 0;
    hole = (in && i < L && !live) ? 1 : 0;
    mover = (live && i >= L) ? 1 : 0;
}

// per block of TPB rows: holes << 32 | movers
__global__ __launch_bounds__(TPB) void k_compact_count(int64_t pool_n, int64_t L, const uint8_t *__restrict__ mark,
                                                       int64_t *__restrict__ blk_tot)
{
    int hole, mover, eh, em, th, tm;
    compact_flags((int64_t)blockIdx.x * TPB + threadIdx.x, pool_n, L, mark, hole, mover);
    block_scan2<TPB>(hole, mover, eh, em, th, tm);
    if (threadIdx.x == 0) blk_tot[blockIdx.x] = ((int64_t)th << 32) | (int64_t)tm;
}

__global__ __launch_bounds__(TPB) void k_compact_lists(int64_t pool_n, int64_t L, const uint8_t *__restrict__ mark,
                                                       const int64_t *__restrict__ blk_off, int64_t M, int32_t *__restrict__ holes,
                                                       int32_t *__restrict__ movers)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    int hole, mover, eh, em, th, tm;
    compact_flags(i, pool_n, L, mark, hole, mover);
    block_scan2<TPB>(hole, mover, eh, em, th, tm);
    const int64_t base = blk_off[blockIdx.x];
    const int64_t kh = (base >> 32) + eh, km = (base & 0xffffffffll) + em;
    if (hole && kh < M) holes[kh] = (int32_t)i;
    if (mover && km < M) movers[km] = (int32_t)i;
}

// one wavefront per pair
__global__ __launch_bounds__(TPB) void k_compact_move(int64_t M, int64_t L, const int32_t *__restrict__ holes,
                                                      const int32_t *__restrict__ movers, int D, float *pool, float *pool_d,
                                                      float2 *rscale, int32_t *__restrict__ remap)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    if (k >= M) return;
    const int64_t src = movers[k], dst = holes[k];
    const float4 *s = (const float4 *)(pool + src * D);
    float4 *d = (float4 *)(pool + dst * D);
    for (int v = lane; v < (D >> 2); v += 64) d[v] = s[v];
    if (lane == 0) {
        pool_d[dst] = pool_d[src];
        if (rscale) rscale[dst] = rscale[src];
        remap[src - L] = (int32_t)dst;
    }
}

__global__ __launch_bounds__(TPB) void k_compact_remap(int64_t n_slots, int cs, const int32_t *__restrict__ store_cnt,
                                                       int32_t *__restrict__ store_rows, int64_t L, int64_t pool_n,
                                                       const int32_t *__restrict__ remap)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_slots) return;
    const int64_t e = i / cs;
    if ((int)(i - e * cs) >= store_cnt[e]) return;
    const int32_t r = store_rows[i];
    if (r >= L && r < pool_n) store_rows[i] = remap[r - L];
}

bsc_status compact_store_impl(bsc_ctx *x, int64_t live_known, int64_t *rows_before, int64_t *rows_after)
{
    hipStream_t s = x->stream;
    const int64_t vcap = x->c.voxel_capacity;
    const int cs = x->c.cache_size, D = x->c.token_dim;
    BSC_TRY(sync_all(x));                        // nothing in flight reads or writes the pool
    int64_t L = live_known;
    if (L < 0) {
        BSC_TRY(enqueue_store_totals(x));
        BSC_TRY(read_scalars(x));
        L = x->hscal[DS_TMP1];
    }
    const int64_t pool_n = x->pool_n_host;
    if (rows_before) *rows_before = pool_n;
    if (rows_after) *rows_after = pool_n;
    if (L > pool_n || pool_n > x->c.token_capacity) {
        bsc_set_error("token store: %lld live rows in a pool of %lld (capacity %lld)", (long long)L, (long long)pool_n,
                      (long long)x->c.token_capacity);
        return BSC_E_STATE;
    }
    if (L == pool_n) return BSC_OK;              // no dead row
    int64_t M = 0;
    if (L > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        // the scratch stays with the context and grows on demand, as that of bsc_localize_regions: no allocation per call
        struct { uint8_t *mark; int64_t *blk_tot, *blk_off; int32_t *holes, *movers, *remap; } w;
        const int64_t nblk = (pool_n + TPB - 1) / TPB, n_slots = (vcap + 1) * cs;
        const dim3 block(TPB), rgrid((unsigned)nblk), sgrid((unsigned)((n_slots + TPB - 1) / TPB));
        BSC_TRY(mem_grow(x->mem, &x->cp_buf[0], &x->cp_cap[0], pool_n + pool_n / 8 + 1024, false, "compaction scratch"));
        BSC_TRY(mem_grow(x->mem, &x->cp_buf[1], &x->cp_cap[1], (int64_t)sizeof(int64_t) * (nblk + nblk / 8 + 64), false, "compaction scratch"));
        BSC_TRY(mem_grow(x->mem, &x->cp_buf[2], &x->cp_cap[2], (int64_t)sizeof(int64_t) * (nblk + nblk / 8 + 64), false, "compaction scratch"));
        w.mark = (uint8_t *)x->cp_buf[0];
        w.blk_tot = (int64_t *)x->cp_buf[1];
        w.blk_off = (int64_t *)x->cp_buf[2];
        BSC_HIP(hipMemsetAsync(w.mark, 0, (size_t)pool_n, s));
        BSC_HIP(hipMemsetAsync(w.blk_tot + nblk, 0, sizeof(int64_t), s));       // the scan's last output is the total
        hipLaunchKernelGGL(k_compact_mark, sgrid, block, 0, s, n_slots, cs, x->store_cnt, x->store_rows, pool_n, w.mark);
        hipLaunchKernelGGL(k_compact_count, rgrid, block, 0, s, pool_n, L, (const uint8_t *)w.mark, w.blk_tot);
        BSC_TRY(prim_exclusive_sum_i64(lane_main(x), w.blk_tot, w.blk_off, (size_t)nblk + 1));
        int64_t tot = 0;
        BSC_HIP(hipGetLastError());
        BSC_HIP(hipMemcpyAsync(&tot, w.blk_off + nblk, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        BSC_HIP(hipStreamSynchronize(s));
        M = tot & 0xffffffffll;
        if ((tot >> 32) != M) {                  // every live row is named once: holes below L == live rows above it
            bsc_set_error("token store: %lld holes for %lld rows to move (a pool row named twice?)", (long long)(tot >> 32), (long long)M);
            return BSC_E_STATE;
        }
        if (M > 0) {
            // the cached scales move with their rows when they are current (cosine_scan.hip refresh_row_scales)
            const bool scales = !x->row_scale_dirty && x->l_rscale && x->l_rscale_cap >= (int64_t)sizeof(float2) * pool_n;
            BSC_TRY(mem_grow(x->mem, &x->cp_buf[3], &x->cp_cap[3], (int64_t)sizeof(int32_t) * (M + M / 8 + 1024), false, "compaction scratch"));
            BSC_TRY(mem_grow(x->mem, &x->cp_buf[4], &x->cp_cap[4], (int64_t)sizeof(int32_t) * (M + M / 8 + 1024), false, "compaction scratch"));
            BSC_TRY(mem_grow(x->mem, &x->cp_buf[5], &x->cp_cap[5], (int64_t)sizeof(int32_t) * (pool_n - L + (pool_n - L) / 8 + 1024), false, "compaction scratch"));
            w.holes = (int32_t *)x->cp_buf[3];
            w.movers = (int32_t *)x->cp_buf[4];
            w.remap = (int32_t *)x->cp_buf[5];
            hipLaunchKernelGGL(k_compact_lists, rgrid, block, 0, s, pool_n, L, (const uint8_t *)w.mark, (const int64_t *)w.blk_off, M,
                               w.holes, w.movers);
            hipLaunchKernelGGL(k_compact_move, dim3((unsigned)((M * 64 + TPB - 1) / TPB)), block, 0, s, M, L, (const int32_t *)w.holes,
                               (const int32_t *)w.movers, D, x->pool, x->pool_d, scales ? x->l_rscale : (float2 *)nullptr, w.remap);
            hipLaunchKernelGGL(k_compact_remap, sgrid, block, 0, s, n_slots, cs, x->store_cnt, x->store_rows, L, pool_n,
                               (const int32_t *)w.remap);
            BSC_HIP(hipGetLastError());
            BSC_HIP(hipStreamSynchronize(s));
            if (!scales) x->row_scale_dirty = true;
            x->cp_runs++;
            x->cp_rows_moved += M;
            x->cp_usec += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        }
    }
    // the scalars as a flush leaves them
    BSC_HIP(hipMemcpy(x->dscal + DS_POOL_N, &L, sizeof(int64_t), hipMemcpyHostToDevice));
    x->hscal[DS_POOL_N] = L;
    x->pool_n_host = L;
    if (rows_after) *rows_after = L;
    return BSC_OK;
}

bsc_status reserve_pool_rows(bsc_ctx *x, int64_t n)
{
    if (x->pool_n_host + n <= x->c.token_capacity) return BSC_OK;
    if (store_compact_auto() && x->pool_n_host > 0) BSC_TRY(compact_store_impl(x, -1, nullptr, nullptr));
    return grow_token_pool(x, x->pool_n_host + n);
}
