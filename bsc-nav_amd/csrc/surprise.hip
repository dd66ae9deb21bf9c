// surprise.hip — update_memory_surp_base (memory_2.py:364-536) for the device-resident token cache, exact mode.
//
// Reference semantics, for EVERY cache row i in order (the unused zero rows at [0,0,0] included):
//   group missing -> create it with this token (:471-478), nothing else;
//   otherwise surprise = min_k (1 - cos(token, n_k)) over the tokens of every existing group at the (2r+1)^3 - 1 positions
//   around the voxel (+inf with none; NaN propagates: a zero token gives NaN and NaN > threshold is false) (:366-384, :480-500);
//   surprise > surprise_threshold -> append (fewer than cache_size tokens) or overwrite the slot of the smallest 1 - cos
//   (argmin: first NaN, else first minimum) (:448-468), then forgetting (:386-446): components of the graph
//   sim(i, j) > boring_threshold, one token per component in the order of its smallest index, a singleton unchanged, a larger
//   component the mean of its tokens and of its distances.
//
// Schedule.  Row i depends only on the last earlier row at each voxel of its closed neighbourhood.  Consecutive rows at one voxel
// form a TASK (their neighbours cannot change in between: the zero tail is one task); a task's LEVEL is 1 + the largest level of
// the last earlier task at any voxel within Chebyshev distance r, computed in one sequential pass by one wavefront over a level
// table in LDS (k_surp_levels).  Tasks of one level sit at pairwise distance > r: they read neighbour groups and write only their
// own group without conflict, so each level is one launch of k_surp_task, one workgroup per task:
//   A  the neighbour groups' pool rows into LDS (all threads);
//   B  surprise of every row of the task (neighbours fixed within the task): lanes over neighbour tokens, row token in LDS;
//   C  wavefront 0 walks the accepted rows in order with the group held in LDS (pool row, pending cache row, distance, inverse
//      norm, adjacency bit mask per slot): add / replace from one pass of dots, components by a Warshall closure on the bit
//      masks, means written into the pool row of the component's smallest slot; cache rows are copied into the pool once, at
//      the end of the task.
#include "bsc_internal.h"

#include <math.h>
#include <stdlib.h>

#define TPB 256
#define SURP_RMAX 3                 // largest neighbour radius: (2r+1)^3 = 343 closed-neighbourhood positions
#define SURP_TASK_LDS 49152         // k_surp_task's dynamic LDS: neighbour rows + their inverse norms + one token
#define SURP_TAB16 81920            // level table entries in LDS (160 KiB) as u16 / as u32
#define SURP_TAB32 40960

struct SurpriseWs {
    int64_t k_cap;                  // neighbour lists sized for closed neighbourhoods of k_cap positions
    int32_t *ent, *head, *tid, *first, *dense;   // per row
    int32_t *tstart, *tent, *lvl, *order;        // per task
    int32_t *cid;                   // (vcap + 1): compact id of a store entry that hosts a task
    int32_t *nb;                    // (tasks, k_cap): compact ids of the closed neighbourhood, -1 where no task voxel
    int32_t *lcnt, *loff;           // per level: tasks, first position in `order`
    int32_t *lvtab;                 // level table when it does not fit in LDS
    float *inv;                     // per row: 1 / |token| (NaN for a zero token)
    int32_t *acc;                   // per row: surprise > threshold
    int32_t *scal;                  // [0] tasks [1] task voxels [2] levels
};

// scratch on the first call (bsc_create allocates nothing for this path), all of it or none: x->surp is published once every
// buffer exists.  The neighbour lists grow with the radius; a failed regrow leaves k_cap == 0 and the next call tries again.
static bsc_status ws_ensure(bsc_ctx *x, int K)
{
    const int64_t n = x->c.iter_size, vcap = x->c.voxel_capacity;
    SurpriseWs *w = x->surp;
    if (!w) {
        w = (SurpriseWs *)calloc(1, sizeof(SurpriseWs));
        if (!w) { bsc_set_error("bsc_flush_surprise: out of host memory"); return BSC_E_HIP; }
        const struct { int32_t **slot; int64_t count; } want[] = {
            {&w->ent, n}, {&w->head, n}, {&w->tid, n}, {&w->first, n}, {&w->dense, n}, {&w->tstart, n + 1}, {&w->tent, n}, {&w->lvl, n},
            {&w->order, n}, {&w->cid, vcap + 1}, {&w->lcnt, n + 2}, {&w->loff, n + 2}, {(int32_t **)&w->inv, n}, {&w->acc, n}, {&w->scal, 4}};
        const uint64_t mark = mem_mark(x->mem);
        for (const auto &a : want) {             // every one is 4 bytes per element (inv: float)
            const bsc_status st = mem_alloc(x->mem, (void **)a.slot, sizeof(int32_t) * (size_t)a.count, "surprise flush scratch");
            if (st != BSC_OK) { mem_release_to(x->mem, mark); free(w); return st; }
        }
        x->surp = w;
    }
    if (w->k_cap < K) {
        mem_free(x->mem, (void **)&w->nb);
        w->k_cap = 0;
        BSC_TRY(mem_alloc(x->mem, (void **)&w->nb, sizeof(int32_t) * (size_t)n * K, "surprise flush neighbour lists"));
        w->k_cap = K;
    }
    return BSC_OK;
}

// store entry of a cache row: entry vcap is the group "grid_0_0_0" (as k_flush_keys)
__device__ __forceinline__ int32_t surp_entry(const int32_t *__restrict__ occ, int64_t cell, int vcap)
{
    if (cell == 0) return vcap;
    const int32_t e = occ[cell];
    return e < 0 ? vcap : e;
}

__device__ __forceinline__ float inv_norm_of(float sumsq) { return sumsq > 0.f ? 1.0f / sqrtf(sumsq) : __int_as_float(0x7fc00000); }

__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc)
{
    return acc + ((a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w));
}

// LDS + global written by lanes of this wavefront become visible to its other lanes
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// ---- plan ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_surp_rows(int n, const int32_t *__restrict__ cache_pos, const int32_t *__restrict__ occ,
                                                   int gs, int nh, int vcap, int32_t *__restrict__ ent, int32_t *__restrict__ head)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    auto entry_of = [&](int j) {
        const int64_t cell = ((int64_t)cache_pos[3 * j] * gs + cache_pos[3 * j + 1]) * nh + cache_pos[3 * j + 2];
        return surp_entry(occ, cell, vcap);
    };
    const int32_t e = entry_of(i);
    ent[i] = e;
    head[i] = (i == 0) || (entry_of(i - 1) != e);
}

// one wavefront per row: 1 / |token| in f32 (NaN for a zero token: memory_2.py:379 divides by the norm)
__global__ __launch_bounds__(TPB) void k_surp_rowinv(int n, const float *__restrict__ cache_f, int D, float *__restrict__ inv)
{
    const int lane = threadIdx.x & 63;
    const int r = (blockIdx.x * TPB + threadIdx.x) >> 6;
    if (r >= n) return;
    const float4 *row = (const float4 *)(cache_f + (int64_t)r * D);
    float s = 0.f;
    for (int v = lane; v < (D >> 2); v += 64) s = dot4(row[v], row[v], s);
    s = wave_sum(s);
    if (lane == 0) inv[r] = inv_norm_of(s);
}

__global__ __launch_bounds__(TPB) void k_surp_tasks(int n, const int32_t *__restrict__ ent, const int32_t *__restrict__ head,
                                                    const int32_t *__restrict__ tid, int32_t *__restrict__ tstart,
                                                    int32_t *__restrict__ tent, int32_t *cid, int32_t *scal)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if (head[i]) {
        const int32_t t = tid[i];
        tstart[t] = i;
        tent[t] = ent[i];
        atomicMin(&cid[ent[i]], t);
    }
    if (i == n - 1) {
        const int32_t nt = tid[i] + head[i];
        scal[0] = nt;
        tstart[nt] = n;
    }
}

__global__ __launch_bounds__(TPB) void k_surp_first(int n, const int32_t *__restrict__ ent, const int32_t *__restrict__ head,
                                                    const int32_t *__restrict__ tid, const int32_t *__restrict__ cid,
                                                    int32_t *__restrict__ first)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    first[i] = head[i] && cid[ent[i]] == tid[i];
}

__global__ __launch_bounds__(TPB) void k_surp_dense(int n, const int32_t *__restrict__ ent, const int32_t *__restrict__ first,
                                                    const int32_t *__restrict__ dense, int32_t *cid, int32_t *scal)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if (first[i]) cid[ent[i]] = dense[i];
    if (i == n - 1) scal[1] = dense[i] + first[i];
}

// closed neighbourhood of every task as compact ids (-1: no task at that position); offset (0,0,0) sits at K / 2
__global__ __launch_bounds__(TPB) void k_surp_nbrs(int n, int r, const int32_t *__restrict__ cache_pos,
                                                   const int32_t *__restrict__ head, const int32_t *__restrict__ tid,
                                                   const int32_t *__restrict__ occ, const int32_t *__restrict__ cid, int gs, int nh,
                                                   int vcap, int32_t n_u, int32_t *__restrict__ nb)
{
    const int w = 2 * r + 1, K = w * w * w;
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= (int64_t)n * K) return;
    const int i = (int)(g / K), o = (int)(g % K);
    if (!head[i]) return;
    const int32_t pr = cache_pos[3 * i] + o / (w * w) - r, pc = cache_pos[3 * i + 1] + (o / w) % w - r,
                  ph = cache_pos[3 * i + 2] + o % w - r;
    int32_t v = -1;
    if (pr >= 0 && pc >= 0 && ph >= 0 && pr < gs && pc < gs && ph < nh) {
        const int64_t cell = ((int64_t)pr * gs + pc) * nh + ph;
        const int32_t e = cell == 0 ? vcap : occ[cell];
        if (e >= 0) {
            const int32_t c = cid[e];
            v = c < n_u ? c : -1;
        }
    }
    nb[(int64_t)tid[i] * K + o] = v;
}

// level recurrence: one wavefront, tasks in order, lanes over the closed neighbourhood
template <typename T>
__device__ __forceinline__ void surp_levels_body(T *tab, int n_u, int n_tasks, int K, const int32_t *__restrict__ nb,
                                                 int32_t *__restrict__ lvl, int32_t *lcnt, int32_t *scal)
{
    const int lane = threadIdx.x;
    for (int i = lane; i < n_u; i += 64) tab[i] = 0;
    __syncthreads();
    const int per = (K + 63) / 64;   // <= 6
    int32_t cur[6], nxt[6];
    for (int q = 0; q < 6; ++q) {
        const int j = lane + 64 * q;
        cur[q] = (q < per && j < K && n_tasks > 0) ? nb[j] : -1;
    }
    int32_t lmax = 0;
    for (int t = 0; t < n_tasks; ++t) {
        for (int q = 0; q < 6; ++q) {
            const int j = lane + 64 * q;
            nxt[q] = (q < per && j < K && t + 1 < n_tasks) ? nb[(int64_t)(t + 1) * K + j] : -1;
        }
        int32_t m = 0;
        for (int q = 0; q < 6; ++q)
            if (cur[q] >= 0) { const int32_t l = (int32_t)tab[cur[q]]; m = l > m ? l : m; }
        for (int o = 32; o > 0; o >>= 1) { const int32_t y = __shfl_xor(m, o); m = y > m ? y : m; }
        const int32_t L = m + 1;
        int32_t mine = -1;
        for (int q = 0; q < 6; ++q)
            if (lane + 64 * q == K / 2) mine = cur[q];
        const int32_t self = __shfl(mine, (K / 2) % 64);
        if (lane == 0) {
            tab[self] = (T)L;
            lvl[t] = L;
            atomicAdd(&lcnt[L], 1);
        }
        lmax = L > lmax ? L : lmax;
        __syncthreads();   // the table write is seen by every lane of the next task
        for (int q = 0; q < 6; ++q) cur[q] = nxt[q];
    }
    if (lane == 0) scal[2] = lmax;
}

template <typename T, int CAP>
__global__ __launch_bounds__(64) void k_surp_levels(int n_u, int n_tasks, int K, const int32_t *__restrict__ nb,
                                                    int32_t *__restrict__ lvl, int32_t *lcnt, int32_t *scal)
{
    __shared__ T tab[CAP];
    surp_levels_body<T>(tab, n_u, n_tasks, K, nb, lvl, lcnt, scal);
}

// more task voxels than the LDS table holds: the same pass on a table in global memory (one workgroup: workgroup-scope fences
// of __syncthreads order its writes before the next task's reads)
__global__ __launch_bounds__(64) void k_surp_levels_global(int32_t *tab, int n_u, int n_tasks, int K, const int32_t *__restrict__ nb,
                                                           int32_t *__restrict__ lvl, int32_t *lcnt, int32_t *scal)
{
    surp_levels_body<int32_t>(tab, n_u, n_tasks, K, nb, lvl, lcnt, scal);
}

__global__ __launch_bounds__(TPB) void k_surp_scatter(int n_tasks, const int32_t *__restrict__ lvl, const int32_t *__restrict__ loff,
                                                      int32_t *fill, int32_t *__restrict__ order)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n_tasks) return;
    const int32_t L = lvl[t];
    order[loff[L] + atomicAdd(&fill[L], 1)] = t;
}

// ---- one level: one workgroup per task ----------------------------------------------------------------------------------------
struct SurpArgs {
    const int32_t *order, *tstart, *tent;
    const int32_t *cache_pos, *occ;
    const float *cache_f, *cache_d, *inv;
    int32_t *acc;
    int32_t *store_rows, *store_cnt;
    float *pool, *pool_d;
    int64_t *dscal;
    int64_t token_cap;
    int gs, nh, vcap, cs, D, r;
    double sthr;
    float bthr;
};

__device__ __forceinline__ const float *slot_tok(const SurpArgs &a, int src, int prow)
{
    return src >= 0 ? a.cache_f + (int64_t)src * a.D : a.pool + (int64_t)prow * a.D;
}

__global__ __launch_bounds__(TPB) void k_surp_task(SurpArgs a)
{
    extern __shared__ float dyn[];
    const int K1 = (2 * a.r + 1) * (2 * a.r + 1) * (2 * a.r + 1) - 1;
    const int nbmax = K1 * a.cs;
    int32_t *nrow = (int32_t *)dyn;                  // pool rows of the neighbour tokens
    float *ninv = dyn + nbmax;                       // their inverse norms
    float *xs = dyn + 2 * nbmax;                     // one token (D)
    __shared__ int32_t s_n, s_nan, s_ndot, s_dotrows[TPB];
    __shared__ float s_min[4];
    __shared__ int32_t s_anynan[4];
    // the group, slot by slot (wavefront 0 only)
    __shared__ int32_t sl_prow[64], sl_src[64];
    __shared__ float sl_dist[64], sl_inv[64];
    __shared__ u64 sl_adj[64];
    __shared__ int32_t t_prow[64], t_src[64];
    __shared__ float t_dist[64], t_inv[64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, D4 = D >> 2, cs = a.cs;
    const int32_t task = a.order[blockIdx.x];
    const int32_t r0 = a.tstart[task], r1 = a.tstart[task + 1], e = a.tent[task];
    const int32_t vr = a.cache_pos[3 * r0], vc = a.cache_pos[3 * r0 + 1], vh = a.cache_pos[3 * r0 + 2];

    // ---- A: pool rows of every existing neighbour group (memory_2.py:482-494); their order does not matter to a minimum
    if (tid == 0) { s_n = 0; s_nan = 0; }
    __syncthreads();
    const int w = 2 * a.r + 1;
    for (int o = tid; o < K1 + 1; o += TPB) {
        if (o == K1 / 2) continue;   // the voxel itself (:369)
        const int32_t pr = vr + o / (w * w) - a.r, pc = vc + (o / w) % w - a.r, ph = vh + o % w - a.r;
        if (pr < 0 || pc < 0 || ph < 0 || pr >= a.gs || pc >= a.gs || ph >= a.nh) continue;
        const int64_t cell = ((int64_t)pr * a.gs + pc) * a.nh + ph;
        const int32_t ne = cell == 0 ? a.vcap : a.occ[cell];
        if (ne < 0) continue;
        const int32_t c = a.store_cnt[ne];
        if (c <= 0) continue;
        const int32_t base = atomicAdd(&s_n, c);
        for (int k = 0; k < c; ++k) nrow[base + k] = a.store_rows[(int64_t)ne * cs + k];
    }
    __syncthreads();
    const int N = s_n;

    // ---- B: surprise of every row (the neighbours cannot change inside the task)
    bool norms_done = false;
    for (int c0 = r0; c0 < r1; c0 += TPB) {
        const int rr = c0 + tid;
        __syncthreads();   // every thread has read the previous chunk's list
        if (tid == 0) s_ndot = 0;
        __syncthreads();
        if (rr < r1) {
            const float xi = a.inv[rr];
            // zero token: NaN with neighbours; no neighbour token: +inf (:375-377), compared like any other value (:500)
            if (xi != xi || N == 0) a.acc[rr] = (N == 0) && (double)INFINITY > a.sthr;
            else s_dotrows[atomicAdd(&s_ndot, 1)] = rr;
        }
        __syncthreads();
        const int nd = s_ndot;
        if (nd > 0 && !norms_done) {
            for (int j = tid; j < N; j += TPB) {
                const float4 *p = (const float4 *)(a.pool + (int64_t)nrow[j] * D);
                float s = 0.f;
                for (int v = 0; v < D4; ++v) s = dot4(p[v], p[v], s);
                const float iv = inv_norm_of(s);
                ninv[j] = iv;
                if (iv != iv) s_nan = 1;
            }
            norms_done = true;
            __syncthreads();
        }
        for (int q = 0; q < nd; ++q) {
            const int32_t row = s_dotrows[q];
            if (s_nan) {                      // a zero neighbour token: its cosine is NaN, and so is the minimum
                if (tid == 0) a.acc[row] = 0;
                continue;
            }
            const float4 *xr = (const float4 *)(a.cache_f + (int64_t)row * D);
            for (int v = tid; v < D4; v += TPB) ((float4 *)xs)[v] = xr[v];
            __syncthreads();
            const float xi = a.inv[row];
            float mn = INFINITY;
            int anynan = 0;
            for (int j = tid; j < N; j += TPB) {
                const float4 *p = (const float4 *)(a.pool + (int64_t)nrow[j] * D);
                float s = 0.f;
                for (int v = 0; v < D4; ++v) s = dot4(p[v], ((const float4 *)xs)[v], s);
                const float d = 1.0f - s * ninv[j] * xi;
                if (d != d) anynan = 1;
                else mn = fminf(mn, d);
            }
            for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); anynan |= __shfl_xor(anynan, o); }
            if (lane == 0) { s_min[wave] = mn; s_anynan[wave] = anynan; }
            __syncthreads();
            if (tid == 0) {
                const float m = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
                const int nan = s_anynan[0] | s_anynan[1] | s_anynan[2] | s_anynan[3];
                a.acc[row] = !nan && (double)m > a.sthr;   // :500, compared as a Python float
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- C: the accepted rows in order, wavefront 0, lane = slot
    int cnt = a.store_cnt[e];
    bool gram = false, changed = false;
    if (lane < cnt) {
        const int32_t pr = a.store_rows[(int64_t)e * cs + lane];
        sl_prow[lane] = pr;
        sl_src[lane] = -1;
        sl_dist[lane] = a.pool_d[pr];
    }
    int rstart = r0;
    if (cnt == 0) {   // group missing: create it with the first row (:471-478)
        if (lane == 0) {
            const int64_t pr = (int64_t)atomicAdd((u64 *)&a.dscal[DS_POOL_N], 1ull);
            if (pr >= a.token_cap) a.dscal[DS_ERROR] = 2;
            sl_prow[0] = pr < a.token_cap ? (int32_t)pr : 0;
            sl_src[0] = r0;
            sl_dist[0] = a.cache_d[r0];
            sl_inv[0] = a.inv[r0];
            sl_adj[0] = 0;
        }
        cnt = 1;
        gram = true;
        changed = true;
        rstart = r0 + 1;
    }
    wave_sync();
    for (int c0 = rstart; c0 < r1; c0 += 64) {
        const int rr = c0 + lane;
        const bool ok = rr < r1 && a.acc[rr];
        u64 act = __ballot(ok);
        if (!act) continue;
        const float my_inv = rr < r1 ? a.inv[rr] : 0.f;
        const u64 zn = __ballot(ok && my_inv != my_inv);
        if (!gram) {
            // the group as stored: inverse norms and the edges sim > boring_threshold among its tokens (:391-413)
            if (lane < cnt) {
                const float4 *p = (const float4 *)slot_tok(a, sl_src[lane], sl_prow[lane]);
                float s = 0.f;
                for (int v = 0; v < D4; ++v) s = dot4(p[v], p[v], s);
                sl_inv[lane] = inv_norm_of(s);
                sl_adj[lane] = 0;
            }
            wave_sync();
            const int np = cnt * (cnt - 1) / 2;
            for (int p = lane; p < np; p += 64) {
                int i = 0, q = p;
                while (q >= cnt - 1 - i) { q -= cnt - 1 - i; ++i; }
                const int j = i + 1 + q;
                const float4 *pi = (const float4 *)slot_tok(a, sl_src[i], sl_prow[i]);
                const float4 *pj = (const float4 *)slot_tok(a, sl_src[j], sl_prow[j]);
                float s = 0.f;
                for (int v = 0; v < D4; ++v) s = dot4(pi[v], pj[v], s);
                if (s * sl_inv[i] * sl_inv[j] > a.bthr) {
                    atomicOr((unsigned long long *)&sl_adj[i], 1ull << j);
                    atomicOr((unsigned long long *)&sl_adj[j], 1ull << i);
                }
            }
            wave_sync();
            gram = true;
        }
        while (act) {
            const int j = __builtin_ctzll(act);
            const bool any_edge = __ballot(lane < cnt && sl_adj[lane] != 0) != 0;
            if (cnt == cs && !any_edge && ((zn >> j) & 1)) {
                // a zero token into a full group without edges: slot 0 (argmin of all-NaN), no edge appears, forgetting keeps
                // every token — a run of such rows leaves only its last row in slot 0
                const u64 later = act & ~zn & (~0ull << j);
                const int lim = later ? __builtin_ctzll(later) : 64;
                const u64 run = act & zn & (lim == 64 ? ~0ull : ((1ull << lim) - 1));
                const int jl = 63 - __builtin_clzll(run);
                if (lane == 0) {
                    sl_src[0] = c0 + jl;
                    sl_dist[0] = a.cache_d[c0 + jl];
                    sl_inv[0] = __int_as_float(0x7fc00000);
                }
                changed = true;
                act &= ~run;
                wave_sync();
                continue;
            }
            act &= act - 1;
            const int32_t row = c0 + j;
            const float xi = __shfl(my_inv, j);
            const float xd = a.cache_d[row];
            // dots of the new token with every slot (:458-461 and the row of the Gram matrix it adds)
            float sim = __int_as_float(0x7fc00000);
            if (xi == xi) {
                const float4 *xr = (const float4 *)(a.cache_f + (int64_t)row * D);
                for (int v = lane; v < D4; v += 64) ((float4 *)xs)[v] = xr[v];
                wave_sync();
                if (lane < cnt) {
                    const float4 *p = (const float4 *)slot_tok(a, sl_src[lane], sl_prow[lane]);
                    float s = 0.f;
                    for (int v = 0; v < D4; ++v) s = dot4(p[v], ((const float4 *)xs)[v], s);
                    sim = s * sl_inv[lane] * xi;
                }
            }
            int slot;
            if (cnt < cs) {      // append (:452-456)
                slot = cnt;
                if (lane == 0) {
                    const int64_t pr = (int64_t)atomicAdd((u64 *)&a.dscal[DS_POOL_N], 1ull);
                    if (pr >= a.token_cap) a.dscal[DS_ERROR] = 2;
                    sl_prow[slot] = pr < a.token_cap ? (int32_t)pr : 0;
                }
                cnt++;
            } else {             // replace the least surprising slot: argmin of 1 - cos, first NaN first (:458-466)
                const float cd = 1.0f - sim;
                const u64 nanm = __ballot(lane < cnt && cd != cd);
                if (nanm) slot = __builtin_ctzll(nanm);
                else {
                    float m = lane < cnt ? cd : INFINITY;
                    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
                    slot = __builtin_ctzll(__ballot(lane < cnt && cd == m));
                }
            }
            const bool edge = lane < cnt && lane != slot && sim > a.bthr;
            const u64 emask = __ballot(edge);
            if (lane == slot) {
                sl_src[lane] = row;
                sl_dist[lane] = xd;
                sl_inv[lane] = xi;
                sl_adj[lane] = emask;
            } else if (lane < cnt) {
                sl_adj[lane] = (sl_adj[lane] & ~(1ull << slot)) | ((u64)edge << slot);
            }
            changed = true;
            wave_sync();
            // forgetting (:386-446): components by a Warshall closure of the bit masks
            if (cnt < 2) continue;
            u64 m = lane < cnt ? (sl_adj[lane] | (1ull << lane)) : 0;
            if (__ballot(lane < cnt && sl_adj[lane] != 0) == 0) continue;
            for (int k = 0; k < cnt; ++k) {
                const u64 mk = shfl_u64(m, k);
                if ((m >> k) & 1) m |= mk;
            }
            const int rep = lane < cnt ? __builtin_ctzll(m) : -1;
            const u64 repmask = __ballot(rep == lane);
            const u64 mergemask = __ballot(rep == lane && __builtin_popcountll(m) > 1);
            // means of the merged components into the pool row of their smallest slot (:427-436)
            u64 mm = mergemask;
            while (mm) {
                const int c = __builtin_ctzll(mm);
                mm &= mm - 1;
                const u64 mem = shfl_u64(m, c);
                const int nmem = __builtin_popcountll(mem);
                const int32_t dst = sl_prow[c];
                float sq = 0.f;
                for (int v = lane; v < D4; v += 64) {
                    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (u64 b = mem; b; b &= b - 1) {
                        const int k = __builtin_ctzll(b);
                        const float4 t = ((const float4 *)slot_tok(a, sl_src[k], sl_prow[k]))[v];
                        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
                    }
                    const float fn = (float)nmem;
                    s.x /= fn; s.y /= fn; s.z /= fn; s.w /= fn;
                    ((float4 *)(a.pool + (int64_t)dst * D))[v] = s;
                    sq = dot4(s, s, sq);
                }
                sq = wave_sum(sq);
                double dsum = 0.0;
                for (u64 b = mem; b; b &= b - 1) dsum += (double)sl_dist[__builtin_ctzll(b)];
                wave_sync();
                if (lane == 0) {
                    sl_src[c] = -1;
                    sl_dist[c] = (float)(dsum / nmem);
                    sl_inv[c] = inv_norm_of(sq);
                }
                wave_sync();
            }
            __threadfence_block();   // the means are read back by other lanes below
            // compaction: one slot per component, in the order of its smallest index (:416-421)
            if (rep == lane) {
                const int pos = __builtin_popcountll(repmask & ((1ull << lane) - 1));
                t_prow[pos] = sl_prow[lane];
                t_src[pos] = sl_src[lane];
                t_dist[pos] = sl_dist[lane];
                t_inv[pos] = sl_inv[lane];
            }
            const int ncnt = __builtin_popcountll(repmask);
            const u64 newmerged = __ballot(rep == lane && __builtin_popcountll(m) > 1);
            // positions of the merged slots after compaction
            u64 newm = 0;
            for (u64 b = newmerged; b; b &= b - 1) {
                const int k = __builtin_ctzll(b);
                newm |= 1ull << __builtin_popcountll(repmask & ((1ull << k) - 1));
            }
            wave_sync();
            if (lane < ncnt) {
                sl_prow[lane] = t_prow[lane];
                sl_src[lane] = t_src[lane];
                sl_dist[lane] = t_dist[lane];
                sl_inv[lane] = t_inv[lane];
                sl_adj[lane] = 0;   // a singleton had no edge; the merged tokens' edges follow
            }
            cnt = ncnt;
            wave_sync();
            for (u64 b = newm; b; b &= b - 1) {
                const int k = __builtin_ctzll(b);
                const float4 *xr = (const float4 *)slot_tok(a, sl_src[k], sl_prow[k]);
                for (int v = lane; v < D4; v += 64) ((float4 *)xs)[v] = xr[v];
                wave_sync();
                bool ed = false;
                if (lane < cnt && lane != k) {
                    const float4 *p = (const float4 *)slot_tok(a, sl_src[lane], sl_prow[lane]);
                    float s = 0.f;
                    for (int v = 0; v < D4; ++v) s = dot4(p[v], ((const float4 *)xs)[v], s);
                    ed = s * sl_inv[lane] * sl_inv[k] > a.bthr;
                }
                const u64 em = __ballot(ed);
                if (lane == k) sl_adj[lane] |= em;
                else if (ed) sl_adj[lane] |= 1ull << k;
                wave_sync();
            }
        }
    }
    if (!changed) return;
    // cache rows still pending go to their slot's pool row once; distances, rows and count of the group
    for (int k = 0; k < cnt; ++k) {
        const int32_t src = sl_src[k];
        if (src < 0) continue;
        const float4 *xr = (const float4 *)(a.cache_f + (int64_t)src * D);
        float4 *dst = (float4 *)(a.pool + (int64_t)sl_prow[k] * D);
        for (int v = lane; v < D4; v += 64) dst[v] = xr[v];
    }
    if (lane < cnt) {
        a.pool_d[sl_prow[lane]] = sl_dist[lane];
        a.store_rows[(int64_t)e * cs + lane] = sl_prow[lane];
    }
    if (lane == 0) a.store_cnt[e] = cnt;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// k_surp_task's dynamic LDS: pool rows and inverse norms of the neighbour tokens, one token
static size_t surp_task_lds(int radius, int cs, int D)
{
    const int w = 2 * radius + 1;
    return sizeof(float) * (2 * (size_t)(w * w * w - 1) * cs + D);
}

bsc_status surprise_check_args(const bsc_ctx *x, const char *who, int32_t radius, double sthr, double bthr)
{
    if (radius < 0 || radius > SURP_RMAX) {
        bsc_set_error("%s: neighbor_radius %d outside [0, %d]", who, radius, SURP_RMAX);
        return BSC_E_INVALID;
    }
    if (sthr != sthr || bthr != bthr) {
        bsc_set_error("%s: NaN threshold", who);
        return BSC_E_INVALID;
    }
    const int cs = x->c.cache_size;
    const size_t lds = surp_task_lds(radius, cs, x->c.token_dim);
    if (cs > 64 || lds > SURP_TASK_LDS) {
        bsc_set_error("%s: cache_size %d with radius %d needs %zu bytes of LDS (limit %d; cache_size <= 64)", who, cs, radius, lds,
                      SURP_TASK_LDS);
        return BSC_E_INVALID;
    }
    return BSC_OK;
}

bsc_status surprise_flush(bsc_ctx *x, int32_t radius, double sthr, double bthr)
{
    const int n = x->c.iter_size, D = x->c.token_dim, cs = x->c.cache_size, vcap = x->c.voxel_capacity;
    const int w = 2 * radius + 1, K = w * w * w;
    hipStream_t s = x->stream;
    BSC_TRY(surprise_check_args(x, "bsc_flush_surprise", radius, sthr, bthr));
    const size_t lds = surp_task_lds(radius, cs, D);
    BSC_TRY(ws_ensure(x, K));
    SurpriseWs *ws = x->surp;
    // at most one new pool row per cache row: dead rows reclaimed / the pool grown before anything changes (as flush_cache)
    BSC_TRY(reserve_pool_rows(x, n));
    const dim3 block(TPB), grid((n + TPB - 1) / TPB), wgrid((unsigned)(((int64_t)n * 64 + TPB - 1) / TPB));
    hipLaunchKernelGGL(k_surp_rows, grid, block, 0, s, n, x->cache_pos, x->occ, x->c.grid_size, x->nh, vcap, ws->ent, ws->head);
    hipLaunchKernelGGL(k_surp_rowinv, wgrid, block, 0, s, n, x->cache_f, D, ws->inv);
    BSC_TRY(prim_exclusive_sum_i32(lane_main(x), ws->head, ws->tid, (size_t)n));
    BSC_HIP(hipMemsetAsync(ws->cid, 0x7f, sizeof(int32_t) * ((size_t)vcap + 1), s));
    hipLaunchKernelGGL(k_surp_tasks, grid, block, 0, s, n, ws->ent, ws->head, ws->tid, ws->tstart, ws->tent, ws->cid, ws->scal);
    hipLaunchKernelGGL(k_surp_first, grid, block, 0, s, n, ws->ent, ws->head, ws->tid, ws->cid, ws->first);
    BSC_TRY(prim_exclusive_sum_i32(lane_main(x), ws->first, ws->dense, (size_t)n));
    hipLaunchKernelGGL(k_surp_dense, grid, block, 0, s, n, ws->ent, ws->first, ws->dense, ws->cid, ws->scal);
    int32_t hs[3] = {0, 0, 0};
    BSC_HIP(hipMemcpyAsync(hs, ws->scal, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, s));
    BSC_HIP(hipStreamSynchronize(s));
    const int n_tasks = hs[0], n_u = hs[1];
    hipLaunchKernelGGL(k_surp_nbrs, dim3((unsigned)(((int64_t)n * K + TPB - 1) / TPB)), block, 0, s, n, radius, x->cache_pos,
                       ws->head, ws->tid, x->occ, ws->cid, x->c.grid_size, x->nh, vcap, n_u, ws->nb);
    BSC_HIP(hipMemsetAsync(ws->lcnt, 0, sizeof(int32_t) * ((size_t)n + 2), s));
    if (n_tasks < 65535 && n_u <= SURP_TAB16)
        hipLaunchKernelGGL((k_surp_levels<uint16_t, SURP_TAB16>), dim3(1), dim3(64), 0, s, n_u, n_tasks, K, ws->nb, ws->lvl,
                           ws->lcnt, ws->scal);
    else if (n_u <= SURP_TAB32)
        hipLaunchKernelGGL((k_surp_levels<uint32_t, SURP_TAB32>), dim3(1), dim3(64), 0, s, n_u, n_tasks, K, ws->nb, ws->lvl,
                           ws->lcnt, ws->scal);
    else {
        if (!ws->lvtab) BSC_TRY(mem_alloc(x->mem, (void **)&ws->lvtab, sizeof(int32_t) * (size_t)n, "surprise flush level table"));
        hipLaunchKernelGGL(k_surp_levels_global, dim3(1), dim3(64), 0, s, ws->lvtab, n_u, n_tasks, K, ws->nb, ws->lvl, ws->lcnt,
                           ws->scal);
    }
    BSC_HIP(hipGetLastError());
    BSC_HIP(hipMemcpyAsync(hs + 2, ws->scal + 2, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BSC_HIP(hipStreamSynchronize(s));
    const int n_lev = hs[2];
    int32_t *cnt = (int32_t *)malloc(sizeof(int32_t) * (n_lev + 2));
    int32_t *off = (int32_t *)malloc(sizeof(int32_t) * (n_lev + 2));
    hipError_t he = hipMemcpy(cnt, ws->lcnt, sizeof(int32_t) * (n_lev + 1), hipMemcpyDeviceToHost);
    off[0] = 0;
    for (int l = 0; l <= n_lev; ++l) off[l + 1] = off[l] + cnt[l];
    if (he == hipSuccess) he = hipMemcpy(ws->loff, off, sizeof(int32_t) * (n_lev + 1), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemsetAsync(ws->lcnt, 0, sizeof(int32_t) * (n_lev + 1), s);
    if (he != hipSuccess) { free(cnt); free(off); BSC_HIP(he); }
    if (n_tasks > 0)
        hipLaunchKernelGGL(k_surp_scatter, dim3((n_tasks + TPB - 1) / TPB), block, 0, s, n_tasks, ws->lvl, ws->loff, ws->lcnt,
                           ws->order);
    SurpArgs a;
    a.tstart = ws->tstart; a.tent = ws->tent;
    a.cache_pos = x->cache_pos; a.occ = x->occ;
    a.cache_f = x->cache_f; a.cache_d = x->cache_d; a.inv = ws->inv; a.acc = ws->acc;
    a.store_rows = x->store_rows; a.store_cnt = x->store_cnt; a.pool = x->pool; a.pool_d = x->pool_d;
    a.dscal = x->dscal; a.token_cap = x->c.token_capacity;
    a.gs = x->c.grid_size; a.nh = x->nh; a.vcap = vcap; a.cs = cs; a.D = D; a.r = radius;
    a.sthr = sthr; a.bthr = (float)bthr;   // :408 compares an f32 matrix with the threshold in f32
    for (int l = 1; l <= n_lev; ++l) {
        if (!cnt[l]) continue;
        a.order = ws->order + off[l];
        hipLaunchKernelGGL(k_surp_task, dim3((unsigned)cnt[l]), block, lds, s, a);
    }
    free(cnt);
    free(off);
    BSC_HIP(hipGetLastError());
    // the live rows (sum of the groups' counts) ride in the readback below: merges leave pool rows behind that nothing refers to
    BSC_TRY(enqueue_store_totals(x));
    BSC_TRY(read_scalars(x));
    if (x->hscal[DS_ERROR]) {
        bsc_set_error("capacity exceeded during the surprise flush (code %lld; token_capacity=%lld)", (long long)x->hscal[DS_ERROR],
                      (long long)x->c.token_capacity);
        return BSC_E_CAPACITY;
    }
    // _reinit_cache (memory_2.py:536 -> :724-729)
    BSC_HIP(hipMemsetAsync(x->cache_f, 0, sizeof(float) * (size_t)n * D, s));
    BSC_HIP(hipMemsetAsync(x->cache_pos, 0, sizeof(int32_t) * (size_t)n * 3, s));
    BSC_HIP(hipMemsetAsync(x->cache_d, 0, sizeof(float) * (size_t)n, s));
    BSC_HIP(hipGetLastError());
    x->iter_id = 0;
    x->n_flush++;
    x->names_dirty = true; x->row_scale_dirty = true;
    x->pool_n_host = x->hscal[DS_POOL_N];
    // more dead rows than live ones: move the live rows down (at most `live` moves after at least `live` allocations)
    const int64_t live = x->hscal[DS_TMP1];
    // The flush is complete at this point and the compaction is optional: when it cannot run (its scratch could not be
    // allocated) the pool stays as it is — nothing was moved — and the flush still succeeds; the error text names the cause.
    if (x->pool_n_host > 2 * live && store_compact_auto()) (void)compact_store_impl(x, live, nullptr, nullptr);
    return BSC_OK;
}

// counterpart of bsc_export_cache: rows 0 .. n-1 of the cache and iter_id; the other rows are zero as after _reinit_cache
bsc_status import_cache_impl(bsc_ctx *x, int64_t n, const int32_t *pos, const float *feat, const float *dis)
{
    const int64_t D = x->c.token_dim, N = x->c.iter_size, gs = x->c.grid_size;
    if (n < 0 || n > N || (n > 0 && (!pos || !feat || !dis))) {
        bsc_set_error("bsc_import_cache: %lld rows for a cache of %lld", (long long)n, (long long)N);
        return BSC_E_INVALID;
    }
    int32_t *occ = (int32_t *)malloc(sizeof(int32_t) * x->ncell);
    hipError_t e = hipStreamSynchronize(x->stream);
    if (e == hipSuccess) e = hipMemcpy(occ, x->occ, sizeof(int32_t) * x->ncell, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(occ); BSC_HIP(e); }
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = pos[3 * i], c = pos[3 * i + 1], h = pos[3 * i + 2];
        const bool zero = r == 0 && c == 0 && h == 0;
        const bool in = r >= 0 && c >= 0 && h >= 0 && r < gs && c < gs && h < x->nh;
        if (!zero && (!in || occ[(r * gs + c) * x->nh + h] < 0)) {
            free(occ);
            bsc_set_error("bsc_import_cache: row %lld at [%d, %d, %d] has no voxel", (long long)i, r, c, h);
            return BSC_E_INVALID;
        }
    }
    free(occ);
    hipStream_t s = x->stream;
    BSC_HIP(hipMemsetAsync(x->cache_f, 0, sizeof(float) * (size_t)N * D, s));
    BSC_HIP(hipMemsetAsync(x->cache_pos, 0, sizeof(int32_t) * (size_t)N * 3, s));
    BSC_HIP(hipMemsetAsync(x->cache_d, 0, sizeof(float) * (size_t)N, s));
    if (n > 0) {
        BSC_HIP(hipMemcpyAsync(x->cache_f, feat, sizeof(float) * (size_t)n * D, hipMemcpyHostToDevice, s));
        BSC_HIP(hipMemcpyAsync(x->cache_pos, pos, sizeof(int32_t) * (size_t)n * 3, hipMemcpyHostToDevice, s));
        BSC_HIP(hipMemcpyAsync(x->cache_d, dis, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    BSC_HIP(hipStreamSynchronize(s));
    x->iter_id = n;
    return BSC_OK;
}
