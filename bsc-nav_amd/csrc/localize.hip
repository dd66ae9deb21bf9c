// localize.hip — voxel_localized (memory_2.py:563-671) around the cosine scan (cosine_scan.hip): query pooling before it; after it
// the per-voxel max and the stable top-K in HDF5 group-name order.
//
//   k_pool_query   Gaussian centre-weighted pooling of (B,T,D) query tokens -> (D)          (:591-608)
//   k_name_keys    HDF5 link-name order of the stored voxels -> name ranks, rebuilt when the set of voxels changed
//   VoxelView      the store as the candidate kernels see it; CandArgs / RegionCandArgs: the two candidate lists built on it
//   k_candidates   per voxel: region / floor filters, max over its <= cache_size tokens, 64-bit
//                  rank key (similarity descending, then name order)                         (:624-663)
//   k_block_topk   rounds of per-1024 bitonic selections (large sets: behind a sample threshold and k_cand_filter) shrink the
//                  candidates to the K smallest rank keys = the reference's stable-sort top-K (device-wide radix sort only for
//                  K > 512)                                                                   (:665-667)
//   k_region_*     bsc_localize_regions (end of this file): a sphere and floor band per query (BSCAgent.py:630-647,1078-1098),
//                  visibility pass, compaction + gather of the visible rows, the scan over those rows only
#include "bsc_internal.h"
#include "localize_cand.h"

#include <math.h>
#include <type_traits>

#define TPB 256

// ---- HDF5 link-name order of "grid_{r}_{c}_{h}" --------------------------------------------------
// Bytewise string order: digits sort before '_' (0x5f), end-of-string before digits.  Each number is
// written as 6 left-aligned base-11 symbols; non-final fields pad with 10 (after every digit), the final
// field shifts digits to 1..10 and pads with 0.
#define NAME_DIGITS 6
__host__ __device__ static inline u64 name_field(int32_t v, bool last)
{
    int dig[12];
    int n = 0;
    if (v == 0) dig[n++] = 0;
    while (v > 0) { dig[n++] = v % 10; v /= 10; }
    u64 k = 0;
    for (int i = 0; i < NAME_DIGITS; ++i) {
        int sym = (i < n) ? dig[n - 1 - i] + (last ? 1 : 0) : (last ? 0 : 10);
        k = k * 11 + (u64)sym;
    }
    return k;
}
__host__ __device__ static inline u64 name_key(int32_t r, int32_t c, int32_t h)
{
    const u64 B = 1771561ull;   // 11^6
    return (name_field(r, false) * B + name_field(c, false)) * B + name_field(h, true);
}

// memory_2.py:591-608.  One thread per feature d; weights recomputed in f32 like the torch expression.
__global__ __launch_bounds__(TPB) void k_pool_query(const float *__restrict__ tokens, int B, int T, int D,
                                                    float *__restrict__ out)
{
    const int d = blockIdx.x * TPB + threadIdx.x;
    if (d >= D) return;
    const int g = (int)sqrtf((float)T);
    const float center = (float)((g - 1) / 2.0);
    const float sigma = (float)((g / 2.0) * (g / 2.0));
    float wsum = 0.f;
    for (int t = 0; t < T; ++t) {
        const float xs = (float)(t % g) - center, ys = (float)(t / g) - center;
        wsum += expf(-(xs * xs + ys * ys) / (2 * sigma));
    }
    float total = 0.f;
    for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) {
            const float xs = (float)(t % g) - center, ys = (float)(t / g) - center;
            const float w = expf(-(xs * xs + ys * ys) / (2 * sigma)) / wsum;
            s += tokens[((int64_t)b * T + t) * D + d] * w;
        }
        total += s;
    }
    out[d] = total / (float)B;
}

// candidate c in [0, n_cand): c < max_id is voxel id c, c == max_id is the grid_0_0_0 group (entry vcap)
__global__ __launch_bounds__(TPB) void k_name_keys(int n_cand, int max_id, int vcap, const int32_t *__restrict__ rgb_pos,
                                                   const int32_t *__restrict__ cnt, u64 *__restrict__ keys,
                                                   uint32_t *__restrict__ vals)
{
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= n_cand) return;
    const int e = (c == max_id) ? vcap : c;
    u64 k = ~0ull;
    if (cnt[e] > 0) k = (c == max_id) ? name_key(0, 0, 0) : name_key(rgb_pos[3 * e], rgb_pos[3 * e + 1], rgb_pos[3 * e + 2]);
    keys[c] = k;
    vals[c] = (uint32_t)c;
}

__global__ __launch_bounds__(TPB) void k_name_rank(int n_cand, const uint32_t *__restrict__ sorted_vals,
                                                   uint32_t *__restrict__ rank)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n_cand) return;
    rank[sorted_vals[i]] = (uint32_t)i;
}

// ---- the candidates of the selection (VoxelView, RegionDev, CandArgs / RegionCandArgs: localize_cand.h) --------------------------
// what the context's store holds now (read_scalars first): the view, and through the pointers the candidates (max_id + 1) and the
// matrix the scan reads
static VoxelView store_view(const bsc_ctx *x, int *n_cand, int64_t *n_rows, const float **rows)
{
    const bool exact = x->c.mode == BSC_MODE_EXACT;
    VoxelView v;
    v.max_id = (int)x->hscal[DS_MAX_ID]; v.vcap = x->c.voxel_capacity; v.cache_size = x->c.cache_size; v.exact = exact ? 1 : 0;
    v.rgb_pos = x->rgb_pos; v.cnt = exact ? x->store_cnt : x->acnt; v.store_rows = x->store_rows; v.name_rank = x->l_name_rank;
    *n_cand = v.max_id + 1;
    *n_rows = exact ? x->hscal[DS_POOL_N] : v.max_id;
    *rows = exact ? x->pool : x->acc;
    return v;
}

static RegionDev region_dev(double radius, const int32_t *curr, int32_t floor_lo, int32_t floor_hi)
{
    return RegionDev{radius * radius, curr ? curr[0] : 0, curr ? curr[1] : 0, curr ? curr[2] : 0, floor_lo, floor_hi, radius >= 0 ? 1 : 0};
}

static CandArgs cand_args(const VoxelView &v, int n_cand, const RegionDev &region) { return CandArgs{v, n_cand, region}; }
// every voxel for every query
static CandArgs cand_args_open(const VoxelView &v, int n_cand) { return cand_args(v, n_cand, region_dev(-1.0, nullptr, 0, -1)); }

__device__ __forceinline__ uint32_t cand_val(const CandArgs &, int c) { return (uint32_t)c; }
__device__ __forceinline__ uint32_t cand_rank(const CandArgs &a, int c) { return a.name_rank[c]; }
__device__ __forceinline__ uint32_t cand_simkey(const CandArgs &a, int c, int, const float *__restrict__ sims)
{
    if (c >= a.n_cand) return 0xffffffffu;
    const int e = a.entry(c);
    const int m = a.cnt[e];
    if (m <= 0) return 0xffffffffu;
    if (!region_open(a.region)) {
        int r, cc, h;
        a.position(c, r, cc, h);
        if (!region_sees(a.region, r, cc, h)) return 0xffffffffu;
    }
    return simkey_of(a.best_sim(e, m, sims));
}

__device__ __forceinline__ uint32_t cand_rank(const RegionCandArgs &a, int i) { return a.name_rank[cand_val(a, i)]; }
__device__ __forceinline__ uint32_t cand_simkey(const RegionCandArgs &a, int i, int q, const float *__restrict__ sims)
{
    float best;
    return cand_score(a, i, q, sims, best) ? simkey_of(best) : 0xffffffffu;
}

// full rank key: similarity descending, ties in HDF5 name order
template <class A>
__device__ __forceinline__ u64 cand_key(const A &a, int c, int q, const float *__restrict__ sims)
{
    const uint32_t sk = cand_simkey(a, c, q, sims);
    if (sk == 0xffffffffu) return ~0ull;
    return ((u64)sk << 32) | (u64)cand_rank(a, c);
}

template <class A>
__global__ __launch_bounds__(TPB) void k_candidates(A a, int q, const float *__restrict__ sims, u64 *__restrict__ keys,
                                                    uint32_t *__restrict__ vals)
{
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= a.n_cand) return;
    keys[c] = cand_key(a, c, q, sims);
    vals[c] = cand_val(a, c);
}

__global__ __launch_bounds__(TPB) void k_gather_topk(int K, int n_cand, int max_id, int vcap,
                                                     const u64 *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                     int64_t in_stride, const int32_t *__restrict__ rgb_pos,
                                                     int32_t *__restrict__ out_pos, float *__restrict__ out_sim)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= K) return;
    keys += (int64_t)blockIdx.y * in_stride;
    vals += (int64_t)blockIdx.y * in_stride;
    out_pos += (int64_t)blockIdx.y * K * 3;
    out_sim += (int64_t)blockIdx.y * K;
    int32_t r = -1, c = -1, h = -1;
    float s = -INFINITY;
    if (i < n_cand && keys[i] != ~0ull) {
        const uint32_t cand = vals[i];
        if ((int)cand != max_id) { r = rgb_pos[3 * cand]; c = rgb_pos[3 * cand + 1]; h = rgb_pos[3 * cand + 2]; }
        else { r = 0; c = 0; h = 0; }
        uint32_t u = ~(uint32_t)(keys[i] >> 32);
        u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
        s = __uint_as_float(u);
    }
    out_pos[3 * i] = r; out_pos[3 * i + 1] = c; out_pos[3 * i + 2] = h;
    out_sim[i] = s;
}

// K smallest rank keys of each 1024-element slice: bitonic sort in LDS (keys are unique: similarity key | name rank).
// Rounds of this kernel shrink n candidates to K without a device-wide sort: n -> ceil(n/1024)*K -> ... -> K.
#define TK_N 1024
#define SEL_CNT_PAD 32          // int32 slots between the survivor counters of consecutive queries (one 128-byte line each)
// Ascending bitonic sort of 1024 (key, value) pairs held 4 per thread (element e = 256 r + tid in slot r).  A compare-exchange
// distance j >= 256 pairs two slots of one thread, j < 64 two lanes of one wavefront (shuffles), only j = 64 and 128 cross
// wavefronts and go through LDS: 7 of the 55 steps, one barrier each (two buffers alternate), instead of a barrier after every
// step of an all-LDS network (round 3: ~40 us per block sort, most of it barriers).
__device__ __forceinline__ void kv_cx(u64 &k, uint32_t &v, const u64 pk, const uint32_t pv, const bool take_min)
{
    const bool swap = take_min ? (pk < k) : (pk > k);
    k = swap ? pk : k;
    v = swap ? pv : v;
}

// value of lane (lane ^ j), j < 64, without the LDS crossbar: DPP quad permutes / row mirrors below 16 (xor 4 = reverse of 8, then
// of each quad; xor 8 = reverse of 16, then of each 8), v_permlane16_swap / v_permlane32_swap above.  As ds_bpermute a 1024-key sort
// issued 2 160 wavefront-wide permutes at ~32 cycles of the CU's LDS pipe each: 33 us per sort and CU, whatever else ran beside it.
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, int j, int lane)
{
    if (j == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);           // quad_perm [1,0,3,2]
    if (j == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);           // quad_perm [2,3,0,1]
    if (j == 4) {
        const int t = __builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true);                     // row_half_mirror
        return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x1B, 0xf, 0xf, true);                        // quad_perm [3,2,1,0]
    }
    if (j == 8) {
        const int t = __builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, true);                     // row_mirror
        return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x141, 0xf, 0xf, true);                       // row_half_mirror
    }
    if (j == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (lane & 16) ? r[0] : r[1];
    }
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);                           // j == 32
    return (lane & 32) ? r[0] : r[1];
}

__device__ __forceinline__ void bitonic_1024_regs(u64 (&key)[4], uint32_t (&val)[4], u64 (*bk)[TK_N], uint32_t (*bv)[TK_N])
{
    const int tid = threadIdx.x;
    int buf = 0;
#pragma unroll
    for (int k = 2; k <= TK_N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 256) {                             // partner slot r ^ (j / 256) of the same thread
                const int dr = j >> 8;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r & dr) continue;
                    const int e = r * 256 + tid;
                    const bool up = (e & k) == 0;       // the lower element of the pair keeps the minimum when the run ascends
                    const bool sw = (key[r] > key[r | dr]) == up;
                    const u64 ka = key[r], kb = key[r | dr];
                    const uint32_t va = val[r], vb = val[r | dr];
                    key[r] = sw ? kb : ka; key[r | dr] = sw ? ka : kb;
                    val[r] = sw ? vb : va; val[r | dr] = sw ? va : vb;
                }
            } else if (j < 64) {                        // partner lane tid ^ j of the same wavefront
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = r * 256 + tid;
                    const u64 pk = (u64)lane_xor((uint32_t)key[r], j, tid) | ((u64)lane_xor((uint32_t)(key[r] >> 32), j, tid) << 32);
                    const uint32_t pv = lane_xor(val[r], j, tid);
                    kv_cx(key[r], val[r], pk, pv, ((e & j) == 0) == ((e & k) == 0));
                }
            } else {                                    // j = 64, 128: another wavefront, through LDS
#pragma unroll
                for (int r = 0; r < 4; ++r) { bk[buf][r * 256 + tid] = key[r]; bv[buf][r * 256 + tid] = val[r]; }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = r * 256 + tid;
                    kv_cx(key[r], val[r], bk[buf][e ^ j], bv[buf][e ^ j], ((e & j) == 0) == ((e & k) == 0));
                }
                buf ^= 1;                               // the next cross-wavefront step writes the other buffer: one barrier per step
            }
        }
    }
}

// the K smallest of a sorted slice (element 256 r + tid in slot r) -> the K winner slots at out_keys / out_vals
__device__ __forceinline__ void store_winners(const u64 (&key)[4], const uint32_t (&val)[4], int K, u64 *__restrict__ out_keys,
                                              uint32_t *__restrict__ out_vals)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = r * 256 + (int)threadIdx.x;
        if (e < K) {
            out_keys[e] = key[r];
            out_vals[e] = val[r];
        }
    }
}

// first round, fused with the candidate scan: block (b, q) ranks candidates [1024 b, 1024 b + 1024) of query q
template <class A>
__global__ __launch_bounds__(TPB) void k_cand_topk(A a, const float *__restrict__ sims, int64_t sims_stride, int K,
                                                   u64 *__restrict__ out_keys, uint32_t *__restrict__ out_vals,
                                                   int64_t out_stride, int nb, int nq, int bstride)
{
    __shared__ u64 bk[2][TK_N];
    __shared__ uint32_t bv[2][TK_N];
    for (int wi = blockIdx.x; wi < nb * nq; wi += gridDim.x) {      // persistent: (block, query) items
        const int q = wi / nb, bx = wi - q * nb;
        const float *qs = sims + (int64_t)q * sims_stride;
        u64 key[4];
        uint32_t val[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = bx * bstride * TK_N + r * 256 + (int)threadIdx.x;     // bstride > 1: a sample of blocks spread over the whole map
            key[r] = cand_key(a, c, q, qs);
            val[r] = cand_val(a, c);
        }
        __syncthreads();                                            // the previous item's partner reads are done
        bitonic_1024_regs(key, val, bk, bv);
        store_winners(key, val, K, out_keys + (int64_t)q * out_stride + (int64_t)bx * K, out_vals + (int64_t)q * out_stride + (int64_t)bx * K);
    }
}

__global__ __launch_bounds__(TPB) void k_block_topk(const u64 *__restrict__ in_keys, const uint32_t *__restrict__ in_vals,
                                                    int64_t n, const int32_t *__restrict__ n_per_q, int64_t in_stride, int K,
                                                    u64 *__restrict__ out_keys, uint32_t *__restrict__ out_vals,
                                                    int64_t out_stride, int nb, int nq)
{
    __shared__ u64 bk[2][TK_N];
    __shared__ uint32_t bv[2][TK_N];
    for (int wi = blockIdx.x; wi < nb * nq; wi += gridDim.x) {      // persistent: (block, query) items
        // the query is the FAST index: the non-empty slices of the survivor lists (the first ~7 of every query's 32) are then the
        // first items and spread over all CUs — with the slice as the fast index they sat in every fourth workgroup of an XCD,
        // i.e. on a quarter of its CUs, 16 sorts deep (first survivor round 258 us)
        const int bx = wi / nq, q = wi - bx * nq;
        const int64_t nn = n_per_q ? min((int64_t)n_per_q[q * SEL_CNT_PAD], n) : n;
        const int64_t base = (int64_t)bx * TK_N;
        if (base >= nn) {
            // nothing in this slice (survivor lists are sized for the worst case: ~6 400 of 32 768 slots hold a candidate at K = 100,
            // so 25 of a query's 32 first-round slices are empty): no sort, K empty winners
            for (int e = (int)threadIdx.x; e < K; e += TPB) {
                out_keys[(int64_t)q * out_stride + (int64_t)bx * K + e] = ~0ull;
                out_vals[(int64_t)q * out_stride + (int64_t)bx * K + e] = 0u;
            }
            continue;
        }
        u64 key[4];
        uint32_t val[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t g = base + r * 256 + (int)threadIdx.x;
            key[r] = g < nn ? in_keys[(int64_t)q * in_stride + g] : ~0ull;
            val[r] = g < nn ? in_vals[(int64_t)q * in_stride + g] : 0u;
        }
        __syncthreads();
        bitonic_1024_regs(key, val, bk, bv);
        store_winners(key, val, K, out_keys + (int64_t)q * out_stride + (int64_t)bx * K, out_vals + (int64_t)q * out_stride + (int64_t)bx * K);
    }
}

// (persistent 1-D grid: 16 k workgroups walking the (query, chunk) items measured 2x faster than one short-lived
//  workgroup per item, see profiles/README.md)
// threshold filter: the K-th best key of a SAMPLE of the candidates bounds the K-th best of all of them from above,
// so only candidates at least that good can be in the answer; they are appended (unordered) to a short survivor list
#define FILT_PER_BLOCK 4096
#define FILT_G (FILT_PER_BLOCK / (4 * TPB))
// bit c of the map: candidate c (a dense row) holds points.  The filter reads a query's similarities once and, per 16 of them, two
// bytes of this map instead of 64 bytes of counts.
__global__ __launch_bounds__(TPB) void k_valid_bits(const int32_t *__restrict__ cnt, int n, uint32_t *__restrict__ bits)
{
    const int c = blockIdx.x * TPB + threadIdx.x;
    const u64 b = __ballot(c < n && cnt[c < n ? c : 0] > 0);
    if ((threadIdx.x & 63) == 0) *(u64 *)(bits + 2 * (c >> 6)) = b;
}
template <bool FAST, class A>      // FAST: dense map, no region / floor filter — candidate c is row c, validity from the bitmap (zero past max_id)
__global__ __launch_bounds__(TPB) void k_cand_filter(A a, const float *__restrict__ sims, int64_t sims_stride,
                                                     const u64 *__restrict__ thr_keys, int K, int cap,
                                                     u64 *__restrict__ out_keys, uint32_t *__restrict__ out_vals,
                                                     int32_t *__restrict__ counts, int nbf, int nq, const uint32_t *__restrict__ valid)
{
  for (int wi = blockIdx.x; wi < nbf * nq; wi += gridDim.x) {
    const int q = wi / nbf, bx = wi - q * nbf;
    const u64 thr = thr_keys[q];
    const uint32_t thr_hi = (uint32_t)(thr >> 32);
    const float *qs = sims + (int64_t)q * sims_stride;
    const int lane = threadIdx.x & 63;
    uint32_t sk[FILT_G][4];
    // phase 1: every load of the block's 4096 candidates is in flight before anything is consumed
#pragma unroll
    for (int g = 0; g < FILT_G; ++g) {
        const int c0 = bx * FILT_PER_BLOCK + g * 4 * TPB + threadIdx.x * 4;
        if constexpr (FAST) {
            // (a group of four that reaches past max_id — the map's tail, max_id rounded up to 4 — reads nothing: its bits count as zero;
            //  inside the last word the bits past max_id ARE zero)
            const bool in = c0 < a.max_id;
            const float4 sv = in ? *(const float4 *)(qs + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            const uint32_t vb = in ? valid[c0 >> 5] >> (c0 & 31) : 0u;  // c0 is a multiple of 4: its four bits sit in one word
            sk[g][0] = (vb & 1u) ? float_desc_key(sv.x) : 0xffffffffu;
            sk[g][1] = (vb & 2u) ? float_desc_key(sv.y) : 0xffffffffu;
            sk[g][2] = (vb & 4u) ? float_desc_key(sv.z) : 0xffffffffu;
            sk[g][3] = (vb & 8u) ? float_desc_key(sv.w) : 0xffffffffu;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) sk[g][k] = cand_simkey(a, c0 + k, q, qs);
        }
    }
    // phase 2: which of the lane's 16 candidates survive (the name rank breaks ties with the threshold's similarity bits)
    uint32_t keepbits = 0u;
#pragma unroll
    for (int g = 0; g < FILT_G; ++g) {
        const int c0 = bx * FILT_PER_BLOCK + g * 4 * TPB + threadIdx.x * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool keep = sk[g][k] != 0xffffffffu && sk[g][k] <= thr_hi;
            if (keep && sk[g][k] == thr_hi) keep = (((u64)sk[g][k] << 32) | (u64)cand_rank(a, c0 + k)) <= thr;
            keepbits |= keep ? (1u << (g * 4 + k)) : 0u;
        }
    }
    // phase 3: ONE atomic per wavefront with survivors (the counters of the queries sit a cache line apart: with one counter
    // per survivor on 16 shared lines this kernel spent 1.1 ms of its 1.2 ms queueing at the L2 atomic units)
    const int mine = __popc(keepbits);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const int total = __shfl(incl, 63);
    // ONE atomic per work item (4096 candidates): the four wavefronts' totals meet in LDS.  Atomics on one address are served one
    // at a time by the L2 (~0.4 us each with the returned value): with an atomic per wavefront a query's counter took 1024 of them in
    // a row — that, not the 1.07 GB it reads, was this kernel's 0.46 ms
    __shared__ int s_tot[TPB / 64], s_base;
    const int wv = threadIdx.x >> 6;
    __syncthreads();                                    // the previous item's readers of s_tot / s_base are done
    if (lane == 0) s_tot[wv] = total;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) { const int t = s_tot[w]; before += w < wv ? t : 0; all += t; }
    if (all == 0) continue;                             // (uniform for the workgroup)
    if (threadIdx.x == 0) s_base = atomicAdd(&counts[q * SEL_CNT_PAD], all);
    __syncthreads();
    int base = s_base + before + incl - mine;
#pragma unroll
    for (int g = 0; g < FILT_G; ++g) {
        const int c0 = bx * FILT_PER_BLOCK + g * 4 * TPB + threadIdx.x * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (keepbits & (1u << (g * 4 + k))) {
                if (base < cap) {
                    out_keys[(int64_t)q * cap + base] = ((u64)sk[g][k] << 32) | (u64)cand_rank(a, c0 + k);
                    out_vals[(int64_t)q * cap + base] = cand_val(a, c0 + k);
                }
                ++base;
            }
        }
    }
  }
}

// thresholds of the sample selection: K-th key of every query's winners -> thr[q]; also clears the survivor counters
__global__ void k_sel_thresholds(const u64 *__restrict__ win_keys, int64_t stride, int K, int nq, u64 *__restrict__ thr,
                                 int32_t *__restrict__ counts)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    thr[q] = win_keys[(int64_t)q * stride + (K - 1)];
    counts[q * SEL_CNT_PAD] = 0;
}

// the filter is exact unless a survivor list overflowed or the sample held fewer than K valid candidates
// (!strict, bsc_localize_regions: a sample with fewer than K valid candidates gives the all-ones threshold, which every valid
//  candidate passes — the survivors are then ALL of the query's candidates and only an overflow makes them incomplete; a query
//  with a small region among queries with large ones must not send the whole batch to the unfiltered rounds)
__global__ void k_sel_check(const u64 *__restrict__ thr, const int32_t *__restrict__ counts, int nq, int cap, int32_t *flag, int strict)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (counts[q * SEL_CNT_PAD] > cap || (strict && thr[q] == ~0ull)) *flag = 1;
#ifdef BSC_SEL_DEBUG
    if (q < 4 || q == nq - 1) printf("query %d: %d survivors (cap %d)\n", q, counts[q * SEL_CNT_PAD], cap);
#endif
}

// K <= 512, all queries at once, no device-wide sort:
//   small candidate sets: rounds of 1024-key bitonic selections (round 1 fused with the candidate scan);
//   large sets: selection over a sample of 16 blocks spread over the map gives a per-query threshold, one streaming filter
//   pass keeps the few candidates that beat it, rounds over the survivors finish.  *overflow is set when the host must fall
//   back.  Sample size: nbs x nq bitonic selections for the sample + (K n_cand / (1024 nbs)) / 1024 x nq for the survivors —
//   at 2^20 candidates and K = 100, 16 blocks (~6400 survivors per query) cost a third of 64 blocks (~1600 survivors).
#define SEL_SAMPLE_BLOCKS 16
#define SEL_SURVIVOR_CAP 32768
static bsc_status bitonic_rounds(bsc_ctx *x, int nq, int64_t n, const int32_t *n_per_q, int K, int64_t stride, int *cur)
{
    bool first = true;
    while (n > K || first) {
        const int64_t nb = (n + TK_N - 1) / TK_N;
        const int64_t items = nb * nq;
        hipLaunchKernelGGL(k_block_topk, dim3((unsigned)(items < 4096 ? items : 4096)), dim3(TPB), 0, x->stream,
                           x->l_sel_key[*cur], x->l_sel_val[*cur], n, first ? n_per_q : (const int32_t *)nullptr, stride, K,
                           x->l_sel_key[*cur ^ 1], x->l_sel_val[*cur ^ 1], stride, (int)nb, nq);
        *cur ^= 1;
        n = nb * K;
        first = false;
        if (nb == 1) break;
    }
    return BSC_OK;
}

template <class A>
static bsc_status select_topk_batched(bsc_ctx *x, const A &ca, int nq, int64_t sims_stride, int K, bool allow_filter,
                                      u64 **win_keys, uint32_t **win_vals, int64_t *win_stride, bool *filtered)
{
    const int64_t nb1 = ((int64_t)ca.n_cand + TK_N - 1) / TK_N;
    // the K-th best of a sample of nbs blocks lets about K nb1 / nbs candidates through the filter: enough sample blocks that this
    // stays at a quarter of the survivor lists (K = 100 over 2^20 candidates: 16 blocks, 6 400 survivors; K = 512: 64 blocks;
    // 3 M candidates, K = 100: 36 blocks) — with the fixed 16 of round 3 every K > ~180 overflowed the lists on every call and
    // paid the sample, the filter AND the unfiltered fallback
    int64_t nbs_want = (4 * (int64_t)K * nb1 + SEL_SURVIVOR_CAP - 1) / SEL_SURVIVOR_CAP;
    if (nbs_want < SEL_SAMPLE_BLOCKS) nbs_want = SEL_SAMPLE_BLOCKS;
    const bool use_filter = allow_filter && nb1 > 4 * nbs_want;
    const int64_t nbs = use_filter ? nbs_want : nb1;
    int64_t stride = nbs * K;
    if (use_filter && stride < SEL_SURVIVOR_CAP) stride = SEL_SURVIVOR_CAP;
    BSC_TRY(mem_grow(x->mem, (void **)&x->l_sel_key[0], &x->l_sel_cap[0], sizeof(u64) * stride * nq, false, "localize selection scratch"));
    BSC_TRY(mem_grow(x->mem, (void **)&x->l_sel_key[1], &x->l_sel_cap[1], sizeof(u64) * stride * nq, false, "localize selection scratch"));
    BSC_TRY(mem_grow(x->mem, (void **)&x->l_sel_val[0], &x->l_sel_cap[2], sizeof(uint32_t) * stride * nq, false, "localize selection scratch"));
    BSC_TRY(mem_grow(x->mem, (void **)&x->l_sel_val[1], &x->l_sel_cap[3], sizeof(uint32_t) * stride * nq, false, "localize selection scratch"));
    BSC_TRY(mem_grow(x->mem, (void **)&x->l_sel_thr, &x->l_sel_cap[4], sizeof(u64) * (int64_t)(nq + 1), false, "localize selection scratch"));
    BSC_TRY(mem_grow(x->mem, (void **)&x->l_sel_cnt, &x->l_sel_cap[5], sizeof(int32_t) * nq * SEL_CNT_PAD, false, "localize selection scratch"));
    int cur = 0;
    // round 1 over the sample (or over everything), fused with the candidate keys
    hipLaunchKernelGGL(k_cand_topk<A>, dim3((unsigned)(nbs * nq < 4096 ? nbs * nq : 4096)), dim3(TPB), 0, x->stream, ca, x->l_sims,
                       sims_stride, K, x->l_sel_key[0], x->l_sel_val[0], stride, (int)nbs, nq, use_filter ? (int)(nb1 / nbs) : 1);
    if (nbs > 1) BSC_TRY(bitonic_rounds(x, nq, nbs * K, nullptr, K, stride, &cur));
    *filtered = false;
    if (use_filter) {
        // per-query threshold = K-th key of the sample winners (kept aside: the selection buffers are reused)
        hipLaunchKernelGGL(k_sel_thresholds, dim3((nq + 255) / 256), dim3(256), 0, x->stream, x->l_sel_key[cur], stride, K, nq,
                           x->l_sel_thr, x->l_sel_cnt);
        cur = 0;
        const unsigned nbf = (unsigned)(((int64_t)ca.n_cand + FILT_PER_BLOCK - 1) / FILT_PER_BLOCK);
        if (!ca.exact && std::is_same<A, CandArgs>::value) {
            // every wavefront of the ceil(max_id / TPB) workgroups stores one 64-bit word: TPB / 32 uint32 per workgroup.  Grown with
            // slack (a map that gains a few voxels between two queries keeps its bitmap allocation)
            const int64_t words = (TPB / 32) * (((int64_t)ca.max_id + TPB - 1) / TPB) + 2;
            if ((int64_t)sizeof(uint32_t) * words > x->l_sel_cap[6])
                BSC_TRY(mem_grow(x->mem, (void **)&x->l_valid, &x->l_sel_cap[6], sizeof(uint32_t) * (words + words / 4 + 1024), false, "localize row bitmap"));
            if (ca.max_id > 0)
                hipLaunchKernelGGL(k_valid_bits, dim3((unsigned)((ca.max_id + TPB - 1) / TPB)), dim3(TPB), 0, x->stream, ca.cnt, ca.max_id, x->l_valid);
        }
        // dense maps without region / floor filter: candidate c is row c, similarities stream as 16-byte loads
        bool fast = false;
        if constexpr (std::is_same<A, CandArgs>::value)
            fast = !ca.exact && region_open(ca.region) && (sims_stride % 4 == 0);
        const dim3 fgrid(nbf * (unsigned)nq < 16384u ? nbf * (unsigned)nq : 16384u);
        if constexpr (std::is_same<A, CandArgs>::value) {
          if (fast)
            hipLaunchKernelGGL((k_cand_filter<true, A>), fgrid, dim3(TPB), 0, x->stream, ca, x->l_sims, sims_stride, x->l_sel_thr, K,
                               SEL_SURVIVOR_CAP, x->l_sel_key[0], x->l_sel_val[0], x->l_sel_cnt, (int)nbf, nq, (const uint32_t *)x->l_valid);
        }
        if (!fast)
            hipLaunchKernelGGL((k_cand_filter<false, A>), fgrid, dim3(TPB), 0, x->stream, ca, x->l_sims, sims_stride, x->l_sel_thr, K,
                               SEL_SURVIVOR_CAP, x->l_sel_key[0], x->l_sel_val[0], x->l_sel_cnt, (int)nbf, nq, (const uint32_t *)x->l_valid);
        // survivors of query q sit at [q * CAP, q * CAP + count); the rounds use stride CAP for them
        BSC_TRY(bitonic_rounds(x, nq, SEL_SURVIVOR_CAP, x->l_sel_cnt, K, SEL_SURVIVOR_CAP, &cur));
        stride = SEL_SURVIVOR_CAP;
        *filtered = true;
    }
    BSC_HIP(hipGetLastError());
    *win_keys = x->l_sel_key[cur];
    *win_vals = x->l_sel_val[cur];
    *win_stride = stride;
    return BSC_OK;
}

bsc_status pool_query_impl(bsc_ctx *x, const float *tokens, int32_t B, int32_t T, int32_t D, float *out)
{
    hipLaunchKernelGGL(k_pool_query, dim3((D + TPB - 1) / TPB), dim3(TPB), 0, x->stream, tokens, B, T, D, out);
    BSC_HIP(hipGetLastError());
    return BSC_OK;
}

// name ranks (HDF5 iteration order) are rebuilt only when the set of stored voxels changed
static bsc_status ensure_name_ranks(bsc_ctx *x, const VoxelView &v)
{
    if (!x->names_dirty) return BSC_OK;
    const int n_cand = v.max_id + 1;
    const dim3 block(TPB), cgrid((n_cand + TPB - 1) / TPB);
    hipLaunchKernelGGL(k_name_keys, cgrid, block, 0, x->stream, n_cand, v.max_id, v.vcap, v.rgb_pos, v.cnt, x->l_key_a, x->l_val_a);
    BSC_TRY(prim_sort_pairs(lane_main(x), x->l_key_a, x->l_key_b, x->l_val_a, x->l_val_b, (size_t)n_cand, 0, 64));
    hipLaunchKernelGGL(k_name_rank, cgrid, block, 0, x->stream, n_cand, x->l_val_b, x->l_name_rank);
    x->names_dirty = false;
    return BSC_OK;
}

// What the first query after a change of the stored voxels / rows would have to do first — the name ranks (HDF5 iteration order)
// and, for the batched fp16-piece scan, every row's operand scale and inverse norm — done by the one that changed them.  Called at
// the end of the import entry points (round 6: a loaded memory's first batch of 256 queries took 3.1 ms instead of 2.2; an ingest
// leaves both current on its own).  A failure here is not an error of the import: the flags stay set and the query does the work.
void localize_prepare(bsc_ctx *x)
{
    if (read_scalars(x) != BSC_OK) return;
    int n_cand;
    int64_t n_rows;
    const float *rows;
    const VoxelView v = store_view(x, &n_cand, &n_rows, &rows);
    if (v.max_id > 0 && ensure_name_ranks(x, v) != BSC_OK) return;
    if (x->row_scale_dirty && refresh_row_scales(x, rows, n_rows, &x->l_rscale, &x->l_rscale_cap, &x->row_scale_dirty) != BSC_OK) return;
    (void)hipGetLastError();
}

// the counts the callers get (entries of a query's K with a position) and the shape of the results that stay resident
static void record_counts(bsc_ctx *x, int nq, int K, const int32_t *out_pos, int32_t *out_count)
{
    for (int qi = 0; qi < nq; ++qi) {
        int n = 0;
        while (n < K && out_pos[((int64_t)qi * K + n) * 3] >= 0) ++n;
        out_count[qi] = n;
        x->last_counts[qi] = n;
    }
    x->last_nq = nq;
    x->last_K = K;
}

// top-K of every query from its similarities (x->l_sims, rows sstride apart) -> x->l_out_pos / l_out_sim (they stay resident as the
// "last localize" results) and the host arrays
template <class A>
static bsc_status select_and_copy_out(bsc_ctx *x, const A &ca, int nq, int K, int64_t sstride, int strict, int32_t *out_pos,
                                      float *out_sim, int32_t *out_count)
{
    hipStream_t s = x->stream;
    const dim3 block(TPB), cgrid((ca.n_cand + TPB - 1) / TPB);
    bool filtered = false;
    if (K <= TK_N / 2) {
        static const int sel_min_q = getenv("BSC_SEL_MIN_Q") ? atoi(getenv("BSC_SEL_MIN_Q")) : 5;     // sample + filter from this many queries on (Q = 1: 0.79 vs 0.87 ms without / with; Q = 8: 1.08 vs 0.98; Q = 12: 1.20 vs 1.00)
        for (int attempt = 0; attempt < 2; ++attempt) {
            u64 *wk; uint32_t *wv; int64_t ws;
            BSC_TRY(select_topk_batched(x, ca, nq, sstride, K, attempt == 0 && nq >= sel_min_q, &wk, &wv, &ws, &filtered));
            hipLaunchKernelGGL(k_gather_topk, dim3((K + TPB - 1) / TPB, (unsigned)nq), block, 0, s, K, /*entries*/ K, ca.max_id,
                               ca.vcap, wk, wv, ws, x->rgb_pos, x->l_out_pos, x->l_out_sim);
            if (!filtered) break;
            int32_t *flag = (int32_t *)(x->l_sel_thr + nq);      // spare slot behind the thresholds
            BSC_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
            hipLaunchKernelGGL(k_sel_check, dim3((nq + 255) / 256), dim3(256), 0, s, x->l_sel_thr, x->l_sel_cnt, nq,
                               SEL_SURVIVOR_CAP, flag, strict);
            int32_t redo = 0;
            BSC_HIP(hipMemcpyAsync(&redo, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            BSC_HIP(hipStreamSynchronize(s));
            if (!redo) break;
        }
    } else {                                   // large K: device-wide sort per query
        for (int qi = 0; qi < nq; ++qi) {
            hipLaunchKernelGGL(k_candidates<A>, cgrid, block, 0, s, ca, qi, x->l_sims + (int64_t)qi * sstride, x->l_key_a, x->l_val_a);
            BSC_TRY(prim_sort_pairs(lane_main(x), x->l_key_a, x->l_key_b, x->l_val_a, x->l_val_b, (size_t)ca.n_cand, 0, 64));
            hipLaunchKernelGGL(k_gather_topk, dim3((K + TPB - 1) / TPB), block, 0, s, K, ca.n_cand, ca.max_id, ca.vcap, x->l_key_b,
                               x->l_val_b, (int64_t)0, x->rgb_pos, x->l_out_pos + (int64_t)qi * K * 3,
                               x->l_out_sim + (int64_t)qi * K);
        }
    }
    BSC_HIP(hipGetLastError());
    BSC_HIP(hipMemcpyAsync(out_pos, x->l_out_pos, sizeof(int32_t) * (size_t)nq * K * 3, hipMemcpyDeviceToHost, s));
    BSC_HIP(hipMemcpyAsync(out_sim, x->l_out_sim, sizeof(float) * (size_t)nq * K, hipMemcpyDeviceToHost, s));
    BSC_HIP(hipStreamSynchronize(s));
    record_counts(x, nq, K, out_pos, out_count);
    return BSC_OK;
}

bsc_status localize_impl(bsc_ctx *x, const float *q_dev, int32_t nq, int32_t K, double radius, const int32_t *curr,
                         int32_t floor_lo, int32_t floor_hi, int32_t *out_pos, float *out_sim, int32_t *out_count)
{
    BSC_TRY(read_scalars(x));
    int n_cand;
    int64_t n_rows;
    const float *rows;
    const VoxelView v = store_view(x, &n_cand, &n_rows, &rows);
    if (K > 4096 || K < 1 || nq < 1 || nq > 1024) {
        bsc_set_error("bsc_localize: K=%d (1..4096), n_queries=%d (1..1024)", K, nq);
        return BSC_E_INVALID;
    }
    BSC_TRY(ensure_name_ranks(x, v));
    BSC_TRY(stage_queries(x, q_dev, nq));
    stat_begin(x, 1);
    int passes = 0;                          // times the row matrix is streamed
    BSC_TRY(cosine_scan(x, rows, n_rows, nq, &x->l_rscale, &x->l_rscale_cap, &x->row_scale_dirty, &passes));
    stat_end(x, 1, (double)n_rows * x->c.token_dim * 4.0 * passes + (double)nq * n_rows * 4.0);
    return select_and_copy_out(x, cand_args(v, n_cand, region_dev(radius, curr, floor_lo, floor_hi)), nq, K, sims_row_stride(n_rows),
                               /*strict*/ 1, out_pos, out_sim, out_count);
}

// ---- bsc_localize_regions: a sphere and a floor band per query, pruned scan ---------------------------------------------
// Every call of voxel_localized in the reference's agent carries its own curr_grid / region_radius (BSCAgent.py:630,643,647;
// the adaptive loop :1078-1098 asks one prompt with radius 30, 40, 50).  One call ranks Q queries, each inside its own region:
//   k_region_visibility  one thread per voxel against the Q regions (in LDS): the (query, voxel) bits the selection reads back
//                        instead of repeating the test, "some query sees it", and per 256 voxels the visible voxels / rows
//   k_region_scatter     (pruned scan) exclusive positions of the visible voxels: entry -> voxel, entry -> first gathered row
//   k_region_gather_rows (pruned scan) the visible voxels' rows, 16-byte loads, into a scratch matrix on which the scan kernels
//                        of bsc_localize run unchanged
// and the selection kernels above, instantiated for RegionCandArgs.
struct RegionWs {
    RegionDev *regions, *regions_pin;     // (1024) device / pinned host
    int64_t *tot_pin;                     // pinned: visible voxels << 40 | visible rows
    uint32_t *mask;
    uint8_t *vis;
    int64_t *blk_tot, *blk_off;           // per 256 voxels: visible voxels << 40 | their rows; exclusive prefix (+ the total)
    uint32_t *cidx;
    int32_t *rowoff;
    float *rows;                          // gathered rows
    float2 *rscale;                       // their fp16-piece scales (recomputed per call)
    int64_t mask_cap, vis_cap, blk_cap[2], cidx_cap, rowoff_cap, rows_cap, rscale_cap;
};
#define RG_ROWS_BITS 40
// Share of the store's rows above which the whole store is scanned instead of a gathered copy of the visible rows.  The gather
// reads and writes every visible row once before the scan reads it again, so the break-even sits near a third: measured (Q = 8,
// store shape, 2^20 voxels / 5.77 M rows x 1024, sweep of radii in DESIGN.md section 4) pruned 3.96 ms against 5.26 ms at a
// share of 0.25, 5.85 against 5.38 at 0.38 — crossover 0.34.  BSC_REGION_PRUNE = never | always | <share> overrides it per call.
#ifndef BSC_REGION_PRUNE_SHARE
#define BSC_REGION_PRUNE_SHARE 0.33
#endif

static bsc_status region_ws_get(bsc_ctx *x, RegionWs **out)
{
    if (!x->regn) {
        RegionWs *w = (RegionWs *)calloc(1, sizeof(RegionWs));
        if (!w) { bsc_set_error("bsc_localize_regions: out of host memory"); return BSC_E_HIP; }
        const uint64_t mark = mem_mark(x->mem);
        bsc_status st = mem_alloc(x->mem, (void **)&w->regions, sizeof(RegionDev) * 1024, "regions");
        if (st == BSC_OK) st = mem_alloc_pinned(x->mem, (void **)&w->regions_pin, sizeof(RegionDev) * 1024, MEM_PIN_DEFAULT, "pinned regions");
        if (st == BSC_OK) st = mem_alloc_pinned(x->mem, (void **)&w->tot_pin, sizeof(int64_t), MEM_PIN_DEFAULT, "pinned region totals");
        if (st != BSC_OK) { mem_release_to(x->mem, mark); free(w); return st; }
        x->regn = w;                          // published once all of it exists: a failed first call leaves it null
    }
    *out = x->regn;
    return BSC_OK;
}

__global__ __launch_bounds__(TPB) void k_region_visibility(int n_cand, int max_id, int vcap, int exact,
                                                           const int32_t *__restrict__ rgb_pos, const int32_t *__restrict__ cnt,
                                                           const RegionDev *__restrict__ regions, int nq,
                                                           uint32_t *__restrict__ mask, int64_t mask_stride,
                                                           uint8_t *__restrict__ vis, int64_t *__restrict__ blk_tot)
{
    __shared__ RegionDev sreg[1024];
    for (int i = threadIdx.x; i < nq; i += TPB) sreg[i] = regions[i];
    __syncthreads();
    const int c = blockIdx.x * TPB + threadIdx.x;
    const bool in = c < n_cand;
    const int e = (c == max_id) ? vcap : c;
    const int m = in ? cnt[e] : 0;
    int r = 0, cc = 0, h = 0;
    if (in && c != max_id) { r = rgb_pos[3 * e]; cc = rgb_pos[3 * e + 1]; h = rgb_pos[3 * e + 2]; }
    uint32_t any = 0u;
    for (int w = 0; w * 32 < nq; ++w) {
        uint32_t bits = 0u;
        if (m > 0) {                                            // voxels without tokens see nothing
            const int nb = min(32, nq - w * 32);
            for (int b = 0; b < nb; ++b) bits |= region_sees(sreg[w * 32 + b], r, cc, h) ? (1u << b) : 0u;
        }
        if (in) mask[(int64_t)w * mask_stride + c] = bits;
        any |= bits;
    }
    const int seen = any != 0u ? 1 : 0;
    if (in) vis[c] = (uint8_t)seen;
    int ea, eb, ta, tb;
    block_scan2<TPB>(seen, seen ? (exact ? m : 1) : 0, ea, eb, ta, tb);
    if (threadIdx.x == 0) blk_tot[blockIdx.x] = ((int64_t)ta << RG_ROWS_BITS) | (int64_t)tb;
}

__global__ __launch_bounds__(TPB) void k_region_scatter(int n_cand, int max_id, int vcap, int exact, const int32_t *__restrict__ cnt,
                                                        const uint8_t *__restrict__ vis, const int64_t *__restrict__ blk_off,
                                                        uint32_t *__restrict__ cidx, int32_t *__restrict__ rowoff)
{
    const int c = blockIdx.x * TPB + threadIdx.x;
    const int seen = (c < n_cand && vis[c]) ? 1 : 0;
    const int nr = seen ? (exact ? cnt[(c == max_id) ? vcap : c] : 1) : 0;
    int ea, eb, ta, tb;
    block_scan2<TPB>(seen, nr, ea, eb, ta, tb);
    if (!seen) return;
    const int64_t base = blk_off[blockIdx.x];
    const int64_t i = (base >> RG_ROWS_BITS) + ea;
    cidx[i] = (uint32_t)c;
    rowoff[i] = (int32_t)((base & (((int64_t)1 << RG_ROWS_BITS) - 1)) + eb);
}

// one wavefront per visible voxel: its rows (token-pool rows of an exact store, the accumulator row of a dense map) -> out
__global__ __launch_bounds__(TPB) void k_region_gather_rows(int n_vis, int max_id, int vcap, int exact, int cache_size, int D,
                                                            const uint32_t *__restrict__ cidx, const int32_t *__restrict__ rowoff,
                                                            const int32_t *__restrict__ cnt, const int32_t *__restrict__ store_rows,
                                                            const float *__restrict__ rows, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    if (i >= n_vis) return;
    const int c = (int)cidx[i];
    const int e = (c == max_id) ? vcap : c;
    const int m = exact ? cnt[e] : 1;
    const int64_t base = rowoff[i];
    for (int k = 0; k < m; ++k) {
        const int64_t src_row = exact ? (int64_t)store_rows[(int64_t)e * cache_size + k] : (int64_t)c;
        const float4 *src = (const float4 *)(rows + src_row * D);
        float4 *dst = (float4 *)(out + (base + k) * D);
        for (int v = lane; v < (D >> 2); v += 64) dst[v] = src[v];
    }
}

__global__ __launch_bounds__(TPB) void k_fill_no_result(int64_t n, int32_t *__restrict__ out_pos, float *__restrict__ out_sim)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    out_pos[3 * i] = -1; out_pos[3 * i + 1] = -1; out_pos[3 * i + 2] = -1;
    out_sim[i] = -INFINITY;
}

// The front half of bsc_localize_regions, shared with bsc_score_map (score_map.hip): both calls run the identical scan, on the same
// rows with the same kernel choice, so their scores agree bit for bit.
bsc_status region_scan(bsc_ctx *x, const float *q_dev, int32_t nq, const bsc_region *regions, RegionScan *out)
{
    hipStream_t s = x->stream;
    const int D = x->c.token_dim;
    const dim3 block(TPB);
    RegionWs *w;
    BSC_TRY(region_ws_get(x, &w));
    BSC_TRY(read_scalars(x));
    int n_cand;
    int64_t n_rows;
    const float *rows;
    const VoxelView v = store_view(x, &n_cand, &n_rows, &rows);
    BSC_TRY(ensure_name_ranks(x, v));
    BSC_TRY(stage_queries(x, q_dev, nq));
    // the regions as the kernels read them; a query with neither sphere nor band sees every voxel
    bool any_open = false, all_open = true;
    for (int qi = 0; qi < nq; ++qi) {
        w->regions_pin[qi] = regions ? region_dev(regions[qi].radius, regions[qi].curr, regions[qi].floor_lo, regions[qi].floor_hi)
                                     : region_dev(-1.0, nullptr, 0, -1);
        if (region_open(w->regions_pin[qi])) any_open = true;
        else all_open = false;
    }
    BSC_HIP(hipMemcpyAsync(w->regions, w->regions_pin, sizeof(RegionDev) * (size_t)nq, hipMemcpyHostToDevice, s));
    // pruning knob, read per call like the BSC_COSINE_* knobs
    double share = BSC_REGION_PRUNE_SHARE;
    bool never = false, always = false;
    if (const char *e = getenv("BSC_REGION_PRUNE")) {
        if (!strcmp(e, "never")) never = true;
        else if (!strcmp(e, "always")) always = true;
        else if (*e) share = atof(e);
    }
    // visibility pass (skipped when the union of the regions is the whole map)
    const bool pass = !any_open;
    const int64_t mask_stride = ((int64_t)n_cand + 63) & ~(int64_t)63;
    const int nblk = (n_cand + TPB - 1) / TPB;
    int64_t n_vis = 0, n_vis_rows = 0;
    bool pruned = false;
    if (pass) {
        const int nwords = (nq + 31) / 32;
        if (w->mask_cap < (int64_t)sizeof(uint32_t) * mask_stride * nwords)
            BSC_TRY(mem_grow(x->mem, (void **)&w->mask, &w->mask_cap, sizeof(uint32_t) * (mask_stride + mask_stride / 8 + 1024) * nwords, false, "region scratch"));
        if (w->vis_cap < n_cand) BSC_TRY(mem_grow(x->mem, (void **)&w->vis, &w->vis_cap, n_cand + n_cand / 8 + 1024, false, "region scratch"));
        if (w->blk_cap[0] < (int64_t)sizeof(int64_t) * (nblk + 1)) {
            BSC_TRY(mem_grow(x->mem, (void **)&w->blk_tot, &w->blk_cap[0], sizeof(int64_t) * (nblk + nblk / 8 + 64), false, "region scratch"));
            BSC_TRY(mem_grow(x->mem, (void **)&w->blk_off, &w->blk_cap[1], sizeof(int64_t) * (nblk + nblk / 8 + 64), false, "region scratch"));
        }
        BSC_HIP(hipMemsetAsync(w->blk_tot + nblk, 0, sizeof(int64_t), s));           // the scan's last output is the total
        hipLaunchKernelGGL(k_region_visibility, dim3(nblk), block, 0, s, n_cand, v.max_id, v.vcap, v.exact, v.rgb_pos, v.cnt,
                           (const RegionDev *)w->regions, nq, w->mask, mask_stride, w->vis, w->blk_tot);
        if (!never) {
            BSC_TRY(prim_exclusive_sum_i64(lane_main(x), w->blk_tot, w->blk_off, (size_t)nblk + 1));
            BSC_HIP(hipMemcpyAsync(w->tot_pin, w->blk_off + nblk, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            BSC_HIP(hipStreamSynchronize(s));
            n_vis = *w->tot_pin >> RG_ROWS_BITS;
            n_vis_rows = *w->tot_pin & (((int64_t)1 << RG_ROWS_BITS) - 1);
            pruned = always || (double)n_vis_rows < share * (double)n_rows;
        }
    }
    out->n_voxels = n_cand;
    out->all_open = all_open;
    out->nothing = pruned && n_vis == 0;   // no query sees anything
    out->sstride = 0;
    if (out->nothing) return BSC_OK;
    const float *scan_rows = rows;
    int64_t scan_n = n_rows;
    float2 **rs = &x->l_rscale;
    int64_t *rs_cap = &x->l_rscale_cap;
    bool scratch_dirty = true, *rs_dirty = &x->row_scale_dirty;
    if (pruned) {
        if (w->cidx_cap < (int64_t)sizeof(uint32_t) * n_vis) {
            BSC_TRY(mem_grow(x->mem, (void **)&w->cidx, &w->cidx_cap, sizeof(uint32_t) * (n_vis + n_vis / 4 + 1024), false, "region scratch"));
            BSC_TRY(mem_grow(x->mem, (void **)&w->rowoff, &w->rowoff_cap, sizeof(int32_t) * (n_vis + n_vis / 4 + 1024), false, "region scratch"));
        }
        if (w->rows_cap < (int64_t)sizeof(float) * n_vis_rows * D)
            BSC_TRY(mem_grow(x->mem, (void **)&w->rows, &w->rows_cap, sizeof(float) * (n_vis_rows + n_vis_rows / 4 + 1024) * D, false, "region scratch"));
        hipLaunchKernelGGL(k_region_scatter, dim3(nblk), block, 0, s, n_cand, v.max_id, v.vcap, v.exact, v.cnt,
                           (const uint8_t *)w->vis, (const int64_t *)w->blk_off, w->cidx, w->rowoff);
        hipLaunchKernelGGL(k_region_gather_rows, dim3((unsigned)((n_vis * 64 + TPB - 1) / TPB)), block, 0, s, (int)n_vis, v.max_id, v.vcap,
                           v.exact, v.cache_size, D, (const uint32_t *)w->cidx, (const int32_t *)w->rowoff, v.cnt, v.store_rows, rows,
                           w->rows);
        scan_rows = w->rows; scan_n = n_vis_rows;
        rs = &w->rscale; rs_cap = &w->rscale_cap; rs_dirty = &scratch_dirty;
    }
    stat_begin(x, 1);
    out->sstride = sims_row_stride(scan_n);
    int passes = 0;
    BSC_TRY(cosine_scan(x, scan_rows, scan_n, nq, rs, rs_cap, rs_dirty, &passes));
    stat_end(x, 1, (double)scan_n * D * 4.0 * passes + (double)nq * scan_n * 4.0);
    RegionCandArgs &ca = out->ca;
    (VoxelView &)ca = v;
    ca.n_cand = pruned ? (int)n_vis : n_cand;
    ca.regions = w->regions;
    ca.mask = pass ? w->mask : nullptr; ca.mask_stride = mask_stride;
    ca.cidx = pruned ? w->cidx : nullptr; ca.rowoff = pruned ? w->rowoff : nullptr;
    return BSC_OK;
}

bsc_status localize_regions_impl(bsc_ctx *x, const float *q_dev, int32_t nq, int32_t K, const bsc_region *regions,
                                 int32_t *out_pos, float *out_sim, int32_t *out_count)
{
    hipStream_t s = x->stream;
    RegionScan rg;
    BSC_TRY(region_scan(x, q_dev, nq, regions, &rg));
    if (rg.nothing) {
        hipLaunchKernelGGL(k_fill_no_result, dim3((unsigned)(((int64_t)nq * K + TPB - 1) / TPB)), dim3(TPB), 0, s, (int64_t)nq * K,
                           x->l_out_pos, x->l_out_sim);
        BSC_HIP(hipGetLastError());
        BSC_HIP(hipStreamSynchronize(s));
        for (int64_t i = 0; i < (int64_t)nq * K; ++i) { out_pos[3 * i] = out_pos[3 * i + 1] = out_pos[3 * i + 2] = -1; out_sim[i] = -INFINITY; }
        record_counts(x, nq, K, out_pos, out_count);      // all zero
        return BSC_OK;
    }
    if (rg.all_open)                       // no region anywhere: bsc_localize's own selection (its dense fast filter included)
        return select_and_copy_out(x, cand_args_open(rg.ca, rg.n_voxels), nq, K, rg.sstride, /*strict*/ 1, out_pos, out_sim, out_count);
    return select_and_copy_out(x, rg.ca, nq, K, rg.sstride, /*strict*/ 0, out_pos, out_sim, out_count);
}
