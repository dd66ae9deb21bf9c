// cosine_scan.hip — the cosine scan of voxel_localized (memory_2.py:656): staged queries x stored rows -> x->l_sims, the similarity
// matrix the selection of localize.hip reads.  cosine_scan picks the kernel by the number of queries and the BSC_COSINE_* knobs:
//   k_cosine         up to 4 queries: one wavefront per token row on the vector ALUs, the row streamed from HBM once per pass
//   k_cosine_mfma    5..64 queries (and every remainder <= 64): 32-query tiles on the f32 matrix cores
//   k_cosine_f16x2   more than 64 queries: two fp16 pieces per operand, three products, f32 accuracy (row scales: k_row_scale)
//   k_cosine_bf16x3  its A/B form (BSC_COSINE_BF16): three bf16 pieces, six (BSC_COSINE_PIECES=3: three) products
// The matrix-core kernels share clear_tiles / store_tiles, the two piece kernels also load_x and QStage; the piece split and the
// product ladder are each kernel's own.
#include "bsc_internal.h"

#include <math.h>

#define TPB 256

// q (Q,D) -> q / max(|q|, 1e-8)   (torch cosine_similarity eps clamp)
__global__ __launch_bounds__(64) void k_normalize_q(const float *__restrict__ q, int D, float *__restrict__ qn)
{
    const int lane = threadIdx.x;
    const float *src = q + (int64_t)blockIdx.x * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s += src[k] * src[k];
    s = wave_sum(s);
    const float nrm = fmaxf(sqrtf(s), 1e-8f);
    for (int k = lane; k < D; k += 64) qn[(int64_t)blockIdx.x * D + k] = src[k] / nrm;
}

// Wave-wide sums of QT per-lane values at once (QT = 2, 4, 8): every butterfly step over a lane bit also halves the number
// of values a lane carries (the half of the wavefront with the bit set keeps the upper values), so QT sums cost
// QT - 1 + log2(64 / QT) exchanges instead of 6 QT.  The pairs added at each distance are those of wave_sum, so every
// sum is bit-identical to wave_sum of that value.  Returns the sum of value `q` in the lanes whose bits 5.. select q:
// q = lane >> (6 - log2 QT); all lanes of that group hold it.
template <int QT>
__device__ __forceinline__ float multi_wave_sum(float (&v)[QT], int lane)
{
    int mask = 32;
#pragma unroll
    for (int keep = QT >> 1; keep >= 1; keep >>= 1) {
        const bool hi = (lane & mask) != 0;
#pragma unroll
        for (int i = 0; i < keep; ++i) {
            const float mine = hi ? v[i + keep] : v[i], theirs = hi ? v[i] : v[i + keep];
            v[i] = mine + __shfl_xor(theirs, mask);
        }
        mask >>= 1;
    }
    float r = v[0];
    for (; mask > 0; mask >>= 1) r += __shfl_xor(r, mask);
    return r;
}

// sims[qi * n_rows + row] = dot(q^[qi], x[row]) / max(|x[row]|, 1e-8).
// One wavefront per row (grid-stride), NV float4 per lane; the row is loaded once and reused for QT queries.
template <int NV, int QT>
__global__ __launch_bounds__(TPB) void k_cosine(const float *__restrict__ rows, int64_t n_rows, int D,
                                                const float *__restrict__ qn, int q0, float *__restrict__ sims,
                                                int64_t sims_stride)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * TPB) >> 6;
    const int D4 = D >> 2;
    float4 qv[QT][NV];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi)
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int v = lane + 64 * t;
            qv[qi][t] = (v < D4) ? ((const float4 *)(qn + (int64_t)(q0 + qi) * D))[v] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    for (int64_t r = wave; r < n_rows; r += nwaves) {
        const float4 *src = (const float4 *)(rows + r * D);
        float4 xv[NV];
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int v = lane + 64 * t;
            xv[t] = (v < D4) ? src[v] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float n2 = 0.f;
#pragma unroll
        for (int t = 0; t < NV; ++t) n2 += xv[t].x * xv[t].x + xv[t].y * xv[t].y + xv[t].z * xv[t].z + xv[t].w * xv[t].w;
        n2 = wave_sum(n2);
        const float inv = 1.0f / fmaxf(sqrtf(n2), 1e-8f);
        float dsum[QT];
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            float d = 0.f;
#pragma unroll
            for (int t = 0; t < NV; ++t)
                d += xv[t].x * qv[qi][t].x + xv[t].y * qv[qi][t].y + xv[t].z * qv[qi][t].z + xv[t].w * qv[qi][t].w;
            dsum[qi] = d;
        }
        if (QT == 1) {
            const float d = wave_sum(dsum[0]);
            if (lane == 0) sims[(int64_t)q0 * sims_stride + r] = d * inv;
        } else {
            // the wavefront's QT groups of 64 / QT lanes end up with one query's sum each; their first lanes store
            const float d = multi_wave_sum<QT>(dsum, lane);
            if ((lane & (64 / QT - 1)) == 0) sims[(int64_t)(q0 + lane / (64 / QT)) * sims_stride + r] = d * inv;
        }
    }
}

// ---- what the three matrix-core kernels share -------------------------------------------------------------------------------
// A wavefront owns 32 rows of X and NT tiles of 32 queries: S^T tile (32 queries x 32 rows), 16 accumulator registers per tile.
// Queries sit on the M axis so that the accumulator columns are rows of X: stores are 128-byte row runs per query.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
__device__ __forceinline__ void clear_tiles(f32x16 (&acc)[NT])
{
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// epilogue of lane (n, g) = (lane & 31, lane >> 5), whose row is `row`: accumulator register r of tile t belongs to query
// q0 + 32 t + (r & 3) + 8 (r >> 2) + 4 g; `factor` is what turns the row's dot products into cosines
template <int NT>
__device__ __forceinline__ void store_tiles(const f32x16 (&acc)[NT], float factor, int64_t row, int64_t n_rows, int g, int q0,
                                            int q_valid, float *sims, int64_t sims_stride)
{
    if (row >= n_rows) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
            if (q < q_valid) sims[(int64_t)q * sims_stride + row] = acc[t][r] * factor;
        }
}

// ---- batched queries on the matrix cores -----------------------------------------------------------------------
// S^T tile = Qn (32 x D) . X^T (D x 32) with v_mfma_f32_32x32x2_f32: fp32 in, fp32 accumulate, bit-for-bit an fmaf chain
// (no TF32 on gfx950), 64 cycles per instruction.  One workgroup = 4 waves = 128 rows.  K is walked in chunks of 32 staged
// through LDS (row stride 33 floats: conflict-free ds_read_b32 for the 32-lane operand groups), double-buffered
// with register prefetch of the next chunk.  The squared row norms fall out of the B operands the lanes already hold.
#define MF_KC 32
#ifndef BSC_MFMA_MIN_Q
#define BSC_MFMA_MIN_Q 5     // up to 4 queries: one wavefront per row on the vector ALUs (k_cosine, 5.6 TB/s); from 5 on the
                             // VALU dot products no longer hide behind the row stream (8 queries: 3.6 TB/s) and a zero-padded
                             // 32-query MFMA tile is faster (4.9 TB/s for 5..32 queries over 2^20 x 768)
#endif
#define MF_LD 33
template <int NT>
__global__ __launch_bounds__(TPB) void k_cosine_mfma(const float *__restrict__ X, int64_t n_rows, int D,
                                                     const float *__restrict__ qn, int q0, int q_valid,
                                                     float *__restrict__ sims, int64_t sims_stride)
{
    __shared__ float Xs[2][128 * MF_LD];
    __shared__ float Qs[2][NT * 32 * MF_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * 128;
    const int nchunks = D / MF_KC;
    f32x16 acc[NT];
    clear_tiles(acc);
    float nrm = 0.f;
    float4 xr[4], qr[NT];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + TPB * i, r = idx >> 3, c4 = idx & 7;
            const int64_t gr = row0 + r;
            xr[i] = gr < n_rows ? *(const float4 *)(X + gr * D + c * MF_KC + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int idx = tid + TPB * i, r = idx >> 3, c4 = idx & 7;
            qr[i] = *(const float4 *)(qn + (int64_t)(q0 + r) * D + c * MF_KC + c4 * 4);
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + TPB * i, r = idx >> 3, c4 = idx & 7;
            float *d = &Xs[buf][r * MF_LD + c4 * 4];
            d[0] = xr[i].x; d[1] = xr[i].y; d[2] = xr[i].z; d[3] = xr[i].w;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int idx = tid + TPB * i, r = idx >> 3, c4 = idx & 7;
            float *d = &Qs[buf][r * MF_LD + c4 * 4];
            d[0] = qr[i].x; d[1] = qr[i].y; d[2] = qr[i].z; d[3] = qr[i].w;
        }
    };
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) load_chunk(c + 1);
        const float *xb = &Xs[buf][(w * 32 + (lane & 31)) * MF_LD + (lane >> 5)];
        const float *qb = &Qs[buf][(lane & 31) * MF_LD + (lane >> 5)];
#pragma unroll 4
        for (int kk = 0; kk < MF_KC; kk += 2) {
            const float b = xb[kk];
            nrm = fmaf(b, b, nrm);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float a = qb[t * 32 * MF_LD + kk];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
            }
        }
        if (c + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }
    nrm += __shfl_xor(nrm, 32);
    const float inv = 1.0f / fmaxf(sqrtf(nrm), 1e-8f);
    store_tiles(acc, inv, row0 + w * 32 + (lane & 31), n_rows, lane >> 5, q0, q_valid, sims, sims_stride);
}

// ---- the two piece kernels: what they share ---------------------------------------------------------------------------------
// The f32 MFMA peaks at 157 TFLOP/s, the 16-bit ones at 2.5 PFLOP/s; an f32 operand split into 16-bit pieces whose products
// accumulate in the matrix core's f32 accumulators keeps f32 accuracy at a fraction of the matrix time.  Layout of the work in both:
//   A operand (M axis): 32 queries per tile, NT tiles — the pieces of the normalised queries come precomputed as PL planes
//                       (k_split_q / k_split_q_f16) and are staged per 32-wide K chunk through LDS (80-byte row pitch),
//                       double-buffered with a register prefetch;
//   B operand (N axis): the wavefront's 32 rows straight from global memory in fragment layout — lane (n, g) loads the 16
//                       floats [32 c + 16 g, + 16) of row n (one 128-byte line per row and chunk over the two lane groups),
//                       splits them in registers; sub-step s of a chunk contracts floats [8 s, 8 s + 8) of every lane;
//   WV wavefronts per workgroup, 32 rows each: WV = 8 puts two wavefronts on every SIMD (256 registers each) that share one staged
//   query chunk — one covers the other's LDS / global / barrier waits.
#define BX_KC 32                 // K chunk
#define BX_PITCH 40              // 16-bit elements per staged query row (80 bytes: conflict-free 16-byte reads)

// prefetch registers as first-class vector values: an ARRAY that is live across the chunk loop is left in scratch memory
// by the compiler (12 scratch stores + 12 loads per chunk and lane: 4.5 ms instead of 1.x)
typedef float xf_t __attribute__((ext_vector_type(16)));

// the lane's 16 floats of chunk c; xrow = its (clamped) row + 16 g
__device__ __forceinline__ void load_x(xf_t &xf, const float *xrow, int c)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = *(const float4 *)(xrow + c * BX_KC + 4 * i);
        xf[4 * i] = v.x; xf[4 * i + 1] = v.y; xf[4 * i + 2] = v.z; xf[4 * i + 3] = v.w;
    }
}

// staging of one query chunk, PL planes x NT * 32 queries x 32 elements, by the 64 WV threads of a workgroup: global -> prefetch
// registers (load) -> LDS buffer [PL][NT * 32][BX_PITCH] (store)
template <int PL, int NT, int WV>
struct QStage {
    static constexpr int QROWS = NT * 32;
    static constexpr int BUF = PL * QROWS * BX_PITCH;                       // 16-bit elements of one LDS buffer
    static constexpr int NTHR = 64 * WV;
    static constexpr int NLD = PL * QROWS * 4 / NTHR;                       // 16-byte pieces of a query chunk per thread
    static_assert(PL * QROWS * 4 % NTHR == 0, "query staging plan");
    typedef uint32_t regs_t __attribute__((ext_vector_type(4 * NLD)));

    const uint16_t *qp; int64_t q_plane; int q0, D, tid;
    __device__ __forceinline__ void load(regs_t &qr, int c) const
    {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + NTHR * j, p = i / (QROWS * 4), rem = i - p * (QROWS * 4), q = rem >> 2, part = rem & 3;
            const uint4 v = *(const uint4 *)(qp + (int64_t)p * q_plane + (int64_t)(q0 + q) * D + c * BX_KC + part * 8);
            qr[4 * j] = v.x; qr[4 * j + 1] = v.y; qr[4 * j + 2] = v.z; qr[4 * j + 3] = v.w;
        }
    }
    __device__ __forceinline__ void store(const regs_t &qr, uint16_t *Qs, int buf) const
    {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + NTHR * j, p = i / (QROWS * 4), rem = i - p * (QROWS * 4), q = rem >> 2, part = rem & 3;
            *(uint4 *)&Qs[buf * BUF + (p * QROWS + q) * BX_PITCH + part * 8] = make_uint4(qr[4 * j], qr[4 * j + 1], qr[4 * j + 2], qr[4 * j + 3]);
        }
    }
};

// ---- batched queries on the bf16 matrix cores at f32 accuracy -----------------------------------------------------------
// gfx950 has no TF32.  An f32 value is the exact sum of three bf16 pieces (8 significand bits each: h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m), the differences are exact), so a product x q is the sum of nine piece products; the six of weight >= 2^-16
// (hh, hm, mh, hl, mm, lh) leave a truncation of 2^-24 per product — the rounding an f32 multiply has anyway.  Six bf16 MFMAs at
// 16x the rate replace one f32 MFMA: 0.375x the matrix time, and the scan moves from MFMA-bound (4.1 ms for 256 queries over
// 2^20 x 768) towards its HBM time.  v_mfma_f32_32x32x16_bf16: 12 per tile and chunk, interleaved over the NT independent accumulators.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

__device__ __forceinline__ uint32_t pack_bf16_rne(float lo, float hi)      // v_cvt_pk_bf16_f32
{
    const f32x2_t v = {lo, hi};
    const bf16x2_t r = __builtin_convertvector(v, bf16x2_t);
    return *(const uint32_t *)&r;
}

// (a, b) -> packed bf16 pieces h, m, l of both
__device__ __forceinline__ void split3(float a, float b, uint32_t &h, uint32_t &m, uint32_t &l)
{
    h = pack_bf16_rne(a, b);
    const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
    m = pack_bf16_rne(ra, rb);
    l = pack_bf16_rne(ra - __uint_as_float(m << 16), rb - __uint_as_float(m & 0xffff0000u));
}

// qn (Q, D) f32 -> qp (3, Q, D) bf16 pieces
__global__ __launch_bounds__(TPB) void k_split_q(const float *__restrict__ qn, int64_t n, uint16_t *__restrict__ qp)
{
    const int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 2;
    if (i >= n) return;
    uint32_t h, m, l;
    split3(qn[i], qn[i + 1], h, m, l);
    *(uint32_t *)(qp + i) = h;
    *(uint32_t *)(qp + n + i) = m;
    *(uint32_t *)(qp + 2 * n + i) = l;
}

// SIX: all six products of weight >= 2^-16 (hh, hm, mh, hl, mm, lh: 2^-24 per product, what an f32 multiply rounds away); otherwise
// the three of weight >= 2^-8 (hh, hm, mh): 2^-16 per product term, ~4e-7 on the cosine of unit vectors after the 1/sqrt(D)
// averaging of D independent terms — inside the 2e-6 the tests hold the scan to and 2 500x inside the north star's 1e-3 —
// at half the matrix work and without the l plane of the queries.
template <int NT, int WV, bool SIX>
__global__ __launch_bounds__(64 * WV) void k_cosine_bf16x3(const float *__restrict__ X, int64_t n_rows, int D,
                                                       const uint16_t *__restrict__ qp, int64_t q_plane, int q0, int q_valid,
                                                       float *__restrict__ sims, int64_t sims_stride)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t Qs[];           // [2][3][NT * 32][BX_PITCH]
    typedef QStage<3, NT, WV> QS;
    constexpr int QROWS = QS::QROWS;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = lane & 31, g = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * (32 * WV);
    const int64_t row = row0 + w * 32 + n;
    const int64_t rowc = row < n_rows ? row : n_rows - 1;                  // clamped: results of padded rows are not stored
    const float *xrow = X + rowc * D + g * 16;
    const int nchunks = D / BX_KC;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)           // (not clear_tiles: through it this kernel's register allocation changes)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float nrm = 0.f;
    xf_t xf;
    typename QS::regs_t qr;
    const QS qs{qp, q_plane, q0, D, tid};
    load_x(xf, xrow, 0);
    qs.load(qr, 0);
    qs.store(qr, Qs, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        // this chunk's rows -> bf16 pieces (two sub-steps of 8 floats), then the next chunk's loads go in flight
        uint32_t bh[2][4], bm[2][4], bl[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = make_float4(xf[4 * i], xf[4 * i + 1], xf[4 * i + 2], xf[4 * i + 3]);
            nrm = fmaf(v.x, v.x, nrm); nrm = fmaf(v.y, v.y, nrm); nrm = fmaf(v.z, v.z, nrm); nrm = fmaf(v.w, v.w, nrm);
            split3(v.x, v.y, bh[i >> 1][2 * (i & 1)], bm[i >> 1][2 * (i & 1)], bl[i >> 1][2 * (i & 1)]);
            split3(v.z, v.w, bh[i >> 1][2 * (i & 1) + 1], bm[i >> 1][2 * (i & 1) + 1], bl[i >> 1][2 * (i & 1) + 1]);
        }
        if (c + 1 < nchunks) { load_x(xf, xrow, c + 1); qs.load(qr, c + 1); }
        const uint16_t *qb = &Qs[buf * QS::BUF + n * BX_PITCH + g * 16];
#pragma unroll
        for (int sstep = 0; sstep < 2; ++sstep) {
            const bf16x8_t xh = *(const bf16x8_t *)bh[sstep], xm = *(const bf16x8_t *)bm[sstep], xl = *(const bf16x8_t *)bl[sstep];
            // one piece of the queries at a time (NT fragments live instead of 3 NT): l is used once, m twice, h three times;
            // smallest terms first; consecutive MFMAs go to different accumulators
            bf16x8_t af[NT];
            if (SIX) {
#pragma unroll
                for (int t = 0; t < NT; ++t) af[t] = *(const bf16x8_t *)(qb + (2 * QROWS + t * 32) * BX_PITCH + sstep * 8);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], xh, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) af[t] = *(const bf16x8_t *)(qb + (1 * QROWS + t * 32) * BX_PITCH + sstep * 8);
            if (SIX) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], xm, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], xh, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) af[t] = *(const bf16x8_t *)(qb + (0 * QROWS + t * 32) * BX_PITCH + sstep * 8);
            if (SIX) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], xl, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], xm, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], xh, acc[t], 0, 0, 0);
        }
        if (c + 1 < nchunks) qs.store(qr, Qs, buf ^ 1);
        __syncthreads();
    }
    nrm += __shfl_xor(nrm, 32);
    const float inv = 1.0f / fmaxf(sqrtf(nrm), 1e-8f);
    store_tiles(acc, inv, row, n_rows, g, q0, q_valid, sims, sims_stride);
}

// ---- the same scan on fp16 pieces: three products instead of six -------------------------------------------------------------
// An f32 value is, to 22 significant bits, the sum of TWO fp16 pieces (11 significand bits each): x q = xh qh + xh ql + xl qh +
// O(2^-22 |x q|) — three v_mfma_f32_32x32x16_f16 per product instead of the six bf16 ones above, the same f32 accumulators
// (encoder_gemm.hip runs the encoder's dense layers this way).  What fp16 lacks is range (5 exponent bits), so both operands are
// brought to a fixed magnitude by exact power-of-two scales that leave through the result:
//   queries  unit vectors (k_normalize_q) x 2^11: |element| <= 2048;
//   rows     x s_r with s_r = the power of two that puts the row's NORM in [2^11, 2^12): every element below 4096, the typical
//            one (norm / sqrt(D)) near 2^7; an element 2^10 below the typical one keeps its l piece to an absolute 2^-25 of the
//            scaled row — far below the 2^-22 relative error of the typical term.
// s_r and 1 / (norm s_r 2^11) per row come from k_row_scale, one pass over the rows that is redone only after the rows changed
// (x->row_scale_dirty: ingest, flush, imports, merges, reset) — a loaded memory that is queried many times pays it once.
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
#define FX_QSCALE 2048.0f

__device__ __forceinline__ void split2h(f32x2_t v, uint32_t &h, uint32_t &l)      // 2 x v_cvt_pk_f16_f32 around a packed subtract
{
    const half2_t hv = __builtin_convertvector(v, half2_t);
    h = *(const uint32_t *)&hv;
    const half2_t lv = __builtin_convertvector(v - __builtin_convertvector(hv, f32x2_t), half2_t);
    l = *(const uint32_t *)&lv;
}

// one wavefront per row: rs[row] = (s_r, 1 / (max(norm, 1e-8) s_r 2^11))
__global__ __launch_bounds__(TPB) void k_row_scale(const float *__restrict__ X, int64_t n_rows, int D, float2 *__restrict__ rs)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6;
    if (row >= n_rows) return;
    const float4 *xr = (const float4 *)(X + row * D);
    float a = 0.f;
    for (int k = lane; k < D / 4; k += 64) {
        const float4 v = xr[k];
        a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a); a = fmaf(v.z, v.z, a); a = fmaf(v.w, v.w, a);
    }
    a = wave_sum(a);
    if (lane == 0) rs[row] = bsc_row_scale_of(a);
}

// qn (Q, D) f32 unit rows -> qp (2, Q, D) fp16 pieces of 2^11 qn
__global__ __launch_bounds__(TPB) void k_split_q_f16(const float *__restrict__ qn, int64_t n, uint16_t *__restrict__ qp)
{
    const int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 2;
    if (i >= n) return;
    uint32_t h, l;
    const f32x2_t v = {qn[i] * FX_QSCALE, qn[i + 1] * FX_QSCALE};
    split2h(v, h, l);
    *(uint32_t *)(qp + i) = h;
    *(uint32_t *)(qp + n + i) = l;
}

template <int NT, int WV>
__global__ __launch_bounds__(64 * WV) void k_cosine_f16x2(const float *__restrict__ X, int64_t n_rows, int D,
                                                           const uint16_t *__restrict__ qp, int64_t q_plane, int q0, int q_valid,
                                                           const float2 *__restrict__ rs, float *__restrict__ sims, int64_t sims_stride)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t Qs[];           // [2][2][NT * 32][BX_PITCH]
    typedef QStage<2, NT, WV> QS;
    constexpr int QROWS = QS::QROWS;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = lane & 31, g = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * (32 * WV);
    const int64_t row = row0 + w * 32 + n;
    const int64_t rowc = row < n_rows ? row : n_rows - 1;                  // clamped: results of padded rows are not stored
    const float *xrow = X + rowc * D + g * 16;
    const float2 rsc = rs[rowc];
    const f32x2_t sc2 = {rsc.x, rsc.x};
    const int nchunks = D / BX_KC;
    f32x16 acc[NT];
    clear_tiles(acc);
    xf_t xf;
    typename QS::regs_t qr;
    const QS qs{qp, q_plane, q0, D, tid};
    load_x(xf, xrow, 0);
    qs.load(qr, 0);
    qs.store(qr, Qs, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        // this chunk's rows -> fp16 pieces of s_r x (two sub-steps of 8 floats), then the next chunk's loads go in flight
        uint32_t bh[2][4], bl[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2_t p0 = (f32x2_t){xf[4 * i], xf[4 * i + 1]} * sc2, p1 = (f32x2_t){xf[4 * i + 2], xf[4 * i + 3]} * sc2;
            split2h(p0, bh[i >> 1][2 * (i & 1)], bl[i >> 1][2 * (i & 1)]);
            split2h(p1, bh[i >> 1][2 * (i & 1) + 1], bl[i >> 1][2 * (i & 1) + 1]);
        }
        if (c + 1 < nchunks) { load_x(xf, xrow, c + 1); qs.load(qr, c + 1); }
        const uint16_t *qb = &Qs[buf * QS::BUF + n * BX_PITCH + g * 16];
#pragma unroll
        for (int sstep = 0; sstep < 2; ++sstep) {
            const half8_t xh = *(const half8_t *)bh[sstep], xl = *(const half8_t *)bl[sstep];
            // one piece of the queries at a time; smallest terms first; consecutive MFMAs go to different accumulators
            half8_t af[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) af[t] = *(const half8_t *)(qb + (1 * QROWS + t * 32) * BX_PITCH + sstep * 8);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], xh, acc[t], 0, 0, 0);      // ql xh
#pragma unroll
            for (int t = 0; t < NT; ++t) af[t] = *(const half8_t *)(qb + (0 * QROWS + t * 32) * BX_PITCH + sstep * 8);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], xl, acc[t], 0, 0, 0);      // qh xl
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], xh, acc[t], 0, 0, 0);      // qh xh
        }
        if (c + 1 < nchunks) qs.store(qr, Qs, buf ^ 1);
        __syncthreads();
    }
    store_tiles(acc, rsc.y, row, n_rows, g, q0, q_valid, sims, sims_stride);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// similarity rows of consecutive queries must not sit a power of two apart: a 2^22-byte stride puts the rows that
// are read concurrently (8+ queries in flight) on the same HBM channel / bank set and the candidate passes drop to
// 0.4 TB/s.  Rows are padded to a multiple of 64 floats plus an odd number of 256-byte units.
int64_t sims_row_stride(int64_t n_rows) { return ((n_rows + 63) & ~(int64_t)63) + 64 * 33; }

// the matrix-core kernels read whole query tiles: l_q (1024 rows) is zero-padded up to the next multiple of 256 queries
static int padded_queries(int nq) { return ((nq + 255) / 256) * 256 > 1024 ? 1024 : ((nq + 255) / 256) * 256; }

bsc_status stage_queries(bsc_ctx *x, const float *q_dev, int nq)
{
    const int D = x->c.token_dim;
    BSC_HIP(hipMemsetAsync(x->l_q, 0, sizeof(float) * (size_t)padded_queries(nq) * D, x->stream));
    hipLaunchKernelGGL(k_normalize_q, dim3(nq), dim3(64), 0, x->stream, q_dev, D, x->l_q);
    return BSC_OK;
}

bsc_status refresh_row_scales(bsc_ctx *x, const float *rows, int64_t n_rows, float2 **rs, int64_t *rs_cap, bool *rs_dirty)
{
    const int64_t need = (int64_t)sizeof(float2) * n_rows;
    if (n_rows <= 0 || x->c.token_dim % MF_KC != 0) return BSC_OK;       // cosine_scan stays off the matrix cores then
    if (!*rs_dirty && *rs && *rs_cap >= need) return BSC_OK;
    if (*rs_cap < need) BSC_TRY(mem_grow(x->mem, (void **)rs, rs_cap, sizeof(float2) * (n_rows + n_rows / 8 + 1024), false, "row scales"));
    hipLaunchKernelGGL(k_row_scale, dim3((unsigned)((n_rows * 64 + TPB - 1) / TPB)), dim3(TPB), 0, x->stream, rows, n_rows,
                       x->c.token_dim, *rs);
    *rs_dirty = false;
    return BSC_OK;
}

template <int QT>
static void launch_cosine(bsc_ctx *x, const float *rows, int64_t n_rows, int q0)
{
    const int D = x->c.token_dim;
    const int nv = (D / 4 + 63) / 64;
    int64_t blocks = (n_rows * 64 + TPB - 1) / TPB;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), block(TPB);
#define LC(NV) hipLaunchKernelGGL((k_cosine<NV, QT>), grid, block, 0, x->stream, rows, n_rows, D, x->l_q, q0, x->l_sims, sims_row_stride(n_rows))
    if (nv <= 1) LC(1);
    else if (nv == 2) LC(2);
    else if (nv == 3) LC(3);
    else if (nv == 4) LC(4);
    else LC(8);
#undef LC
}

// one pass of a piece kernel over queries [q0, q0 + 32 NT): WV wavefronts x 32 rows per workgroup, two LDS buffers of PL planes
template <int NT>
static void launch_f16x2(bsc_ctx *x, const float *rows, int64_t n_rows, int64_t nel, int q0, int nq, const float2 *rs)
{
    const size_t lds = (size_t)2 * 2 * (NT * 32) * BX_PITCH * sizeof(uint16_t);
    (void)hipFuncSetAttribute((const void *)k_cosine_f16x2<NT, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_cosine_f16x2<NT, 8>), dim3((unsigned)((n_rows + 255) / 256)), dim3(512), lds, x->stream, rows, n_rows,
                       x->c.token_dim, (const uint16_t *)x->l_qp, nel, q0, nq, rs, x->l_sims, sims_row_stride(n_rows));
}

template <int NT, int WV, bool SIX>
static void launch_bf16x3(bsc_ctx *x, const float *rows, int64_t n_rows, int64_t nel, int q0, int nq)
{
    const size_t lds = (size_t)2 * 3 * (NT * 32) * BX_PITCH * sizeof(uint16_t);
    (void)hipFuncSetAttribute((const void *)k_cosine_bf16x3<NT, WV, SIX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_cosine_bf16x3<NT, WV, SIX>), dim3((unsigned)((n_rows + 32 * WV - 1) / (32 * WV))), dim3(64 * WV), lds,
                       x->stream, rows, n_rows, x->c.token_dim, (const uint16_t *)x->l_qp, nel, q0, nq, x->l_sims,
                       sims_row_stride(n_rows));
}

template <int NT>
static void launch_pieces(bsc_ctx *x, bool bf16, bool wv8, bool six, const float *rows, int64_t n_rows, int64_t nel, int q0, int nq,
                          const float2 *rs)
{
    if (!bf16) launch_f16x2<NT>(x, rows, n_rows, nel, q0, nq, rs);
    else if (wv8 && six) launch_bf16x3<NT, 8, true>(x, rows, n_rows, nel, q0, nq);
    else if (wv8) launch_bf16x3<NT, 8, false>(x, rows, n_rows, nel, q0, nq);
    else if (six) launch_bf16x3<NT, 4, true>(x, rows, n_rows, nel, q0, nq);
    else launch_bf16x3<NT, 4, false>(x, rows, n_rows, nel, q0, nq);
}

template <int NT>
static void launch_mfma(bsc_ctx *x, const float *rows, int64_t n_rows, int q0, int nq)
{
    hipLaunchKernelGGL((k_cosine_mfma<NT>), dim3((unsigned)((n_rows + 127) / 128)), dim3(TPB), 0, x->stream, rows, n_rows,
                       x->c.token_dim, x->l_q, q0, nq, x->l_sims, sims_row_stride(n_rows));
}

bsc_status cosine_scan(bsc_ctx *x, const float *rows, int64_t n_rows, int nq, float2 **rs, int64_t *rs_cap, bool *rs_dirty,
                       int *passes_out)
{
    hipStream_t s = x->stream;
    const int D = x->c.token_dim;
    const dim3 block(TPB);
    int done = 0;
    int passes = 0;                          // times the row matrix is streamed
    if (nq >= BSC_MFMA_MIN_Q && D % MF_KC == 0 && n_rows > 0) {
        // batched queries on the matrix cores, 32-query tiles: more than 64 queries -> 16-bit pieces at f32 accuracy (k_cosine_f16x2,
        // or k_cosine_bf16x3 as its A/B form); up to 64 -> the f32 MFMA, HBM-bound at that size anyway (measured over 2^20 x 768:
        // 33..64 queries 1.17-1.28 ms on bf16 pieces against 1.09 ms on the f32 MFMA)
        static const bool f32_only = getenv("BSC_COSINE_F32") != nullptr;              // A/B: the f32 MFMA scan throughout
        // six piece products (f32 accuracy, the default) or BSC_COSINE_PIECES=3 (hh, hm, mh): 0.7x the scan time, scores within
        // ~4e-6 instead of 3e-7 — enough for the north star's 1e-3, not for the 2e-6 the fp64 parity tests ask; read per call
        const char *pcs = getenv("BSC_COSINE_PIECES");
        const bool six = !(pcs && atoi(pcs) == 3);
        static const bool wv8 = getenv("BSC_COSINE_WV4") == nullptr;                   // A/B: 8 (default) or 4 wavefronts per workgroup of k_cosine_bf16x3
        const bool bf16_pieces = getenv("BSC_COSINE_BF16") != nullptr;                 // A/B (read per call): the six-product bf16 scan
        const int64_t nel = (int64_t)padded_queries(nq) * D;                           // the piece planes lie this far apart
        if (!f32_only && nq > 64) {
            const dim3 sgrid((unsigned)((nel / 2 + TPB - 1) / TPB));
            if (!bf16_pieces) {               // fp16 pieces, three products: per-row scales / inverse norms cached until the rows change
                BSC_TRY(refresh_row_scales(x, rows, n_rows, rs, rs_cap, rs_dirty));
                hipLaunchKernelGGL(k_split_q_f16, sgrid, block, 0, s, x->l_q, nel, x->l_qp);
            } else {
                hipLaunchKernelGGL(k_split_q, sgrid, block, 0, s, x->l_q, nel, x->l_qp);
            }
            for (int left = nq; left > 64; left = nq - done) {      // the remainder (<= 64 queries) goes to the f32 MFMA below
                ++passes;
                if (left > 128) { launch_pieces<8>(x, bf16_pieces, wv8, six, rows, n_rows, nel, done, nq, *rs); done += 256; }
                else { launch_pieces<4>(x, bf16_pieces, wv8, six, rows, n_rows, nel, done, nq, *rs); done += 128; }
            }
        }
        while (done < nq) {
            const int left = nq - done;
            ++passes;
            if (left > 128) { launch_mfma<8>(x, rows, n_rows, done, nq); done += 256; }
            else if (left > 64) { launch_mfma<4>(x, rows, n_rows, done, nq); done += 128; }
            else if (left > 32) { launch_mfma<2>(x, rows, n_rows, done, nq); done += 64; }
            else { launch_mfma<1>(x, rows, n_rows, done, nq); done += 32; }
        }
        done = nq;
    }
    while (done < nq && n_rows > 0) {      // the row matrix is streamed once per group of up to 8 queries
        const int left = nq - done;
        ++passes;
        if (left >= 8) { launch_cosine<8>(x, rows, n_rows, done); done += 8; }
        else if (left >= 4) { launch_cosine<4>(x, rows, n_rows, done); done += 4; }
        else if (left >= 2) { launch_cosine<2>(x, rows, n_rows, done); done += 2; }
        else { launch_cosine<1>(x, rows, n_rows, done); done += 1; }
    }
    *passes_out = passes;
    return BSC_OK;
}
