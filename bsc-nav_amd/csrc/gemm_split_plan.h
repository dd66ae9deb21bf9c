// gemm_split_plan.h — the launch plan of k_gemm_split (encoder_gemm.hip) as plain integer arithmetic: which tile, how the tiles are
// dealt to the persistent workgroups, how many split-K slices, how much LDS — and the lane -> address maps of its main loop (the
// weight image in LDS, the MFMA fragments, the accumulator layout).  No HIP header: tests/host/gemm_plan_main.cpp walks the plans
// on the CPU, tests/host/gemm_frag_main.cpp the maps.  gs_tile_of is the one definition of "which tile is entry qv of an XCD's
// list", gs_dma_* / gs_frag_off / gs_acc_* of "which byte goes where" — the kernel calls them too.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD inline
#endif

#define GS_KC 32                 // K chunk
#define GS_PITCH 40              // fp16 elements per weight row of the few-rows tile, which stages its weights through registers (80 bytes)
#define GS_LDS_MAX (160 * 1024)

enum { GS_EPI_BIAS = 0, GS_EPI_GELU = 1, GS_EPI_RESID = 2, GS_EPI_GELU_ERF = 3 };
enum { GS_A_F32 = 0, GS_A_PIECES = 1, GS_A_LN = 2 };

// Width of the half tile that a short last round is split into, 0 where the shape has none (its weight staging plan must exist).
// NT column tiles per wavefront, WR x WC wavefronts: the template arguments of k_gemm_split.
GS_HD constexpr int gs_half_cols(int NT, int WR, int WC)
{
    return (NT % 2 == 0 && (WC * (NT / 2) * 32) % (16 * WR * WC) == 0) ? WC * (NT / 2) * 32 : 0;
}

struct GsPlan {
    int tile;                    // 1: 256 x 256 (k_gemm_split<1, 8, 8, 1>), 3: 128 x 128 (<1, 4, 4, 1>), 6: 32 x 128 (<1, 1, 1, 4>)
    int rows, cols, threads;     // of a tile / a workgroup
    int half_cols;               // gs_half_cols of the tile
    int64_t n_pad;               // N rounded up to the 256 rows the weight planes are padded to
    int n_tiles_n;
    int64_t n_tiles_m;
    int64_t q_full, q_virtual;   // entries of an XCD's tile list: the first q_full are whole tiles, the rest half tiles
    int64_t per_round;           // workgroups per XCD = the stride of a workgroup through its XCD's list
    int64_t n_wg;
    int64_t lds_loop, lds_epi, lds;      // bytes: weight buffers, the wavefronts' epilogue blocks, all with the bias row
    int S, k_len;                // split-K slices (grid.y) and the columns each contracts
};

struct GsTile { int64_t tm; int n0; bool half, valid; };

// Entry qv of the tile list of XCD xcd.  XCD k takes the row tiles k, k + 8, ... and all column tiles of one before the next; the
// entries from q_full on are pairs of half-width tiles (cols, half_cols: columns of a whole and of a half tile).
GS_HD GsTile gs_tile_of(int n_tiles_n, int64_t n_tiles_m, int64_t q_full, int64_t q_virtual, int cols, int half_cols, int xcd, int64_t qv)
{
    GsTile t;
    t.half = half_cols != 0 && qv >= q_full;
    const int64_t qt = t.half ? q_full + ((qv - q_full) >> 1) : qv;
    t.tm = (qt / n_tiles_n) * 8 + xcd;
    t.n0 = (int)(qt % n_tiles_n) * cols + (t.half ? (int)((qv - q_full) & 1) * half_cols : 0);
    t.valid = qv < q_virtual && t.tm < n_tiles_m;
    return t;
}

// ---- the LDS weight image and the fragment maps of the DMA-scheduled tiles (every tile but the few-rows one) -----------------------
// v_mfma_f32_16x16x32_f16 with the weights as the first operand (D' = W X^T): lane l = (i = l & 15, g = l >> 4) holds, of a 16-row
// weight tile, row i and the chunk's halfs [8 g, 8 g + 8) — one 16-byte column of a 64-byte LDS row —, of the activations the same
// eight k of rows i and i + 16 of the wavefront's 32, and of the accumulator tile (row half, tile) ROW 16 half + i of C and the four
// consecutive columns 16 tile + 4 g + (0..3).  tests/host/gemm_frag_main.cpp composes these maps on the CPU; the kernel calls them.
//
// The image: [gs_w_ring buffers][2 pieces][wrows rows][4 columns of 16 bytes], one chunk per buffer (buf = 0 .. gs_w_ring - 1 in
// gs_dma_lds_off / gs_frag_off; chunk c of a tile sits in buffer (first + c) % gs_w_ring).  A DMA instruction of a wavefront lands in lane
// order (16 rows x 64 bytes), so the swizzle is applied to the SOURCE column: slot (row, c) holds global column c ^ gs_w_swz(row).
// A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): four blocks
// of four rows, two of them at g and two at g + 1.  A 256-byte bank window is four rows, so the four blocks must sit in four different
// columns: with q = (row >> 2) & 3 the groups hold {q 0, 3 at g; q 1, 2 at g ^ 1} or {q 1, 2 at g; q 0, 3 at g ^ 1}, and
// s = {0, 3, 2, 1} separates both (the plain s = q of the 32-row fragment of v_mfma_f32_32x32x16 does not: 0 ^ s[0] = 1 ^ s[1]).
//
// Weight buffers of a workgroup of nthr threads.  The 256-row tiles (512 threads, one workgroup per CU; whole and half width) keep a
// ring of THREE: the buffer of chunk c + 2 was last read in chunk c - 1, whose closing barrier every wavefront has passed, so chunk
// c may request c + 2 anywhere — the kernel does it behind its last fragment read, off the chunk's top where all eight wavefronts
// wait for their first fragments — and the request has all of chunk c + 1 to land.  The 128 x 128 tile keeps two (requested at the
// chunk's top, one ahead): a third would put it at 81 KB with the bias row of N = 4096, one workgroup per CU where the plan launches
// two.  (The few-rows tile stages through registers into two buffers of its own pitch.)
GS_HD constexpr int gs_w_ring(int nthr) { return nthr == 512 ? 3 : 2; }
// the ring of three: the buffer of the chunk after the one in buf, and of the chunk before it — where the chunk two ahead goes
GS_HD constexpr int gs_ring_next(int buf) { return buf == 2 ? 0 : buf + 1; }
GS_HD constexpr int gs_ring_prev(int buf) { return buf == 0 ? 2 : buf - 1; }
GS_HD constexpr int gs_w_swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }
GS_HD constexpr int gs_w_col(int row, int c) { return c ^ gs_w_swz(row); }         // slot -> global column and back (an involution)
// DMA plan of a workgroup of nthr threads for a chunk of wrows rows per piece: instruction j of thread tid moves 16 bytes
GS_HD constexpr int gs_dma_count(int wrows, int nthr) { return 2 * wrows * 4 / nthr; }
GS_HD constexpr int gs_dma_piece(int wrows, int nthr, int j) { return j / (wrows / (nthr / 4)); }
GS_HD constexpr int gs_dma_row(int wrows, int nthr, int j, int tid) { return (j % (wrows / (nthr / 4))) * (nthr / 4) + (tid >> 2); }
GS_HD constexpr int gs_dma_src_col(int tid) { return gs_w_col(tid >> 2, tid & 3); }                  // (nthr / 4 is a multiple of 16)
// byte offsets into the image: where instruction j of a WAVEFRONT's lane 0 lands (lane l: + 16 l), and what a lane reads
GS_HD constexpr int gs_w_buf_bytes(int wrows) { return 2 * wrows * GS_KC * 2; }
GS_HD constexpr int gs_dma_lds_off(int wrows, int nthr, int buf, int j, int wave)
{
    return buf * gs_w_buf_bytes(wrows) + (gs_dma_piece(wrows, nthr, j) * wrows + gs_dma_row(wrows, nthr, j, 64 * wave)) * (GS_KC * 2);
}
GS_HD constexpr int gs_frag_off(int wrows, int buf, int piece, int strip_row0, int tile, int lane)
{
    return buf * gs_w_buf_bytes(wrows) + (piece * wrows + strip_row0 + 16 * tile + (lane & 15)) * (GS_KC * 2) + 16 * gs_w_col(lane & 15, lane >> 4);
}
// accumulator register r of tile (half, tile) of lane -> (row, column) of the wavefront's 32 x NT 32 strip
GS_HD constexpr int gs_acc_row(int lane, int half) { return 16 * half + (lane & 15); }
GS_HD constexpr int gs_acc_col(int lane, int tile, int r) { return 16 * tile + 4 * (lane >> 4) + r; }

// The plan of C (M, N) = A (M, K) W^T.  c_pieces: C leaves as pieces; ln_bufs: the caller gave both LayerNorm buffers (statistics
// records and means); stats: the residual epilogue leaves the row statistics; ws_bytes: the caller's workspace for split-K partial
// results (0: none); n_cu: compute units of the device.  false + *why: the arguments break a rule of the kernel.
inline bool gs_plan(int64_t M, int K, int N, int epilogue, int a_mode, bool c_pieces, bool ln_bufs, bool stats, int64_t ws_bytes,
                    int n_cu, GsPlan *plan, const char **why)
{
    *why = nullptr;
    const bool ln = a_mode == GS_A_LN;
    if (M <= 0 || N <= 0 || K <= 0 || (K % GS_KC) || epilogue < 0 || epilogue > 3 || a_mode < 0 || a_mode > 2 || (c_pieces && (N % 32)))
        *why = "bsc_enc_gemm_split: invalid argument (K must be a multiple of 32; piece output needs N % 32 == 0)";
    else if (epilogue == GS_EPI_RESID && c_pieces)
        *why = "bsc_enc_gemm_split: the residual epilogue writes f32";
    else if ((ln || stats) && !ln_bufs)
        *why = "bsc_enc_gemm_split_ln: the LayerNorm modes need both ln_stats_dev and ln_mu_dev";
    else if (ln && (K % 128 || K > 1024 || epilogue == GS_EPI_RESID || !c_pieces))
        // (an f32-output form was measured and dropped: fc1 2 497 -> 2 687 us, its epilogue holds the tile twice)
        *why = "bsc_enc_gemm_split_ln: a_mode 2 reads rows of width K = 128 .. 1024 (multiple of 128) and writes pieces (epilogue 0 / 1)";
    else if (stats && (N % 128 || N > 1024 || ln))
        *why = "bsc_enc_gemm_split_ln: row statistics ride on the residual epilogue of a GEMM with N = 128 .. 1024 (multiple of 128)";
    if (*why) return false;
    // Tile shape: 256 x 256 (8 wavefronts x 32 rows x 256 columns) — unless there are few rows (a frame or a handful per call:
    // M = 197 .. ~3 500): 256-row tiles leave N / 256 = 3 .. 12 workgroups on 256 CUs and a forward of ONE frame took 6 ms (3x
    // PyTorch's f32 GEMMs).  Tile 6 = 32 rows x 128 columns, four wavefronts side by side on the columns (each 32 x 32): 60 KB of
    // LDS, two or three workgroups per CU cover each other's chunk latency (a 32-row tile has 6 MFMAs per chunk to hide a weight
    // chunk's round trip behind).  While even those tiles do not fill the chip, K is split over grid.y: every slice writes an f32
    // partial result, k_splitk_finish adds them in slice order (deterministic) and applies the epilogue.  Per flop the small tile
    // moves 8x the weight bytes through LDS, so it is taken only while the big tiles would not fill the chip once.  (LayerNorm-in-
    // the-load and the statistics epilogue exist for the big tile only: callers with few rows use the LayerNorm pass.)
    const int64_t big_tiles = ((M + 255) / 256) * ((N + 255) / 256);
    const bool few_rows = !(ln || stats) && big_tiles <= n_cu && M <= 8192;
    // (32-row tiles re-read the weights once per 32 rows: from ~500 rows on the launch is bound by that L2 traffic — 4.6 TB/s at
    //  1 576 rows — and 128 x 128 tiles, 4 wavefronts x 32 rows x 128 columns, take over, with the same split-K)
    GsPlan p;
    p.tile = !few_rows ? 1 : M <= 512 ? 6 : 3;
    const int NT = p.tile == 1 ? 8 : p.tile == 3 ? 4 : 1, WR = p.tile == 1 ? 8 : p.tile == 3 ? 4 : 1, WC = p.tile == 6 ? 4 : 1;
    p.rows = WR * 32;
    p.cols = WC * NT * 32;
    p.threads = 64 * WR * WC;
    p.half_cols = gs_half_cols(NT, WR, WC);
    p.n_pad = ((int64_t)N + 255) / 256 * 256;
    p.n_tiles_n = (int)(p.n_pad / p.cols);
    p.n_tiles_m = (M + p.rows - 1) / p.rows;
    const int64_t groups = (p.n_tiles_m + 7) / 8;                   // row tiles per XCD
    // persistent workgroups: one per CU; the 60 KB few-rows tiles two per CU
    const int64_t q_all = groups * p.n_tiles_n;
    p.per_round = (p.tile == 1 ? 1 : 2) * (n_cu / 8 > 0 ? n_cu / 8 : 1);
    // a last round that fills at most half of the CUs runs as half-width tiles (tile 1 only): N = 768 at 384 frames is 888 tiles
    // on 256 CUs, 3.47 rounds — that round then costs half a tile's time instead of a whole one
    const int64_t q_rem = q_all % p.per_round;
    p.q_full = (p.tile == 1 && q_rem > 0 && 2 * q_rem <= p.per_round && q_all > p.per_round) ? q_all - q_rem : q_all;
    p.q_virtual = p.q_full + 2 * (q_all - p.q_full);
    p.n_wg = (p.q_virtual < p.per_round ? p.q_virtual : p.per_round) * 8;
    // [buffers][2 pieces][cols][pitch] fp16: three buffers of 32 KB for the 256 x 256 tile (with 34 KB of epilogue blocks and at most
    // 16 KB of bias row 146 KB), two for the others
    p.lds_loop = (int64_t)gs_w_ring(p.threads) * 2 * p.cols * (p.tile == 6 ? GS_PITCH : GS_KC) * 2;
    p.lds_epi = (int64_t)(p.threads / 64) * (32 * 136);            // the epilogue's per-wavefront tile blocks
    p.lds = p.lds_loop + p.lds_epi + p.n_pad * 4;                   // + the bias row
    if (p.lds > GS_LDS_MAX) { *why = "bsc_enc_gemm_split: N does not fit the kernel's LDS plan (bias row)"; return false; }
    // split-K of the few-rows tiles: the largest slice count that keeps the launch within two workgroups per CU, slices of whole
    // chunks, at least two chunks each
    p.S = 1;
    static const int cand[] = {24, 16, 12, 8, 6, 4, 3, 2};
    auto slices_ok = [&](int c) { return K % (GS_KC * c) == 0 && K / c >= 2 * GS_KC; };
    if (few_rows && (N % 4) == 0)
        for (int c : cand)
            if (slices_ok(c) && p.n_tiles_m * p.n_tiles_n * c <= 2 * (int64_t)n_cu) { p.S = c; break; }
    // the f32 partial results live in the caller's workspace (stream-ordered, capture-safe: the library allocates nothing); a
    // workspace that is absent or too small means fewer slices
    while (p.S > 1 && (int64_t)p.S * M * N * 4 > ws_bytes) {
        int fewer = 1;
        for (int c : cand)
            if (c < p.S && slices_ok(c)) { fewer = c; break; }
        p.S = fewer;
    }
    p.k_len = K / p.S;
    *plan = p;
    return true;
}
