// bsc_internal.h — shared declarations of libbscnav.so (gfx950 only; no CPU path).
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscnav.h"
#include "ctx_mem.h"

typedef unsigned long long u64;
// per-point payload of the rgb chain: one 12-byte gather per point
struct PointRec {
    uint32_t alo, ahi; // exp(-r^2 / 1.2) as a double, low / high word   (memory_2.py:875)
    uint32_t rgbv;     // rgb[py, px] packed r | g << 8 | b << 16   (memory_2.py:870)
};
#define BSC_EV_RING 512
// timed stages (bsc_kernel_stats `which`)
enum {
    BSC_STAT_DENSE = 0,    // k_dense_reduce
    BSC_STAT_COSINE = 1,   // cosine scan of bsc_localize / bsc_localize_regions (bytes: the rows actually streamed)
    BSC_STAT_POINTS = 2,   // k_points
    BSC_STAT_PAIRS = 3,    // k_keys_pairs + tile scan + k_pair_compact
    BSC_STAT_ORDER = 4,    // new-voxel ids, k_run_keys, run sort, scan, k_expand, segment order (everything the rgb chain needs)
    BSC_STAT_PAIRSORT = 5, // pair sort + segment heads
    BSC_STAT_INGEST = 6,   // main-stream work of one bsc_ingest call, first to last kernel
    BSC_STAT_CHAIN = 7,    // k_chain + k_hwin (side stream)
    BSC_STAT_SLOTS = 8
};

// device scalar block indices (int64 each)
enum {
    DS_MAX_ID = 0,      // number of voxel ids assigned so far (memory_2.py max_id)
    DS_MAX_ID_PREV = 1, // max_id before the batch in flight (voxels >= this are new in the batch)
    DS_NPASS_TOTAL = 2, // points that passed all checks since creation
    DS_NSEEN_TOTAL = 3,
    DS_POOL_N = 4,      // rows used in the token pool (exact mode)
    DS_ERROR = 5,       // sticky device-side error flag (capacity)
    DS_B_NPASS = 6,     // batch: passing points
    DS_B_NFIRST = 7,    // batch: first-touch points (= new voxels)
    DS_N_HITS = 8,      // flush: rows that met a full voxel
    DS_B_NSEG = 9,      // batch: voxel segments in the sorted point list
    DS_RMW_TOTAL = 10,  // dense: voxel rows read-modify-written since creation
    DS_B_NPAIR = 11,    // batch: unique (voxel, frame, patch) pairs emitted by the tiles
    DS_TMP0 = 12,       // bsc_counters scratch (store voxels / tokens)
    DS_TMP1 = 13,
    DS_B_NPSEG = 14,    // batch: voxel segments of the sorted pair list
    DS_PAIR_TOTAL = 15, // dense: pairs reduced since creation
    DS_B_NRUN = 16,     // batch: runs of consecutive points that fall into the same cell
    DS_B_NNEW = 17,     // batch: cells listed as new by their first claimer (== new voxels; before the capacity clip)
    DS_COUNT = 18
};

// workspace of the in-tree radix sort (radix.hip), one per stream that sorts
struct RadixWs {
    u64 *status;               // per tile and digit: epoch << 32 | state << 30 | count
    uint32_t *partial;         // histogram partials of the workgroups of k_radix_hist
    uint32_t *gpartial;        // ... added up per group of 32 workgroups
    uint32_t *goff;            // (4, 256) exclusive digit offsets of the passes
    uint32_t *tickets;         // [0] k_radix_hist's last-group ticket, [1 + p] the tile ticket of pass p, [8 + g] the ticket of group g
    uint32_t *tmp_k, *tmp_v;   // intermediate passes
    size_t max_items;
    uint32_t epoch;            // host counter: one value per (sort, pass)
};

// the scratch a call shares with its rgb chain, double-buffered: the chain of call n reads set n & 1 on the side stream while
// call n + 1 fills the other
struct IngestSet {
    PointRec *p_rec;                // read by the rgb chain on the side stream
    uint32_t *skey_b;               // sorted run keys
    uint32_t *sval_b;               // point order: j of the k-th point, voxel by voxel — written only where the quad chain reads it
                                    // (short segments, the first points of new voxels: k_expand_short)
    // the point order by RUNS (read by k_chain_long): position k belongs to the run whose start is the last set bit at or below k
    u64 *run_bits;                  // bit k: a run starts at position k
    uint32_t *ck_run, *ck_start;    // per 64 positions: the sorted run that covers position 64 w, and where it starts
    uint32_t *run_val;              // sorted run values (first record of the run)
    int4 *seg_info;                 // per voxel segment: {first k, end k, voxel id, rank in the length-class order}
    int32_t *seg_last;
    int64_t *bscal;                 // per-set scalars: [0] voxel segments of the batch, [1] max_id before the batch
    bool rec8;                      // record format of the call in this set (its chain is launched later)
    hipEvent_t ev_ready, ev_done;   // side: the set's point order is complete; its chain is done with the set
    bool ev_done_valid;
};

struct SurpriseWs;   // surprise.hip: scratch of bsc_flush_surprise, allocated on its first call
struct RegionWs;     // localize.hip: scratch of bsc_localize_regions, allocated on its first call
struct ClusterWs;    // cluster.hip: inputs, result block and pinned staging of bsc_cluster_centers(_batch), grown on demand

struct bsc_ctx {
    BscMem *mem;               // owns every device / pinned-host buffer below (ctx_mem.h): created first, released last
    bsc_config c;
    int device;
    hipStream_t stream;
    int nh;
    int64_t ncell;
    int g2;
    // ---- persistent state in HBM ----
    int32_t *occ;      // (gs,gs,nh) voxel id or -1 (memory_2.py occupied_ids)
    int32_t *rgb_pos;  // (vcap+1,3)
    uint8_t *rgb;      // (vcap,3)
    float *weight;     // (vcap)
    u64 *hmap;         // (gs,gs) packed (h+1)<<40 | order  (max_height + tie order)
    uint8_t *cv_map;   // (gs,gs,3)
    // fast geometry (geometry_dev.h geom_point_fast): pinhole intrinsics + per-pixel patch tables, verified at creation
    bool geom_fast;
    bool proj_id;              // K Kinv p2d == p2d up to rounding and min_depth >= 0: source pixel without the division (GeomConst.proj_id)
    bool pat_all_in;           // no pixel centre outside the patch grid: the every-pixel dense build needs no patch-table look-ups
    bool long_chain;           // segments of >= 64 points go to the wavefront-per-voxel chain (BSC_QUAD_CHAIN_ONLY unsets)
    // 8-byte point records for the every-pixel dense build (geometry_dev.h rec8_*): possible when float_as_uint over the valid
    // depth range (min_depth, max_depth) spans fewer than 2^28 values (BSC_REC12=1 keeps the 12-byte {alpha, rgb} records)
    bool rec8_ok;
    uint32_t rec8_zbase;       // bits of the largest float <= min_depth
    uint32_t dbg_paths;        // BSC_DEBUG: the {fast, plain, rec8} choices of ingest_front_end already reported on stderr
    uint8_t *pat_x, *pat_y;   // (W), (H): patch column / row of a pixel column / row, 255 = outside the patch grid
    double *exp_tab;          // 64 x (hi, lo) of 2^(j/64): the table of bsc_exp (geometry_dev.h)
    // patch-aligned pair tiles (dense.hip): pixel rectangle {x0, width, y0, pixels} of every patch and the start of its
    // staging slice inside a frame; valid when every patch covers at most 3328 pixels
    bool patch_tiles;
    int32_t *pt_rect, *pt_off;
    int pair_path;            // how the pairs of the batch in flight were built: 0 generic tiles, 1 patch tiles
    int64_t *dscal;    // DS_COUNT device scalars
    int64_t *hscal;    // pinned host mirror for readbacks
    int64_t *mail, *mail_dev;  // DS_COUNT scalars + a sequence number, in coherent pinned host memory: written by k_block_totals, polled by
    int64_t mail_seq;          // the host (ingest_batch) — no event / copy / synchronize between the front end and the order stage
    // exact mode
    float *cache_f;     // (iter_size,D)
    int32_t *cache_pos; // (iter_size,3)
    float *cache_d;     // (iter_size)
    int64_t iter_id;    // host mirror of the cache fill
    float *pool;        // (token_capacity,D)
    float *pool_d;      // (token_capacity)
    int32_t *store_rows; // (vcap+1,cache_size) pool rows; entry vcap is the grid_0_0_0 group
    int32_t *store_cnt;  // (vcap+1)
    int64_t n_flush;
    int64_t pool_n_host;   // host mirror of DS_POOL_N (token pool rows in use), exact after every flush / import / compaction / reset
    // the flush bsc_ingest runs when a passing point meets a full cache (bsc_set_flush_policy; configuration: bsc_reset keeps it)
    int32_t flush_policy, fp_radius;
    double fp_sthr, fp_bthr;
    // compaction scratch, kept and grown on demand (store_compact.hip): row marks, block totals / offsets, holes, movers, remap
    void *cp_buf[6];
    int64_t cp_cap[6];       // bytes
    int64_t cp_runs, cp_rows_moved, cp_usec;   // compactions that moved rows, rows moved, host time spent in them (bsc_compact_stats)
    // dense modes
    float *acc;   // (vcap,D)
    int32_t *acnt; // (vcap)
    // point log for the exact colour merge across ranks (bsc_point_log_*): cells + records of every ingested point
    int32_t *log_cell;
    PointRec *log_rec;
    int64_t log_cap, log_n;
    bool log_stale;            // the colour state was imported / replaced while the log was on: the log no longer describes it
    // ---- per-batch scratch (max_points) ----
    int32_t *p_cell;
    uint32_t *p_patf;
    float *p_r2f;
    // Points are ordered per voxel through their RUNS (maximal stretches of consecutive points in one cell; a 10 cm
    // voxel a few metres away covers ~16 pixels of an image row): the runs are sorted by voxel id (stable radix sort
    // keeps the order j inside a voxel) and expanded back into the per-voxel point order the rgb chain walks.
    int32_t *new_cells;                 // cells claimed for the first time in this batch (one entry per new voxel)
    int32_t *blk_cnt, *blk_off;         // per 1024-point block: runs (count / exclusive prefix); also head compaction
    int32_t *blk_pass, *blk_pass_off;   // per block: passing points
    int32_t *hb_cnt, *hb_off;           // segment-head compaction (dense.hip compact_heads): per-block counts / offsets
    int64_t nblk_cap;
    uint32_t *stage_cell, *stage_pos;   // k_points: the runs of every block of points (cell, first position), slice b * GB
    int group_rpw;                      // rounds of 64 points per wavefront in k_points: 4 (1024-point blocks) or 8 (2048; BSC_GROUP_RPW)
    uint32_t *skey_a, *sval_a;          // run sort input: key = voxel id | (length - 1) << id bits, value = first point
    uint32_t *run_val_b;                // sorted run values
    int64_t *run_scan;                  // per 1024-run block: sum, then exclusive prefix, of (length | segment head << 32)
    int32_t *seg_k0, *seg_vid;          // voxel segments of the point order: first position, voxel id
    u64 *f_keys_a, *f_keys_b;  // flush-private sort buffers (iter_size)
    int32_t *pass_list;
    IngestSet set[2];
    int cur_set;
    hipStream_t side;          // rgb chain + top-down map run here, overlapped with the dense reduce / next encoder
    hipStream_t side2;         // the one-wavefront segments of the long chain, beside the hot tiles on `side`
    hipEvent_t ev_chain0, ev_mid;
    struct {
        bool pending;          // the last call's rgb chain / top-down map kernels are still to be launched (deferred)
        int set;
        int64_t order_base;
        int64_t points;        // points of the batch whose chain is pending
    } chain;
    int last_chain_set;        // scratch set of the most recently launched chain (-1: none since the last reset)
    u64 *pair_key_a, *pair_key_b;   // dense: voxel id << cb | frame << pb | patch
    u64 *pstage_key;                // per-tile staging of the LDS-aggregated pairs
    uint32_t *pstage_cnt;
    int32_t *tile_cnt, *tile_off;
    int64_t max_tiles;
    uint32_t *pair_cnt_a, *pair_cnt_b;
    int32_t *pseg_start;
    int64_t pair_cap;
    double *d_transforms; // (max_frames,16)
    int64_t *d_offsets;   // (max_frames+1)
    int max_frames;
    // flush scratch (iter_size)
    int32_t *f_rowdst, *f_hit, *f_hidx, *f_rowseg, *f_rowe, *f_headpos, *f_win;
    uint32_t *f_draws;
    int64_t draws_cap;
    SurpriseWs *surp;          // surprise flush scratch (nullptr until the first bsc_flush_surprise)
    // localize scratch
    float *l_sims;       // per token row / voxel row
    int64_t l_sims_cap, l_out_pos_cap, l_out_sim_cap;   // bytes
    u64 *l_key_a, *l_key_b;
    uint32_t *l_val_a, *l_val_b;
    uint32_t *l_name_rank;
    float *l_q;          // normalised queries
    uint16_t *l_qp;      // their 16-bit pieces, planes of (padded queries, D): two fp16 (k_cosine_f16x2) or three bf16 (k_cosine_bf16x3)
    u64 *l_sel_key[2];   // batched top-K selection rounds (grown on demand)
    uint32_t *l_sel_val[2];
    u64 *l_sel_thr;      // per-query threshold keys of the sample selection
    int32_t *l_sel_cnt;  // per-query survivor counts
    uint32_t *l_valid;   // one bit per dense row: the row holds points (what the filter needs of acnt)
    int64_t l_sel_cap[7];
    int32_t *l_out_pos;
    float *l_out_sim;
    bool names_dirty;
    // per-row operand scale + inverse norm of the rows the batched fp16-piece scan reads (dense rows or token-pool rows), rebuilt —
    // like the name ranks — only after the rows changed (ingest, flush, imports, merges, reset)
    float2 *l_rscale;
    int64_t l_rscale_cap;
    bool row_scale_dirty;
    bool rscale_from_reduce;        // the last ingest's dense reduce wrote the scale / inverse norm of every row it finished
                                    // (k_dense_reduce_voxels): the scan's k_row_scale pass is then only needed after imports
    int last_nq, last_K;            // shape of the last bsc_localize / bsc_localize_regions call (its top-K stays resident for clustering)
    RegionWs *regn;                 // bsc_localize_regions scratch (nullptr until its first call)
    int32_t last_counts[1024];
    u64 *sm_map;                    // bsc_score_map scratch: packed (score, height) keys of one chunk of queries (score_map.hip)
    int64_t sm_cap;                 // bytes
    u64 *td_mask;                   // bsc_topdown_* scratch: column occupancy bits, (gs, gs, ceil(nh / 64)), then the call's bands (topdown.hip)
    int64_t td_cap;                 // bytes
    u64 *rv_words;                  // bsc_render_views scratch: occupancy bits per 4 x 4 x 4 brick, then the call's transforms (render.hip)
    int64_t rv_cap;                 // bytes
    ClusterWs *clus;                // bsc_cluster_centers / bsc_cluster_centers_batch workspace (nullptr until the first call)
    // frontier helpers (allocated on first use, gs*gs each)
    bool fr_ready;             // all of them exist (frontier.hip fr_alloc)
    uint8_t *fr_mask, *fr_in;
    int32_t *fr_parent, *fr_size, *fr_ord, *fr_roots, *fr_labels, *fr_first, *fr_sizes, *fr_scal;
    unsigned long long *fr_sumx, *fr_sumy;
    double *fr_centers, *fr_gains;
    // primitives workspace
    void *prim_tmp;
    size_t prim_tmp_bytes;
    void *prim_tmp_side;       // second rocPRIM workspace: the order pipeline sorts on the side stream beside the pair sort
    RadixWs rx_main, rx_side;  // in-tree radix sort: the pair sort (main stream) and the run sort (side stream) may run at the same time
    bool radix_intree;         // BSC_SORT_ROCPRIM=1: both sorts through rocPRIM as until round 5
    bool order_on_side;        // per-voxel point order (k_run_keys .. k_expand_short) on the side stream (BSC_ORDER_MAIN=1 keeps it on the main stream)
    hipEvent_t ev_ids, ev_runs;   // voxel ids assigned; side: k_run_keys / k_pass_list have read the call's cells / block offsets
    hipEvent_t ev_tot;            // main: k_block_totals done (the call's run / new-voxel counts exist)
    hipEvent_t ev_psort;          // main: the pair sort of the last call is done (the rgb chain starts behind it, launch_pending_chain)
    bool ev_psort_valid;
    hipStream_t copy;             // early readback of those counts while the main stream goes on with the pair tiles
    void *h2d_pin[4];             // pinned staging of the pageable-host imports (capi.hip h2d_pipelined), allocated on first use
    hipEvent_t h2d_ev[4];
    bool h2d_ready;               // all four buffers and events exist
    bool ev_runs_valid;
    int last_order_set;        // scratch set of the last order stage enqueued on the side stream (-1: none): its ev_ready marks it complete
    // bookkeeping
    int64_t order_base; // global point counter (top-down map tie order)
    // HIP-event rings around the stages of the path (BSC_STAT_*), recorded on the stream the stage is launched on
    hipEvent_t ev[BSC_STAT_SLOTS][2 * BSC_EV_RING];
    int ev_n[BSC_STAT_SLOTS];
    double stat_bytes[BSC_STAT_SLOTS];
    bool timing;
};

#define BSC_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            bsc_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return BSC_E_HIP;                                                                  \
        }                                                                                      \
    } while (0)
#define BSC_TRY(expr)                 \
    do {                              \
        bsc_status _s = (expr);       \
        if (_s != BSC_OK) return _s;  \
    } while (0)

// current device ordinal and its CU count (cached per ordinal; kernel attributes and the persistent grids are per device)
inline bsc_status gs_device(int *dev, int *n_cu)
{
    static int cus[64] = {0};
    BSC_HIP(hipGetDevice(dev));
    int &c = cus[*dev & 63];
    if (!c) BSC_HIP(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, *dev));
    *n_cu = c;
    return BSC_OK;
}

// sum of v over the wavefront's 64 lanes, in every lane (xor butterfly, distances 32 .. 1)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums of two per-thread ints over the workgroup's NT threads, exclusive per thread: (ea, eb), totals (ta, tb); one call per kernel
template <int NT>
__device__ __forceinline__ void block_scan2(int a, int b, int &ea, int &eb, int &ta, int &tb)
{
    __shared__ int s_a[NT / 64], s_b[NT / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ua = __shfl_up(ia, o), ub = __shfl_up(ib, o);
        if (lane >= o) { ia += ua; ib += ub; }
    }
    if (lane == 63) { s_a[wv] = ia; s_b[wv] = ib; }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int va = s_a[w], vb = s_b[w];
        ba += w < wv ? va : 0; bb += w < wv ? vb : 0;
        ta += va; tb += vb;
    }
    ea = ba + ia - a;
    eb = bb + ib - b;
}

// ---- primitives (prims.hip: rocPRIM device-wide sort and scans; radix.hip: the in-tree sort) ----
// where a primitive runs: its stream and the workspaces that belong to that stream
struct PrimLane { hipStream_t stream; void *tmp; size_t tmp_bytes; RadixWs *rx; };
static inline PrimLane lane_main(bsc_ctx *x) { return {x->stream, x->prim_tmp, x->prim_tmp_bytes, &x->rx_main}; }
static inline PrimLane lane_side(bsc_ctx *x) { return {x->side, x->prim_tmp_side, x->prim_tmp_bytes, &x->rx_side}; }
size_t prim_workspace_bytes(size_t max_items);
bsc_status prim_sort_keys(const PrimLane &l, const u64 *in, u64 *out, size_t n, int begin_bit, int end_bit);
bsc_status prim_sort_pairs(const PrimLane &l, const u64 *kin, u64 *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                           int begin_bit, int end_bit);
bsc_status prim_sort_pairs_onesweep(const PrimLane &l, const u64 *kin, u64 *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                                    int begin_bit, int end_bit);
bsc_status prim_sort_pairs_u32(const PrimLane &l, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout,
                               size_t n, int begin_bit, int end_bit);
bsc_status prim_sort_pairs_u32_onesweep(const PrimLane &l, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout,
                                        size_t n, int begin_bit, int end_bit);
// in-tree onesweep radix sort of (u32 key, u32 value) pairs on the key bits [b0, b1): stable, input preserved (radix.hip)
bsc_status radix_ws_create(BscMem *m, RadixWs *ws, size_t max_items);      // the buffers are the ledger's
bsc_status radix_sort_pairs_u32(const PrimLane &l, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                                int b0, int b1);
// the (u32, u32) pair sort of the pipeline: in-tree radix, or rocPRIM under BSC_SORT_ROCPRIM=1 (onesweep: its one-sweep form)
static inline bsc_status sort_pairs_u32(const bsc_ctx *x, const PrimLane &l, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
                                        uint32_t *vout, size_t n, int b0, int b1, bool onesweep = false)
{
    if (x->radix_intree) return radix_sort_pairs_u32(l, kin, kout, vin, vout, n, b0, b1);
    return onesweep ? prim_sort_pairs_u32_onesweep(l, kin, kout, vin, vout, n, b0, b1) : prim_sort_pairs_u32(l, kin, kout, vin, vout, n, b0, b1);
}
bsc_status prim_exclusive_sum_i64(const PrimLane &l, const int64_t *in, int64_t *out, size_t n);
bsc_status prim_exclusive_sum_i32(const PrimLane &l, const int32_t *in, int32_t *out, size_t n);
bsc_status prim_inclusive_max_i32(const PrimLane &l, const int32_t *in, int32_t *out, size_t n);

// ---- kernels launchers ----
bsc_status launch_geometry_debug(bsc_ctx *x, const float *depth, const int32_t *idx, int64_t P, uint8_t *flags,
                                 double *pc, double *pg, int32_t *vox, int32_t *pix, int32_t *pat, double *r2,
                                 double *alpha);
// token rows come as f32 (the reference's DINOv2 output) or as bf16 (what a bf16 encoder emits; widened exactly)
typedef uint16_t bf16_t;
__device__ __forceinline__ float4 load_tok4(const float *row, int v) { return ((const float4 *)row)[v]; }
__device__ __forceinline__ float4 load_tok4(const bf16_t *row, int v)
{
    const uint2 raw = ((const uint2 *)row)[v];
    return make_float4(__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u),
                       __uint_as_float(raw.y << 16), __uint_as_float(raw.y & 0xffff0000u));
}

// (power-of-two operand scale, 1 / (norm scale 2^11)) of a token row from the sum of its squares: what the fp16-piece batched scan
// (cosine_scan.hip k_cosine_f16x2) reads per row; computed by k_row_scale (one pass over the rows) and, row by row, by the dense reduce
__device__ __forceinline__ float2 bsc_row_scale_of(float sumsq)
{
    const float nrm = sqrtf(sumsq);
    int e = 0;
    if (nrm > 0.f && nrm < INFINITY) (void)frexpf(nrm, &e);          // nrm = m 2^e, m in [0.5, 1)
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    const float sc = (nrm > 0.f && nrm < INFINITY) ? ldexpf(1.0f, 12 - e) : 1.0f;     // norm * sc in [2^11, 2^12)
    // the result leaves as acc * (1 / (sc 2^11)) / max(norm, 1e-8): the two powers of two are exact factors
    return make_float2(sc, (1.0f / fmaxf(nrm, 1e-8f)) / sc * (1.0f / 2048.0f));
}

bsc_status ingest_batch(bsc_ctx *x, int32_t n_frames, const float *depth, const uint8_t *rgb, int32_t rgb_ch,
                        const void *tokens, int token_dtype, const int32_t *idx, const int64_t *offsets_host,
                        const double *alpha, bsc_draw_fn draw, void *user);
bsc_status flush_cache(bsc_ctx *x, bsc_draw_fn draw, void *user);
bsc_status grow_token_pool(bsc_ctx *x, int64_t need_rows);
// room for n more pool rows before a flush changes anything: dead rows are reclaimed first (BSC_STORE_COMPACT=auto), the pool
// grows only when the live rows + n still exceed it (store_compact.hip)
bsc_status reserve_pool_rows(bsc_ctx *x, int64_t n);
// the live rows (sum of store_cnt) to pool rows [0, live), DS_POOL_N = live; live_known < 0: counted here (store_compact.hip)
bsc_status compact_store_impl(bsc_ctx *x, int64_t live_known, int64_t *rows_before, int64_t *rows_after);
bool store_compact_auto();                  // BSC_STORE_COMPACT != never, read per call
// store voxels / live tokens (sums over store_cnt or acnt) -> dscal[DS_TMP0 / DS_TMP1], enqueued on the main stream (capi.hip)
bsc_status enqueue_store_totals(bsc_ctx *x);
// the argument checks bsc_flush_surprise and bsc_set_flush_policy share (surprise.hip); `who` names the caller in the message
bsc_status surprise_check_args(const bsc_ctx *x, const char *who, int32_t radius, double surprise_threshold, double boring_threshold);
// update_memory_surp_base (surprise.hip): every iter_size row, tasks level by level; clears the cache like flush_cache
bsc_status surprise_flush(bsc_ctx *x, int32_t radius, double surprise_threshold, double boring_threshold);
bsc_status import_cache_impl(bsc_ctx *x, int64_t n_rows, const int32_t *pos_host, const float *feat_host, const float *dis_host);
bsc_status launch_pending_chain(bsc_ctx *x);
bsc_status launch_keys_pairs(bsc_ctx *x, int64_t P, int n_frames, bool all_pixels, const uint32_t *p_patf);
bsc_status frontier_mask_impl(bsc_ctx *x, const uint8_t *navigable_host, uint8_t *mask_host);
bsc_status frontier_clusters_impl(bsc_ctx *x, const uint8_t *frontier_host, int32_t min_cluster_size, int32_t ig_radius,
                                  int32_t max_clusters, int32_t *n_clusters_host, int32_t *labels_host,
                                  int32_t *first_host, int32_t *sizes_host, double *centers_host, double *gains_host,
                                  int32_t *best_host);
bsc_status dense_reduce_batch(bsc_ctx *x, const void *tokens, int token_dtype, int n_frames);
// list of segment starts of a sorted key array (segments = runs of equal key >> shift; keys == invalid are skipped);
// the number of segments is written to *count_dev.  Deterministic: per-block counts + exclusive scan.
bsc_status compact_heads_u64(bsc_ctx *x, const u64 *keys, int64_t n, int shift, int32_t *out, int64_t *count_dev);
bsc_status localize_impl(bsc_ctx *x, const float *q_dev, int32_t nq, int32_t K, double radius, const int32_t *curr,
                         int32_t floor_lo, int32_t floor_hi, int32_t *out_pos, float *out_sim, int32_t *out_count);
bsc_status localize_regions_impl(bsc_ctx *x, const float *q_dev, int32_t nq, int32_t K, const bsc_region *regions,
                                 int32_t *out_pos, float *out_sim, int32_t *out_count);
// The front half of bsc_localize_regions, which bsc_score_map shares (localize.hip; RegionScan: localize_cand.h): region staging,
// the visibility pass, the pruning decision, the row gather and the cosine scan of nq queries -> x->l_sims and the candidate list
// (RegionCandArgs) that reads it.  regions == nullptr: no region for any query.
struct RegionScan;
BSC_LOCAL bsc_status region_scan(bsc_ctx *x, const float *q_dev, int32_t nq, const bsc_region *regions, RegionScan *out);
// bsc_score_map behind its argument checks (score_map.hip)
bsc_status score_map_impl(bsc_ctx *x, const float *q_dev, int32_t nq, const bsc_region *regions, float *score_dev, int32_t *height_dev);
// bsc_topdown_slices / bsc_topdown_rebuild behind their argument checks (topdown.hip): n_bands slices of the stored voxels into the
// outputs given (device pointers, any may be null; hmap_out: the packed word of x->hmap).  bands_host == nullptr: one open band.
bsc_status topdown_impl(bsc_ctx *x, int32_t n_bands, const bsc_band *bands_host, uint8_t *rgb_out, int32_t *height_out,
                        int32_t *count_out, u64 *hmap_out);
// bsc_render_views behind its argument checks (render.hip): kinv is the matrix to use, band_host may be null (every height), the
// outputs are device pointers (any may be null)
bsc_status render_impl(bsc_ctx *x, int32_t n_views, const double *transforms_host, const double *kinv, int32_t height, int32_t width,
                       double t_min, double t_max, const bsc_band *band_host, int32_t *voxel_out, float *depth_out, uint8_t *rgb_out);
// ---- the cosine scan (cosine_scan.hip), as localize.hip calls it ----
int64_t sims_row_stride(int64_t n_rows);   // floats between the similarity rows of consecutive queries
// q_dev (nq, D) -> x->l_q: normalised, zero-padded to the whole query tiles the matrix-core kernels read
BSC_LOCAL bsc_status stage_queries(bsc_ctx *x, const float *q_dev, int nq);
// rs / rs_cap / rs_dirty: the cached per-row scales of THESE rows for the fp16-piece scan (the context's own for its store, a
// scratch set for a gathered matrix); grown and recomputed (k_row_scale) when the rows changed or the buffer is too small.
// Nothing to do without rows or when token_dim rules the matrix-core scan out.
BSC_LOCAL bsc_status refresh_row_scales(bsc_ctx *x, const float *rows, int64_t n_rows, float2 **rs, int64_t *rs_cap, bool *rs_dirty);
// The scan of nq staged queries (x->l_q) over the matrix rows (n_rows, D) -> x->l_sims, query rows sims_row_stride(n_rows)
// apart.  *passes_out = times the matrix was streamed.
BSC_LOCAL bsc_status cosine_scan(bsc_ctx *x, const float *rows, int64_t n_rows, int nq, float2 **rs, int64_t *rs_cap, bool *rs_dirty,
                                 int *passes_out);
bsc_status pool_query_impl(bsc_ctx *x, const float *tokens, int32_t B, int32_t T, int32_t D, float *out);
bsc_status read_scalars(bsc_ctx *x); // dscal -> hscal (synchronises the main stream)
void localize_prepare(bsc_ctx *x);   // name ranks + row scales of the batched scan, eagerly (localize.hip; the imports call it)
bsc_status sync_all(bsc_ctx *x);     // main + side stream
// record the start / stop event of launch number ev_n[which] (ring; older launches are overwritten)
static inline void stat_begin(bsc_ctx *x, int which, hipStream_t s = nullptr)
{
    if (x->timing) (void)hipEventRecord(x->ev[which][2 * (x->ev_n[which] % BSC_EV_RING)], s ? s : x->stream);
}
static inline void stat_end(bsc_ctx *x, int which, double bytes, hipStream_t s = nullptr)
{
    if (x->timing) {
        (void)hipEventRecord(x->ev[which][2 * (x->ev_n[which] % BSC_EV_RING) + 1], s ? s : x->stream);
        x->ev_n[which]++;
        x->stat_bytes[which] += bytes;
    }
}

static inline int ceil_log2_u64(uint64_t v)
{
    int b = 0;
    while ((1ull << b) < v) ++b;
    return b;
}
