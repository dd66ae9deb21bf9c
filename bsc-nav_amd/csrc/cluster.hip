// cluster.hip — the step right after localize: GESObjectNavRobot.weighted_cluster_centers (BSCAgent.py:479-497), for one
// query (bsc_cluster_centers) or for every query of a localize batch in one launch (bsc_cluster_centers_batch: what
// working_memory_retrival, BSCAgent.py:587-664, and the three-radius loop, :1078-1098, ask for).
//
// DBSCAN(eps, min_samples) over the K top-ranked voxel positions, similarity-weighted cluster centres, clusters
// ordered by mean similarity.  K is ~100, so one workgroup per query does it out of LDS and the "query -> goal position"
// chain never leaves the GPU.  scikit-learn grows clusters depth-first from unlabelled core points in index order; that
// order-defined result has a closed form which is what the kernel evaluates in parallel:
//   core(i)    = |{ j : d(i,j) <= eps }| >= min_samples            (the point counts itself)
//   component  = connected components of the core points under d <= eps (min-label propagation)
//   label      = rank of the component by its smallest core index  (= order in which sklearn seeds clusters)
//   border     = non-core point with a core neighbour: the smallest label among them (the cluster expanded first
//                claims it); no core neighbour -> noise (-1)
// Up to CL_BITN points the neighbour predicate is evaluated once per ordered pair: the adjacency is kept as bit rows in
// LDS (a row = four 64-bit words, one wavefront ballot each) and core counts, propagation and border points read the
// bits.  Above that the predicate is recomputed where it is needed.  Both forms use the same predicate and reach the same
// fixed point (every core point carries the smallest core index of its component), so the labels cannot differ.
#include "bsc_internal.h"

#include <math.h>
#include <stdlib.h>

#define CL_TPB 256
#define CL_MAXK 1024
#define CL_MAXQ 1024
#define CL_BITN 256          // points up to which the bit-row form runs (= CL_TPB: thread i owns row i)
#define CL_NONE 0x7fffffff

// One workgroup per query (blockIdx.x).  Query q reads its n points from pos / sim at row q (rows `row_stride` points
// apart); n = counts[q], or n_fixed when counts is NULL, clamped to 0 .. K.  It writes row q of the result block:
// centers (K,3) f64 and sizes (K) with the rows from n_clusters on zero, labels (K) with -1 from n on, n_clusters.
// LDS, static, both forms together: px py pz 12288 + sim 4096 + comp 4096 + lab 4096 + core 1024 + avg 8192 + bit rows
// 8192 + core mask 32 + root mask 128 + 4 = 42148 bytes, 42152 allocated (the recompute form leaves the 8224 bytes of bit
// rows / core mask unused); no dynamic LDS.  62 VGPRs, no scratch.
__global__ __launch_bounds__(CL_TPB) void k_cluster_batch(const int32_t *__restrict__ pos, const float *__restrict__ sim,
                                                          int64_t row_stride, const int32_t *__restrict__ counts, int n_fixed,
                                                          int K, int bit_max, double eps2, int min_samples,
                                                          double *__restrict__ centers, int32_t *__restrict__ labels_out,
                                                          int32_t *__restrict__ sizes, int32_t *__restrict__ n_clusters)
{
    __shared__ int32_t px[CL_MAXK], py[CL_MAXK], pz[CL_MAXK];
    __shared__ float ps[CL_MAXK];
    __shared__ int32_t comp[CL_MAXK], lab[CL_MAXK];
    __shared__ uint8_t core[CL_MAXK];
    __shared__ double avg[CL_MAXK];
    __shared__ u64 adj[CL_BITN * 4];             // bit j of adj[4 i + (j >> 6)]: d(i, j) <= eps
    __shared__ u64 cmask[4];                     // core points (bit form)
    __shared__ u64 rmask[CL_MAXK / 64];          // component roots
    __shared__ int changed;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = counts ? counts[q] : n_fixed;
    n = n < 0 ? 0 : (n > K ? K : n);
    pos += (int64_t)q * row_stride * 3;
    sim += (int64_t)q * row_stride;
    centers += (int64_t)q * K * 3;
    labels_out += (int64_t)q * K;
    sizes += (int64_t)q * K;
    if (n == 0) {                                // an empty region: the empty row, nothing else
        for (int i = tid; i < K; i += CL_TPB) {
            labels_out[i] = -1; sizes[i] = 0;
            centers[3 * i] = 0.0; centers[3 * i + 1] = 0.0; centers[3 * i + 2] = 0.0;
        }
        if (tid == 0) n_clusters[q] = 0;
        return;
    }
    for (int i = tid; i < n; i += CL_TPB) { px[i] = pos[3 * i]; py[i] = pos[3 * i + 1]; pz[i] = pos[3 * i + 2]; ps[i] = sim[i]; }
    __syncthreads();
    auto near = [&](int i, int j) {
        const double dx = px[i] - px[j], dy = py[i] - py[j], dz = pz[i] - pz[j];
        return dx * dx + dy * dy + dz * dz <= eps2;
    };
    const bool bits = n <= bit_max;              // uniform over the workgroup
    u64 row[4] = {0, 0, 0, 0};                   // bit form: the core neighbours of point tid
    if (bits) {
        const bool have = tid < n;
        const int nw = (n + 63) >> 6;            // 64-bit words of a row in use
        if (wave < nw)                           // lane j = tid against every i: one ballot is one word of row i
            for (int i = 0; i < n; ++i) {
                const u64 m = __ballot(have && near(i, tid));
                if (lane == 0) adj[4 * i + wave] = m;
            }
        __syncthreads();
        int cnt = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            row[w] = (have && w < nw) ? adj[4 * tid + w] : 0;
            cnt += __popcll(row[w]);
        }
        const bool is_core = have && cnt >= min_samples;
        const u64 cm = __ballot(is_core);
        if (lane == 0) cmask[wave] = cm;
        core[tid] = is_core;
        comp[tid] = is_core ? tid : CL_NONE;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) row[w] &= cmask[w];
        for (int it = 0; it < n; ++it) {        // min-label propagation over the core graph, on the bit rows
            if (tid == 0) changed = 0;
            __syncthreads();
            if (is_core) {
                int m = comp[tid];
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    for (u64 b = row[w]; b; b &= b - 1) m = min(m, comp[64 * w + __ffsll((unsigned long long)b) - 1]);
                m = min(m, comp[m]);             // a core point of the same component: its label is one too
                if (m < comp[tid]) { comp[tid] = m; changed = 1; }
            }
            __syncthreads();
            const int c = changed;
            __syncthreads();
            if (!c) break;
        }
    } else {
        for (int i = tid; i < n; i += CL_TPB) {
            int cnt = 0;
            for (int j = 0; j < n; ++j) cnt += near(i, j) ? 1 : 0;
            core[i] = cnt >= min_samples;
            comp[i] = core[i] ? i : CL_NONE;
        }
        __syncthreads();
        for (int it = 0; it < n; ++it) {        // min-label propagation over the core graph
            if (tid == 0) changed = 0;
            __syncthreads();
            for (int i = tid; i < n; i += CL_TPB) {
                if (!core[i]) continue;
                int m = comp[i];
                for (int j = 0; j < n; ++j)
                    if (core[j] && near(i, j)) m = min(m, comp[j]);
                if (m < comp[i]) { comp[i] = m; changed = 1; }
            }
            __syncthreads();
            const int c = changed;
            __syncthreads();
            if (!c) break;
        }
    }
    // component roots (comp[i] == i) ranked by index = sklearn's cluster numbering
    const int nw64 = (n + 63) >> 6;
    for (int r = 0; r * CL_TPB < n; ++r) {
        const int i = tid + r * CL_TPB;
        const u64 m = __ballot(i < n && core[i] && comp[i] == i);
        if (lane == 0) rmask[4 * r + wave] = m;
    }
    __syncthreads();
    int nl = 0;
    for (int w = 0; w < nw64; ++w) nl += __popcll(rmask[w]);
    for (int i = tid; i < n; i += CL_TPB) {
        int r = -1;
        if (core[i] && comp[i] == i) {
            r = __popcll(rmask[i >> 6] & ((1ull << (i & 63)) - 1));
            for (int w = 0; w < (i >> 6); ++w) r += __popcll(rmask[w]);
        }
        lab[i] = r;                              // label of a root, -1 otherwise
    }
    __syncthreads();
    int fl[CL_MAXK / CL_TPB];                    // final labels of the points tid, tid + 256, ...
#pragma unroll
    for (int r = 0; r < CL_MAXK / CL_TPB; ++r) {
        const int i = tid + r * CL_TPB;
        int l = -1;
        if (i < n) {
            if (core[i]) {
                l = lab[comp[i]];                // roots keep theirs; other cores read their root's label
            } else if (bits) {                   // labels rise with the root's index: the smallest root is the smallest label
                int m = CL_NONE;
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    for (u64 b = row[w]; b; b &= b - 1) m = min(m, comp[64 * w + __ffsll((unsigned long long)b) - 1]);
                if (m != CL_NONE) l = lab[m];
            } else {
                for (int j = 0; j < n; ++j)
                    if (core[j] && near(i, j)) {
                        const int lj = lab[comp[j]];
                        l = (l < 0 || lj < l) ? lj : l;
                    }
            }
        }
        fl[r] = l;
    }
    __syncthreads();                             // comp and lab have been read: comp <- final labels, lab <- cluster sizes
#pragma unroll
    for (int r = 0; r < CL_MAXK / CL_TPB; ++r) {
        const int i = tid + r * CL_TPB;
        if (i < n) { comp[i] = fl[r]; labels_out[i] = fl[r]; }
    }
    for (int i = n + tid; i < K; i += CL_TPB) labels_out[i] = -1;
    __syncthreads();
    // BSCAgent.py:484-491 — per cluster: np.average(points, weights=sim), np.mean(sim), size (index order sums)
    double cx[CL_MAXK / CL_TPB], cy[CL_MAXK / CL_TPB], cz[CL_MAXK / CL_TPB];
#pragma unroll
    for (int r = 0; r < CL_MAXK / CL_TPB; ++r) {
        const int l = tid + r * CL_TPB;
        cx[r] = cy[r] = cz[r] = 0.0;
        if (l < nl) {
            double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
            int c = 0;
            for (int i = 0; i < n; ++i)
                if (comp[i] == l) {
                    const double w = (double)ps[i];
                    sw += w; sx += px[i] * w; sy += py[i] * w; sz += pz[i] * w;
                    ++c;
                }
            avg[l] = sw / c;
            lab[l] = c;
            cx[r] = sx / sw; cy[r] = sy / sw; cz[r] = sz / sw;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CL_MAXK / CL_TPB; ++r) {  // :493 stable descending sort by mean similarity
        const int l = tid + r * CL_TPB;
        if (l < nl) {
            int rank = 0;
            for (int m = 0; m < nl; ++m) rank += (avg[m] > avg[l] || (avg[m] == avg[l] && m < l)) ? 1 : 0;
            centers[3 * rank] = cx[r]; centers[3 * rank + 1] = cy[r]; centers[3 * rank + 2] = cz[r];
            sizes[rank] = lab[l];
        }
    }
    for (int l = nl + tid; l < K; l += CL_TPB) {
        sizes[l] = 0;
        centers[3 * l] = 0.0; centers[3 * l + 1] = 0.0; centers[3 * l + 2] = 0.0;
    }
    if (tid == 0) n_clusters[q] = nl;
}

// ---- host side: everything a call needs lives in the context and grows on demand (no allocator call once it is large
// enough); the results of all queries come back as one block through pinned memory -----------------------------------------
struct ClusterWs {
    int32_t *pos;        // host form: (Q,K,3)
    float *sim;          // host form: (Q,K)
    int32_t *cnt;        // (CL_MAXQ) points per query
    char *out;           // result block: centers (Q,K,3) f64 | labels (Q,K) | sizes (Q,K) | n_clusters (Q)
    char *out_pin;       // the same block in pinned host memory
    int32_t *cnt_pin;    // (CL_MAXQ) pinned staging of the counts a resident call derives
    int64_t pos_cap, sim_cap, out_cap, out_pin_cap;   // bytes
};

static bsc_status cluster_ws_get(bsc_ctx *x, ClusterWs **out)
{
    if (!x->clus) {
        ClusterWs *w = (ClusterWs *)calloc(1, sizeof(ClusterWs));
        if (!w) { bsc_set_error("bsc_cluster_centers: out of host memory"); return BSC_E_HIP; }
        const uint64_t mark = mem_mark(x->mem);
        bsc_status st = mem_alloc(x->mem, (void **)&w->cnt, sizeof(int32_t) * CL_MAXQ, "bsc_cluster_centers counts");
        if (st == BSC_OK) st = mem_alloc_pinned(x->mem, (void **)&w->cnt_pin, sizeof(int32_t) * CL_MAXQ, MEM_PIN_DEFAULT, "bsc_cluster_centers pinned counts");
        if (st != BSC_OK) { mem_release_to(x->mem, mark); free(w); return st; }
        x->clus = w;                          // published once both exist: a failed first call leaves it null
    }
    *out = x->clus;
    return BSC_OK;
}

// Q queries of row length K.  pos_host / sim_host given: uploaded (one copy each); otherwise the rows of d_pos / d_sim,
// `stride` points apart.  cnt_host (pageable or pinned) NULL: every query has K points.  The arguments are valid.
static bsc_status cluster_run(bsc_ctx *x, int Q, int K, const int32_t *pos_host, const float *sim_host, const int32_t *d_pos,
                              const float *d_sim, int64_t stride, const int32_t *cnt_host, double eps, int min_samples,
                              double *centers_host, int32_t *labels_host, int32_t *sizes_host, int32_t *n_clusters_host)
{
    BSC_HIP(hipSetDevice(x->device));
    hipStream_t s = x->stream;
    ClusterWs *w;
    BSC_TRY(cluster_ws_get(x, &w));
    const int64_t QK = (int64_t)Q * K;
    const int64_t off_lab = (int64_t)sizeof(double) * 3 * QK, off_siz = off_lab + (int64_t)sizeof(int32_t) * QK,
                  off_ncl = off_siz + (int64_t)sizeof(int32_t) * QK, total = off_ncl + (int64_t)sizeof(int32_t) * Q;
    const char *what = "bsc_cluster_centers workspace";      // grown with 25 % slack (nothing is in flight: every call ends with a synchronize)
    if (w->out_cap < total) BSC_TRY(mem_grow(x->mem, (void **)&w->out, &w->out_cap, total + total / 4, false, what));
    if (w->out_pin_cap < total) BSC_TRY(mem_grow(x->mem, (void **)&w->out_pin, &w->out_pin_cap, total + total / 4, true, what));
    if (pos_host) {
        const int64_t pos_bytes = (int64_t)sizeof(int32_t) * 3 * QK, sim_bytes = (int64_t)sizeof(float) * QK;
        if (w->pos_cap < pos_bytes) BSC_TRY(mem_grow(x->mem, (void **)&w->pos, &w->pos_cap, pos_bytes + pos_bytes / 4, false, what));
        if (w->sim_cap < sim_bytes) BSC_TRY(mem_grow(x->mem, (void **)&w->sim, &w->sim_cap, sim_bytes + sim_bytes / 4, false, what));
        BSC_HIP(hipMemcpyAsync(w->pos, pos_host, sizeof(int32_t) * 3 * QK, hipMemcpyHostToDevice, s));
        BSC_HIP(hipMemcpyAsync(w->sim, sim_host, sizeof(float) * QK, hipMemcpyHostToDevice, s));
        d_pos = w->pos; d_sim = w->sim; stride = K;
    }
    if (cnt_host) BSC_HIP(hipMemcpyAsync(w->cnt, cnt_host, sizeof(int32_t) * Q, hipMemcpyHostToDevice, s));
    // BSC_CLUSTER_BITROWS=0: the recompute form for every size (A/B timing of the two forms; same results)
    const char *knob = getenv("BSC_CLUSTER_BITROWS");
    const int bit_max = (knob && knob[0] == '0') ? 0 : CL_BITN;
    hipLaunchKernelGGL(k_cluster_batch, dim3((unsigned)Q), dim3(CL_TPB), 0, s, d_pos, d_sim, stride,
                       cnt_host ? (const int32_t *)w->cnt : (const int32_t *)nullptr, K, K, bit_max, eps * eps, min_samples,
                       (double *)w->out, (int32_t *)(w->out + off_lab), (int32_t *)(w->out + off_siz), (int32_t *)(w->out + off_ncl));
    BSC_HIP(hipGetLastError());
    BSC_HIP(hipMemcpyAsync(w->out_pin, w->out, (size_t)total, hipMemcpyDeviceToHost, s));
    BSC_HIP(hipStreamSynchronize(s));
    memcpy(centers_host, w->out_pin, (size_t)off_lab);
    memcpy(labels_host, w->out_pin + off_lab, sizeof(int32_t) * (size_t)QK);
    memcpy(sizes_host, w->out_pin + off_siz, sizeof(int32_t) * (size_t)QK);
    memcpy(n_clusters_host, w->out_pin + off_ncl, sizeof(int32_t) * (size_t)Q);
    return BSC_OK;
}

extern "C" bsc_status bsc_cluster_centers(bsc_ctx *x, int32_t query_index, int32_t K, const int32_t *pos_host,
                                          const float *sim_host, double eps, int32_t min_samples, double *centers_host,
                                          int32_t *labels_host, int32_t *sizes_host, int32_t *n_clusters_host)
{
    if (!x || !centers_host || !labels_host || !sizes_host || !n_clusters_host || K < 1 || K > CL_MAXK || min_samples < 1) {
        bsc_set_error("bsc_cluster_centers: invalid argument (1 <= K <= %d)", CL_MAXK);
        return BSC_E_INVALID;
    }
    if (pos_host) {
        if (!sim_host) { bsc_set_error("bsc_cluster_centers: sim_host missing"); return BSC_E_INVALID; }
        return cluster_run(x, 1, K, pos_host, sim_host, nullptr, nullptr, K, nullptr, eps, min_samples, centers_host, labels_host,
                           sizes_host, n_clusters_host);
    }
    // top-K of the last bsc_localize call, still resident in HBM
    if (query_index < 0 || query_index >= x->last_nq || K > x->last_counts[query_index]) {
        bsc_set_error("bsc_cluster_centers: query %d with %d results is not in the last bsc_localize call", query_index, K);
        return BSC_E_INVALID;
    }
    return cluster_run(x, 1, K, nullptr, nullptr, x->l_out_pos + (int64_t)query_index * x->last_K * 3,
                       x->l_out_sim + (int64_t)query_index * x->last_K, x->last_K, nullptr, eps, min_samples, centers_host,
                       labels_host, sizes_host, n_clusters_host);
}

extern "C" bsc_status bsc_cluster_centers_batch(bsc_ctx *x, int32_t n_queries, int32_t K, const int32_t *counts_host,
                                                const int32_t *pos_host, const float *sim_host, double eps, int32_t min_samples,
                                                double *centers_host, int32_t *labels_host, int32_t *sizes_host,
                                                int32_t *n_clusters_host)
{
    if (!x || !centers_host || !labels_host || !sizes_host || !n_clusters_host) {
        bsc_set_error("bsc_cluster_centers_batch: NULL context or output array");
        return BSC_E_INVALID;
    }
    if (n_queries < 1 || n_queries > CL_MAXQ || K < 1 || K > CL_MAXK || min_samples < 1 || eps != eps) {
        bsc_set_error("bsc_cluster_centers_batch: n_queries=%d (1..%d), K=%d (1..%d), min_samples=%d (>= 1), eps=%g", n_queries,
                      CL_MAXQ, K, CL_MAXK, min_samples, eps);
        return BSC_E_INVALID;
    }
    if ((pos_host == nullptr) != (sim_host == nullptr)) {
        bsc_set_error("bsc_cluster_centers_batch: pos_host and sim_host go together (both NULL: the resident results)");
        return BSC_E_INVALID;
    }
    if (pos_host) {
        for (int i = 0; counts_host && i < n_queries; ++i)
            if (counts_host[i] < 0 || counts_host[i] > K) {
                bsc_set_error("bsc_cluster_centers_batch: counts[%d] = %d outside 0..%d", i, counts_host[i], K);
                return BSC_E_INVALID;
            }
        return cluster_run(x, n_queries, K, pos_host, sim_host, nullptr, nullptr, K, counts_host, eps, min_samples, centers_host,
                           labels_host, sizes_host, n_clusters_host);
    }
    if (x->last_nq < 1 || n_queries != x->last_nq || K > x->last_K) {
        bsc_set_error("bsc_cluster_centers_batch: %d queries x %d results do not match the last localize call (%d x %d)", n_queries,
                      K, x->last_nq, x->last_K);
        return BSC_E_INVALID;
    }
    for (int i = 0; i < n_queries; ++i) {
        const int have = x->last_counts[i] < K ? x->last_counts[i] : K;
        if (counts_host && (counts_host[i] < 0 || counts_host[i] > have)) {
            bsc_set_error("bsc_cluster_centers_batch: counts[%d] = %d, query %d has %d results (K = %d)", i, counts_host[i], i,
                          x->last_counts[i], K);
            return BSC_E_INVALID;
        }
    }
    BSC_HIP(hipSetDevice(x->device));
    ClusterWs *w;
    BSC_TRY(cluster_ws_get(x, &w));
    for (int i = 0; i < n_queries; ++i)
        w->cnt_pin[i] = counts_host ? counts_host[i] : (x->last_counts[i] < K ? x->last_counts[i] : K);
    return cluster_run(x, n_queries, K, nullptr, nullptr, x->l_out_pos, x->l_out_sim, x->last_K, w->cnt_pin, eps, min_samples,
                       centers_host, labels_host, sizes_host, n_clusters_host);
}
