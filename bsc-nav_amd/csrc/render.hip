// render.hip — bsc_render_views: the stored voxels seen from a camera pose, the inverse of bsc_ingest (utils.py:153-214 depth2pc /
// transform_pc / base_pos2grid_id_3d, memory_2.py:859-875,755-756).  Per pixel the first stored voxel its ray meets, how far along
// the ray (the depth z of depth2pc), and its colour.  The rule and the traversal are in ray_walk.h.
//
//   k_rv_bricks    one thread per voxel id < max_id: one 64-bit atomicOr of bit (r&3)<<4 | (c&3)<<2 | (h&3) into the word of the
//                  voxel's 4 x 4 x 4 brick, ceil(gs/4)^2 ceil(nh/4) words — 2 MB at 256^3, 25 MB at 1000^2 x 200: it stays in L2 / the
//                  infinity cache where occ (67 / 800 MB) does not.  OR does not care about arrival order.  Built once per call,
//                  whatever the number of views.
//   k_rv_cast      one thread per pixel, a wavefront per 8 x 8 pixel tile of one view (its 64 rays walk the same bricks): rw_first_hit
//                  over the brick words in f64; occ is read once per ray, at the hit, for the id, then rgb[id].
// The words, then the call's transforms, are scratch of the context.
#include "bsc_internal.h"
#include "ray_walk.h"

#define TPB 256

__global__ __launch_bounds__(TPB) void k_rv_bricks(int64_t n, const int32_t *__restrict__ pos, RwGrid G, u64 *__restrict__ words)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int32_t r = pos[3 * i], c = pos[3 * i + 1], h = pos[3 * i + 2];
    if (r < 0 || c < 0 || h < 0 || r >= G.n[0] || c >= G.n[1] || h >= G.n[2]) return;      // (no state the library builds has such a row)
    atomicOr(words + rw_word_of(G, r, c, h), 1ull << rw_bit_of(r, c, h));
}

struct RvKinv { double m[9]; };

// grid (ceil(W / 32), ceil(H / 8), views), 256 threads: wavefront w of a block has the 8 x 8 tile at x = 32 bx + 8 w, y = 8 by
__global__ __launch_bounds__(TPB) void k_rv_cast(RwGrid G, const u64 *__restrict__ words, const double *__restrict__ transforms, RvKinv K,
                                                 int H, int W, double t_min, double t_max, const int32_t *__restrict__ occ,
                                                 const uint8_t *__restrict__ rgb, int64_t max_id, int32_t *__restrict__ out_voxel,
                                                 float *__restrict__ out_depth, uint8_t *__restrict__ out_rgb)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = (blockIdx.x * 4 + wv) * 8 + (lane & 7), y = blockIdx.y * 8 + (lane >> 3);
    if (x >= W || y >= H) return;
    const double *T = transforms + 16 * (int64_t)blockIdx.z;
    double o[3], d[3];
    rw_ray(T, K.m, x, y, o, d);
    const RwHit hit = rw_first_hit(G, (const uint64_t *)words, o, d, t_min, t_max);
    int32_t id = -1;
    if (hit.cell[0] >= 0) {
        id = occ[((int64_t)hit.cell[0] * G.n[1] + hit.cell[1]) * G.n[2] + hit.cell[2]];
        if (id < 0 || id >= max_id) id = -1;                    // (the cell of a set bit names its voxel in every state the library builds)
    }
    const int64_t p = ((int64_t)blockIdx.z * H + y) * W + x;
    if (out_voxel) out_voxel[p] = id;
    if (out_depth) out_depth[p] = id >= 0 ? (float)hit.t : 0.f;
    if (out_rgb) {
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (id >= 0) { c0 = rgb[3 * (int64_t)id]; c1 = rgb[3 * (int64_t)id + 1]; c2 = rgb[3 * (int64_t)id + 2]; }
        out_rgb[3 * p] = c0; out_rgb[3 * p + 1] = c1; out_rgb[3 * p + 2] = c2;
    }
}

// bsc_render_views behind its argument checks: kinv is the matrix to use (the caller's or the context's own), band_host may be null
bsc_status render_impl(bsc_ctx *x, int32_t n_views, const double *transforms_host, const double *kinv, int32_t height, int32_t width,
                       double t_min, double t_max, const bsc_band *band_host, int32_t *voxel_out, float *depth_out, uint8_t *rgb_out)
{
    hipStream_t s = x->stream;
    BSC_TRY(sync_all(x));                                       // the rgb chain writes colours on the side stream
    BSC_TRY(read_scalars(x));
    const int64_t n = x->hscal[DS_MAX_ID];
    const int nh = x->nh;
    int lo = 0, hi = nh - 1;                                    // NULL, or lo > hi as given: every height (the rules of bsc_topdown_slices)
    if (band_host && band_host->lo <= band_host->hi) {
        lo = band_host->lo < 0 ? 0 : band_host->lo;
        hi = band_host->hi > nh - 1 ? nh - 1 : band_host->hi;  // outside [0, nh): lo > hi now, empty
    }
    RwGrid G;
    rw_grid(G, x->c.grid_size, nh, x->c.min_h, x->c.cell_size, lo, hi);
    const int64_t word_bytes = rw_words(G) * (int64_t)sizeof(u64), tf_bytes = (int64_t)n_views * 16 * (int64_t)sizeof(double);
    BSC_TRY(mem_grow(x->mem, (void **)&x->rv_words, &x->rv_cap, word_bytes + 1024 * 16 * (int64_t)sizeof(double), false,
                     "render brick scratch"));
    double *tf_dev = (double *)((char *)x->rv_words + word_bytes);
    BSC_HIP(hipMemcpyAsync(tf_dev, transforms_host, (size_t)tf_bytes, hipMemcpyHostToDevice, s));
    BSC_HIP(hipMemsetAsync(x->rv_words, 0, (size_t)word_bytes, s));
    if (n > 0)
        hipLaunchKernelGGL(k_rv_bricks, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, n, (const int32_t *)x->rgb_pos, G, x->rv_words);
    RvKinv K;
    for (int i = 0; i < 9; ++i) K.m[i] = kinv[i];
    hipLaunchKernelGGL(k_rv_cast, dim3((unsigned)((width + 31) / 32), (unsigned)((height + 7) / 8), (unsigned)n_views), dim3(TPB), 0, s, G,
                       (const u64 *)x->rv_words, (const double *)tf_dev, K, (int)height, (int)width, t_min, t_max, (const int32_t *)x->occ,
                       (const uint8_t *)x->rgb, n, voxel_out, depth_out, rgb_out);
    BSC_HIP(hipGetLastError());
    BSC_HIP(hipStreamSynchronize(s));
    return BSC_OK;
}
