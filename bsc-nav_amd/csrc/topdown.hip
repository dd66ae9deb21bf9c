// topdown.hip — bsc_topdown_slices / bsc_topdown_rebuild: top-down maps of a height band from the STORED voxels.  The resident
// cv_map / hmap is the map of the points as they arrived (memory_2.py:98-100,901-903) and exists only while frames are ingested;
// this is TrajectoryDrawer._get_rgb_2d_map (BSCAgent.py:203-234) — per column the colour of the highest stored voxel at or below a
// cut — for any number of bands lo <= h <= hi at once (memory_2.py:202-252 computes such a band for one floor).
//
//   k_td_mask      one thread per voxel id < max_id: one 64-bit atomicOr of bit h & 63 into mask[(r * gs + c) * W + (h >> 6)],
//                  W = ceil(nh / 64).  OR does not care about arrival order: the mask is the same from run to run.  Built once per
//                  call, whatever the number of bands; rows >= max_id (stale after a reset) are never read.
//   k_td_decode    one thread per (band, cell): the band clipped to [0, nh), the mask's words walked downwards from hi — the highest
//                  set bit (clz) is h, the popcount within the band the count; the voxel is occ[(r * gs + c) * nh + h], the colour
//                  rgb[id].  bsc_topdown_rebuild runs it for one band with cv_map as the colour output and the packed hmap word.
// The mask (gs^2 W 8 bytes, then the bands of the call) is scratch of the context.
#include "bsc_internal.h"

#define TPB 256

__global__ __launch_bounds__(TPB) void k_td_mask(int64_t n, const int32_t *__restrict__ pos, int gs, int nh, int W, u64 *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int32_t r = pos[3 * i], c = pos[3 * i + 1], h = pos[3 * i + 2];
    if (r < 0 || c < 0 || h < 0 || r >= gs || c >= gs || h >= nh) return;       // (no state the library builds has such a row)
    atomicOr(mask + ((int64_t)r * gs + c) * W + (h >> 6), 1ull << (h & 63));
}

// grid (cells / TPB, bands): consecutive threads read consecutive mask words (W each) and write consecutive outputs
__global__ __launch_bounds__(TPB) void k_td_decode(const u64 *__restrict__ mask, int64_t cells, int nh, int W,
                                                   const bsc_band *__restrict__ bands, const int32_t *__restrict__ occ,
                                                   const uint8_t *__restrict__ rgb, int64_t vcap, uint8_t *__restrict__ out_rgb,
                                                   int32_t *__restrict__ out_h, int32_t *__restrict__ out_cnt, u64 *__restrict__ out_hmap)
{
    const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (c >= cells) return;
    int lo = 0, hi = nh - 1;                                    // lo > hi as given: every height
    if (bands) {
        const bsc_band b = bands[blockIdx.y];
        if (b.lo <= b.hi) { lo = b.lo < 0 ? 0 : b.lo; hi = b.hi > nh - 1 ? nh - 1 : b.hi; }    // outside [0, nh): lo > hi now, empty
    }
    int h = -1, cnt = 0;
    if (lo <= hi) {
        const u64 *m = mask + c * W;
        for (int w = hi >> 6; w >= (lo >> 6); --w) {
            u64 v = m[w];
            if (w == (hi >> 6) && (hi & 63) != 63) v &= (2ull << (hi & 63)) - 1ull;
            if (w == (lo >> 6)) v &= ~0ull << (lo & 63);
            if (h < 0 && v) h = w * 64 + 63 - __clzll((long long)v);
            cnt += __popcll(v);
        }
    }
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    if (h >= 0 && out_rgb) {
        const int32_t id = occ[c * nh + h];
        if (id >= 0 && id < vcap) { c0 = rgb[3 * (int64_t)id]; c1 = rgb[3 * (int64_t)id + 1]; c2 = rgb[3 * (int64_t)id + 2]; }
    }
    const int64_t o = (int64_t)blockIdx.y * cells + c;
    if (out_rgb) { out_rgb[3 * o] = c0; out_rgb[3 * o + 1] = c1; out_rgb[3 * o + 2] = c2; }
    if (out_h) out_h[o] = h;
    if (out_cnt) out_cnt[o] = cnt;
    if (out_hmap) out_hmap[o] = h >= 0 ? (u64)(h + 1) << 40 : 0ull;             // what bsc_import_heightmap writes for h: order bits 0
}

// The shared body: bands_host == nullptr is one open band.  hmap_out is the rebuild's; the others are the caller's (any may be null).
bsc_status topdown_impl(bsc_ctx *x, int32_t n_bands, const bsc_band *bands_host, uint8_t *rgb_out, int32_t *height_out,
                        int32_t *count_out, u64 *hmap_out)
{
    hipStream_t s = x->stream;
    BSC_TRY(sync_all(x));                                       // the rgb chain writes colours on the side stream
    BSC_TRY(read_scalars(x));
    const int64_t n = x->hscal[DS_MAX_ID];
    const int gs = x->c.grid_size, nh = x->nh, W = (nh + 63) / 64;
    const int64_t cells = (int64_t)gs * gs, mask_bytes = cells * W * (int64_t)sizeof(u64);
    BSC_TRY(mem_grow(x->mem, (void **)&x->td_mask, &x->td_cap, mask_bytes + 256 * (int64_t)sizeof(bsc_band), false, "top-down mask scratch"));
    bsc_band *bands_dev = nullptr;
    if (bands_host) {
        bands_dev = (bsc_band *)((char *)x->td_mask + mask_bytes);
        BSC_HIP(hipMemcpyAsync(bands_dev, bands_host, sizeof(bsc_band) * (size_t)n_bands, hipMemcpyHostToDevice, s));
    }
    BSC_HIP(hipMemsetAsync(x->td_mask, 0, (size_t)mask_bytes, s));
    if (n > 0)
        hipLaunchKernelGGL(k_td_mask, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, n, (const int32_t *)x->rgb_pos, gs, nh, W,
                           x->td_mask);
    hipLaunchKernelGGL(k_td_decode, dim3((unsigned)((cells + TPB - 1) / TPB), (unsigned)n_bands), dim3(TPB), 0, s,
                       (const u64 *)x->td_mask, cells, nh, W, (const bsc_band *)bands_dev, (const int32_t *)x->occ,
                       (const uint8_t *)x->rgb, (int64_t)x->c.voxel_capacity, rgb_out, height_out, count_out, hmap_out);
    BSC_HIP(hipGetLastError());
    BSC_HIP(hipStreamSynchronize(s));
    return BSC_OK;
}
