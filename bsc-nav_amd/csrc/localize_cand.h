// localize_cand.h — the candidates of a localize call as its kernels see them: the store (VoxelView), a query's region (RegionDev),
// the two candidate lists (CandArgs / RegionCandArgs) and a candidate's score.  Shared by the two ways out of the cosine scan's
// similarities: the ranked top-K (localize.hip) and the per-cell score map (score_map.hip).
#pragma once
#include "bsc_internal.h"

#include <math.h>

__device__ __forceinline__ uint32_t float_desc_key(float f)
{
    uint32_t u = __float_as_uint(f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending-orderable
    return ~u;                                          // descending similarity == ascending key
}

// The store as the candidate kernels read it, whatever its mode.  Candidate (voxel) c in [0, max_id] sits in entry c of cnt /
// rgb_pos / store_rows, except c == max_id, the grid_0_0_0 group: entry vcap, position (0, 0, 0).  (Dense acnt has no slot of its
// own for that group: it is allocated vcap + 1.)
struct VoxelView {
    int max_id, vcap, cache_size, exact;
    const int32_t *rgb_pos, *cnt, *store_rows;
    const uint32_t *name_rank;

    __device__ __forceinline__ int entry(int c) const { return (c == max_id) ? vcap : c; }
    __device__ __forceinline__ void position(int c, int &r, int &cc, int &h) const
    {
        r = 0; cc = 0; h = 0;
        if (c != max_id) { r = rgb_pos[3 * c]; cc = rgb_pos[3 * c + 1]; h = rgb_pos[3 * c + 2]; }
    }
    // similarity key of the best of the m tokens of entry e (memory_2.py:661) when the scan ran over the store's own rows: token-pool
    // rows of an exact store, row e of a dense map
    __device__ __forceinline__ float best_sim(int e, int m, const float *__restrict__ sims) const
    {
        if (!exact) return sims[e];
        float best = -INFINITY;
        for (int k = 0; k < m; ++k) best = fmaxf(best, sims[store_rows[(int64_t)e * cache_size + k]]);
        return best;
    }
};

// bsc_region as the kernels read it: radius^2 in double, the two switches resolved
struct RegionDev {
    double radius2;
    int32_t c0, c1, c2, floor_lo, floor_hi, use_radius;
};
static_assert(sizeof(RegionDev) == 32, "RegionDev layout");

// neither sphere nor floor band: the region holds every voxel
__host__ __device__ static inline bool region_open(const RegionDev &g) { return !g.use_radius && !(g.floor_lo <= g.floor_hi); }

// memory_2.py:624-640 for one voxel and one region
__device__ __forceinline__ bool region_sees(const RegionDev &g, int r, int cc, int h)
{
    if (g.use_radius) {   // :624-629 (integer squared distance compared with radius**2)
        const double dx = r - g.c0, dy = cc - g.c1, dz = h - g.c2;
        if (!((dx * dx + dy * dy + dz * dz) <= g.radius2)) return false;
    }
    if (g.floor_lo <= g.floor_hi && !((g.floor_lo <= h) && (h <= g.floor_hi))) return false;   // :633-640
    return true;
}

// The selection kernels of localize.hip are written once for two kinds of candidate list: CandArgs (bsc_localize: every voxel, one
// region for all queries) and RegionCandArgs (bsc_localize_regions, bsc_score_map: a region per query, possibly a compacted list).
// Entry i of a list has a similarity key for query q (0xffffffff: filtered out / empty), a voxel (what k_gather_topk reads the
// position of) and a name rank.
struct CandArgs : VoxelView {
    int n_cand;                    // max_id + 1
    RegionDev region;
};

struct RegionCandArgs : VoxelView {
    int n_cand;                    // entries of the list: max_id + 1, or the visible voxels when the scan was pruned
    const RegionDev *regions;      // (Q)
    const uint32_t *mask;          // visibility bits, word (q / 32) * mask_stride + voxel; nullptr: the pass was skipped
    int64_t mask_stride;
    const uint32_t *cidx;          // pruned scan: entry -> voxel (candidate id); nullptr: entry i is voxel i
    const int32_t *rowoff;         // pruned scan: entry -> its first row in the gathered matrix
};

__device__ __forceinline__ uint32_t simkey_of(float best)
{
    const uint32_t sk = float_desc_key(best);
    return sk == 0xffffffffu ? 0xfffffffeu : sk;     // keep the all-ones pattern for "no candidate"
}

__device__ __forceinline__ uint32_t cand_val(const RegionCandArgs &a, int i) { return a.cidx ? (i < a.n_cand ? a.cidx[i] : 0u) : (uint32_t)i; }
// does query q rank entry i, and with which score: the float max of its tokens' cosines (sims: the query's similarity row)
__device__ __forceinline__ bool cand_score(const RegionCandArgs &a, int i, int q, const float *__restrict__ sims, float &best)
{
    if (i >= a.n_cand) return false;
    const int c = (int)cand_val(a, i);
    const int e = a.entry(c);
    const int m = a.cnt[e];
    if (a.mask) {                  // the visibility pass made the test (empty voxels see nothing there)
        if (!((a.mask[(int64_t)(q >> 5) * a.mask_stride + c] >> (q & 31)) & 1u)) return false;
    } else {
        if (m <= 0) return false;
        int r, cc, h;
        a.position(c, r, cc, h);
        if (!region_sees(a.regions[q], r, cc, h)) return false;
    }
    if (!a.rowoff) { best = a.best_sim(e, m, sims); return true; }
    best = -INFINITY;              // gathered rows of entry i are consecutive
    const int base = a.rowoff[i], nr = a.exact ? m : 1;
    for (int k = 0; k < nr; ++k) best = fmaxf(best, sims[base + k]);
    return true;
}

// What the shared front half of bsc_localize_regions and bsc_score_map (localize.hip region_scan) leaves behind: the similarities
// of the nq queries in x->l_sims, query rows `sstride` floats apart, and the candidate list that reads them.
struct RegionScan {
    RegionCandArgs ca;
    int n_voxels;                  // max_id + 1, whatever the list holds
    int64_t sstride;
    bool all_open;                 // no query has a sphere or a band: CandArgs with an open region describes the same candidates
    bool nothing;                  // no query sees any voxel: the scan was not run, ca is not filled in
};
