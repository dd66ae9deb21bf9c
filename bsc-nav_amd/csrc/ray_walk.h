// ray_walk.h — the first stored voxel a ray meets: the traversal of bsc_render_views (render.hip), as plain C++ for the device and the
// host alike (no HIP include: tests/host/ray_walk_main.cpp runs on the CPU the very code k_rv_cast runs).
//
// Cells.  The ingest places a point by truncation toward zero (utils.py:201-205, geometry_dev.h:113-119): along an axis the point
// p lies in truncation cell k = trunc(p / cs), and cell k covers [k cs, (k+1) cs) for k > 0, (-cs, cs) for k = 0 — twice as wide —
// and ((k-1) cs, k cs] for k < 0.  The boundary below cell k is therefore the plane P(k) = (k > 0 ? k : k - 1) cs, and P(k+1) is
// the one above it.  Grid indices run against x and y and with z: row = gs/2 - kx, col = gs/2 - ky, h = kz - min_h (gs even).  In
// grid index space boundary i of an axis (between cells i-1 and i, i = 0 .. n) is rw_plane(): P(gs/2 - i + 1) for rows and
// columns, P(min_h + i) for heights.
//
// Parameters.  The ray is p(t) = o + t d.  Every crossing parameter is taken from its plane, (plane - o) / d, never accumulated, so
// the interval [t_in, t_out) of a cell is the same bits wherever it is evaluated.  An axis with d == 0 is never crossed and never
// divided by: the ray stays in the cell of o on that axis.
//
// Walk.  The ray is clipped to the grid's box; the cell at the start max(t_min, box entry) is found from the point and corrected
// by the plane parameters; then two levels: brick to brick (4 x 4 x 4 cells, one 64-bit word of occupancy bits each, bit
// (r&3)<<4 | (c&3)<<2 | (h&3)), skipping a brick whose word has no bit inside the height band, and cell to cell inside a brick
// that has one, testing bits of the word in registers.  Axes whose next planes tie are stepped together: the cells a ray touches
// only in an edge or a corner have an empty interval and do not qualify.  Both loops are bounded by the grid (rw_brick_steps,
// RW_CELL_STEPS); a ray that reaches a bound reports no hit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RW_HD __host__ __device__ inline
#else
#define RW_HD inline
#endif

#define RW_INF __builtin_huge_val()
#define RW_CELL_STEPS 16                    // a straight line crosses at most 10 cells of a 4 x 4 x 4 brick

struct RwGrid {
    double cs;
    int32_t n[3];                           // cells along rows, columns, heights: gs, gs, nh
    int32_t nb[3];                          // bricks: ceil(n / 4)
    int32_t half, min_h;                    // gs / 2 (gs even), min_h
    int32_t lo, hi;                         // the height band lo <= h <= hi, clipped to [0, nh); lo > hi: empty
};

struct RwHit {
    int32_t cell[3];                        // row, column, h of the hit; -1 without one
    double t;                               // max(t_in, t_min) of that cell; 0 without one
};

RW_HD void rw_grid(RwGrid &G, int32_t gs, int32_t nh, int32_t min_h, double cs, int32_t lo, int32_t hi)
{
    G.cs = cs;
    G.n[0] = gs; G.n[1] = gs; G.n[2] = nh;
    for (int a = 0; a < 3; ++a) G.nb[a] = (G.n[a] + 3) >> 2;
    G.half = gs / 2; G.min_h = min_h;
    G.lo = lo; G.hi = hi;
}

RW_HD int64_t rw_words(const RwGrid &G) { return (int64_t)G.nb[0] * G.nb[1] * G.nb[2]; }
RW_HD int64_t rw_word_of(const RwGrid &G, int r, int c, int h) { return ((int64_t)(r >> 2) * G.nb[1] + (c >> 2)) * G.nb[2] + (h >> 2); }
RW_HD int rw_bit_of(int r, int c, int h) { return (r & 3) << 4 | (c & 3) << 2 | (h & 3); }
RW_HD int rw_brick_steps(const RwGrid &G) { return 2 * (G.nb[0] + G.nb[1] + G.nb[2]) + 8; }

// the bits of brick layer bh whose heights lie in the band
RW_HD uint64_t rw_band_bits(const RwGrid &G, int bh)
{
    uint64_t m = 0;
    for (int l = 0; l < 4; ++l)
        if (4 * bh + l >= G.lo && 4 * bh + l <= G.hi) m |= 1ull << l;
    return m * 0x1111111111111111ull;
}

// boundary i (between cells i - 1 and i) of axis a, in map coordinates
RW_HD double rw_plane(const RwGrid &G, int a, int i)
{
    const int j = a == 2 ? G.min_h + i : G.half - i + 1;
    return (double)(j > 0 ? j : j - 1) * G.cs;
}

// the ray's parameter at that boundary (d != 0)
RW_HD double rw_tp(const RwGrid &G, int a, int i, double o, double d) { return (rw_plane(G, a, i) - o) / d; }

// grid index of the cell of coordinate p on axis a by the truncation intervals; may lie outside [0, n)
RW_HD int rw_cell_of(const RwGrid &G, int a, double p)
{
    double q = p / G.cs;
    q = q > 1e9 ? 1e9 : (q < -1e9 ? -1e9 : q);            // (a NaN fails both and converts to some integer: the callers bound it)
    int k = (int)q;
    for (int it = 0; it < 2; ++it) {                        // the planes, not the quotient, say where a point next to one lies
        const double lo = (double)(k > 0 ? k : k - 1) * G.cs, hi = (double)(k + 1 > 0 ? k + 1 : k) * G.cs;
        if (k > 0 ? p < lo : p <= lo) --k;
        else if (k < 0 ? p > hi : p >= hi) ++k;
    }
    return a == 2 ? k - G.min_h : G.half - k;
}

// pixel (x, y) of a view: o = T[:3,3], d = T[:3,:3] (Kinv (x + 0.5, y + 0.5, 1)); T row-major 4 x 4, Kinv row-major 3 x 3
RW_HD void rw_ray(const double *T, const double *Kinv, int x, int y, double *o, double *d)
{
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    double c[3];
    for (int i = 0; i < 3; ++i) c[i] = (Kinv[3 * i] * px + Kinv[3 * i + 1] * py) + Kinv[3 * i + 2];
    for (int i = 0; i < 3; ++i) {
        o[i] = T[4 * i + 3];
        d[i] = (T[4 * i] * c[0] + T[4 * i + 1] * c[1]) + T[4 * i + 2] * c[2];
    }
}

// Among the cells whose bit is set in `mask` (rw_word_of / rw_bit_of) and whose height lies in the band, the one the ray enters
// first: its interval [t_in, t_out) is not empty and meets [t_min, t_max], and max(t_in, t_min) is the smallest.
RW_HD RwHit rw_first_hit(const RwGrid &G, const uint64_t *mask, const double *o, const double *d, double t_min, double t_max)
{
    RwHit none;
    none.cell[0] = none.cell[1] = none.cell[2] = -1;
    none.t = 0.0;
    int dg[3], g[3], b[3];
    // the box: the ray is inside it on every axis for t in [t0, t_far)
    double t0 = t_min, t_far = RW_INF;
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0) {
            dg[a] = 0;
            g[a] = rw_cell_of(G, a, o[a]);
            if (g[a] < 0 || g[a] >= G.n[a]) return none;
            continue;
        }
        dg[a] = ((d[a] > 0.0) == (a == 2)) ? 1 : -1;
        const double te = rw_tp(G, a, dg[a] > 0 ? 0 : G.n[a], o[a], d[a]), tx = rw_tp(G, a, dg[a] > 0 ? G.n[a] : 0, o[a], d[a]);
        t0 = te > t0 ? te : t0;
        t_far = tx < t_far ? tx : t_far;
    }
    if (!(t0 < t_far && t0 <= t_max)) return none;
    // the cell at t0: from the point, then by the planes' own parameters (entry <= t0 < exit on every axis)
    for (int a = 0; a < 3; ++a) {
        if (dg[a] == 0) continue;
        int c = rw_cell_of(G, a, o[a] + t0 * d[a]);
        c = c < 0 ? 0 : (c >= G.n[a] ? G.n[a] - 1 : c);
        for (int it = 0; it < 2; ++it)
            if (c + dg[a] >= 0 && c + dg[a] < G.n[a] && rw_tp(G, a, dg[a] > 0 ? c + 1 : c, o[a], d[a]) <= t0) c += dg[a];
        for (int it = 0; it < 2; ++it)
            if (c - dg[a] >= 0 && c - dg[a] < G.n[a] && rw_tp(G, a, dg[a] > 0 ? c : c + 1, o[a], d[a]) > t0) c -= dg[a];
        g[a] = c;
    }
    for (int a = 0; a < 3; ++a) b[a] = g[a] >> 2;
    double t_cur = t0;                      // where the ray enters the current brick / cell (t0 in the first)
    bool have_cells = true;                 // g is the cell at t_cur (after a skipped brick only b is known)
    const int max_bricks = rw_brick_steps(G);
    for (int step = 0; step < max_bricks; ++step) {
        const uint64_t word = mask[((int64_t)b[0] * G.nb[1] + b[1]) * G.nb[2] + b[2]] & rw_band_bits(G, b[2]);
        if (word == 0) {
            // to the next brick: the nearest exit plane; tied axes leave together
            double tx[3], t_next = RW_INF;
            for (int a = 0; a < 3; ++a) {
                tx[a] = RW_INF;
                if (dg[a] == 0) continue;
                const int top = 4 * b[a] + 4 < G.n[a] ? 4 * b[a] + 4 : G.n[a];
                tx[a] = rw_tp(G, a, dg[a] > 0 ? top : 4 * b[a], o[a], d[a]);
                t_next = tx[a] < t_next ? tx[a] : t_next;
            }
            if (!(t_next <= t_max)) return none;
            for (int a = 0; a < 3; ++a)
                if (tx[a] == t_next) {
                    b[a] += dg[a];
                    if (b[a] < 0 || b[a] >= G.nb[a]) return none;
                }
            t_cur = t_next;
            have_cells = false;
            continue;
        }
        if (!have_cells) {
            // the cell at t_cur inside brick b: the brick's inner planes already crossed, counted from the side the ray came from
            for (int a = 0; a < 3; ++a) {
                if (dg[a] == 0) continue;
                int crossed = 0;
                for (int l = 1; l < 4; ++l)
                    crossed += rw_tp(G, a, dg[a] > 0 ? 4 * b[a] + l : 4 * b[a] + 4 - l, o[a], d[a]) <= t_cur ? 1 : 0;
                g[a] = dg[a] > 0 ? 4 * b[a] + crossed : 4 * b[a] + 3 - crossed;
            }
            have_cells = true;
        }
        bool left = false;
        for (int cstep = 0; cstep < RW_CELL_STEPS && !left; ++cstep) {
            if (g[0] >= G.n[0] || g[1] >= G.n[1] || g[2] >= G.n[2]) return none;        // (the last brick of an axis may be partial)
            if (word >> rw_bit_of(g[0], g[1], g[2]) & 1) {
                if (!(t_cur <= t_max)) return none;
                RwHit hit;
                double t_in = t_min;
                for (int a = 0; a < 3; ++a) {
                    hit.cell[a] = g[a];
                    if (dg[a] == 0) continue;
                    const double te = rw_tp(G, a, dg[a] > 0 ? g[a] : g[a] + 1, o[a], d[a]);
                    t_in = te > t_in ? te : t_in;
                }
                hit.t = t_in;
                return hit;
            }
            double tx[3], t_next = RW_INF;
            for (int a = 0; a < 3; ++a) {
                tx[a] = RW_INF;
                if (dg[a] == 0) continue;
                tx[a] = rw_tp(G, a, dg[a] > 0 ? g[a] + 1 : g[a], o[a], d[a]);
                t_next = tx[a] < t_next ? tx[a] : t_next;
            }
            if (!(t_next <= t_max)) return none;
            for (int a = 0; a < 3; ++a)
                if (tx[a] == t_next) {
                    g[a] += dg[a];
                    if (g[a] < 0 || g[a] >= G.n[a]) return none;
                    if ((g[a] >> 2) != b[a]) { b[a] = g[a] >> 2; left = true; }
                }
            t_cur = t_next;
        }
        if (!left) return none;             // the cell bound: cannot happen on a straight line
    }
    return none;
}
