// The traversal of bsc_render_views (csrc/ray_walk.h) on the CPU, against a slab test of every ray with every voxel.
//
//   ray_walk_test <scene file> [<result file>]
//
// The scene file (written by tests/test_ray_walk.py; numbers as text, doubles as C99 hex floats):
//   grid <gs> <nh> <min_h> <cs>
//   voxels <N>            then N lines  <row> <col> <h>
//   cases <M>             then per case <name> <H> <W> <t_min> <t_max> <lo> <hi>   (the band, already clipped; lo > hi: empty)
//                                       T <16 doubles>   K <9 doubles: K^-1>
// Per case one line "ok <name> <pixels> <ambiguous>" or "FAIL <name> ...".  A pixel is ambiguous (tol 1e-9) when the winner's interval
// is shorter than tol, lies within tol of t_min / t_max, or another voxel whose interval is longer than -tol enters within tol of
// the winner; everywhere else the walk must name the slab test's voxel with the very same t.  At most 0.5 % of a case's pixels may
// be ambiguous.  The result file gets the walk's "<row> <col> <h> <t>" per pixel, for the NumPy reference of the GPU tests.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bsc-nav_amd/csrc/ray_walk.h"

struct Vox { int r, c, h; };

static double rd(FILE *f)
{
    char buf[128];
    if (fscanf(f, "%127s", buf) != 1) { fprintf(stderr, "scene file: number expected\n"); exit(2); }
    return strtod(buf, nullptr);
}

static int ri(FILE *f) { return (int)rd(f); }

static void expect(FILE *f, const char *word)
{
    char buf[128];
    if (fscanf(f, "%127s", buf) != 1 || strcmp(buf, word)) { fprintf(stderr, "scene file: '%s' expected\n", word); exit(2); }
}

// [t_in, t_out) of the ray through the cell, from the cell's own planes; an axis with d == 0: everything when o is strictly inside
static void slab(const RwGrid &G, const Vox &v, const double *o, const double *d, double &t_in, double &t_out)
{
    const int g[3] = {v.r, v.c, v.h};
    t_in = -INFINITY; t_out = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const double p0 = rw_plane(G, a, g[a]), p1 = rw_plane(G, a, g[a] + 1);
        const double lo = p0 < p1 ? p0 : p1, hi = p0 < p1 ? p1 : p0;
        if (d[a] == 0.0) {
            if (!(o[a] > lo && o[a] < hi)) { t_in = INFINITY; t_out = -INFINITY; }
            continue;
        }
        const double ta = (lo - o[a]) / d[a], tb = (hi - o[a]) / d[a];
        const double tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
        t_in = tn > t_in ? tn : t_in;
        t_out = tf < t_out ? tf : t_out;
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <scene file> [<result file>]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    FILE *out = argc > 2 ? fopen(argv[2], "w") : nullptr;
    expect(f, "grid");
    const int gs = ri(f), nh = ri(f), min_h = ri(f);
    const double cs = rd(f);
    expect(f, "voxels");
    std::vector<Vox> vox((size_t)ri(f));
    for (Vox &v : vox) { v.r = ri(f); v.c = ri(f); v.h = ri(f); }
    expect(f, "cases");
    const int n_cases = ri(f);
    const double tol = 1e-9;
    int failed = 0;
    for (int k = 0; k < n_cases; ++k) {
        char name[128];
        if (fscanf(f, "%127s", name) != 1) return 2;
        const int H = ri(f), W = ri(f);
        const double t_min = rd(f), t_max = rd(f);
        const int lo = ri(f), hi = ri(f);
        double T[16], K[9];
        expect(f, "T");
        for (double &x : T) x = rd(f);
        expect(f, "K");
        for (double &x : K) x = rd(f);
        RwGrid G;
        rw_grid(G, gs, nh, min_h, cs, lo, hi);
        std::vector<uint64_t> mask((size_t)rw_words(G), 0);        // every voxel, as k_rv_bricks builds it: the band is the walk's
        for (const Vox &v : vox) mask[(size_t)rw_word_of(G, v.r, v.c, v.h)] |= 1ull << rw_bit_of(v.r, v.c, v.h);
        int ambiguous = 0, wrong = 0;
        std::string first;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double o[3], d[3];
                rw_ray(T, K, x, y, o, d);
                const RwHit got = rw_first_hit(G, mask.data(), o, d, t_min, t_max);
                if (out) fprintf(out, "%d %d %d %a\n", got.cell[0], got.cell[1], got.cell[2], got.t);
                int best = -1;
                double best_key = INFINITY, best_in = 0, best_out = 0;
                for (size_t i = 0; i < vox.size(); ++i) {
                    if (vox[i].h < lo || vox[i].h > hi) continue;
                    double a, b;
                    slab(G, vox[i], o, d, a, b);
                    if (!(a < b && a <= t_max && b > t_min)) continue;
                    const double key = a > t_min ? a : t_min;
                    if (key < best_key) { best_key = key; best = (int)i; best_in = a; best_out = b; }
                }
                bool amb = best >= 0 && (best_out - best_in < tol || fabs(best_in - t_min) < tol || fabs(best_in - t_max) < tol ||
                                         fabs(best_out - t_min) < tol);
                for (size_t i = 0; i < vox.size() && best >= 0 && !amb; ++i) {
                    if ((int)i == best || vox[i].h < lo || vox[i].h > hi) continue;
                    double a, b;
                    slab(G, vox[i], o, d, a, b);
                    amb = b - a > -tol && b > t_min - tol && (a > t_min ? a : t_min) < best_key + tol;
                }
                if (amb) { ++ambiguous; continue; }
                const bool same = best < 0 ? got.cell[0] == -1 && got.t == 0.0
                                           : got.cell[0] == vox[best].r && got.cell[1] == vox[best].c && got.cell[2] == vox[best].h &&
                                                 got.t == best_key;
                if (!same && ++wrong == 1) {
                    char buf[256];
                    snprintf(buf, sizeof buf, "pixel (%d,%d): walk %d %d %d t=%.17g, slab test %d t=%.17g", x, y, got.cell[0], got.cell[1],
                             got.cell[2], got.t, best, best < 0 ? 0.0 : best_key);
                    first = buf;
                }
            }
        const bool ok = wrong == 0 && ambiguous * 200 <= H * W;
        if (ok) printf("ok %s %d %d\n", name, H * W, ambiguous);
        else printf("FAIL %s %d wrong, %d of %d ambiguous; %s\n", name, wrong, ambiguous, H * W, first.c_str());
        failed += ok ? 0 : 1;
    }
    fclose(f);
    if (out) fclose(out);
    return failed ? 1 : 0;
}
