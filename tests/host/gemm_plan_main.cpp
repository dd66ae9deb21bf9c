// The launch plan of the split GEMM (csrc/gemm_split_plan.h) on the CPU: the plans of a grid of shapes are walked the way the
// kernel's persistent workgroups walk them.  usage: gemm_plan_test <case>  -> "ok <case>", exit status 0
#include "../../bsc-nav_amd/csrc/gemm_split_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s: ", #cond);            \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            return false;                                 \
        }                                                 \
    } while (0)

static const int kCus[] = {8, 64, 256};
static const int64_t kM[] = {1, 197, 261, 512, 513, 1576, 8192, 8193, 75648};
static const int kN[] = {4, 102, 768, 1024, 1280, 2304, 4096};
static const int kK[] = {64, 608, 768, 4096};
static const int kEpi[] = {GS_EPI_RESID, GS_EPI_BIAS, GS_EPI_GELU};
static const int64_t kWs[] = {0, (int64_t)34 << 20};

// every plan of the grid (f32 rows in, f32 out) through fn(plan, M, K, N, n_cu, ws)
template <class F> static bool for_grid(F fn)
{
    for (int n_cu : kCus)
        for (int64_t M : kM)
            for (int N : kN)
                for (int K : kK)
                    for (int epi : kEpi)
                        for (int64_t ws : kWs) {
                            GsPlan p;
                            const char *why = nullptr;
                            CHECK(gs_plan(M, K, N, epi, GS_A_F32, false, false, false, ws, n_cu, &p, &why), "M %lld K %d N %d: %s", (long long)M, K, N, why);
                            if (!fn(p, M, K, N, n_cu, ws)) {
                                std::printf("  at n_cu %d M %lld N %d K %d epilogue %d ws %lld: tile %d S %d\n", n_cu, (long long)M, N, K, epi,
                                            (long long)ws, p.tile, p.S);
                                return false;
                            }
                        }
    return true;
}

// the kernel's schedule: workgroup p serves XCD p & 7 and the entries p >> 3, + per_round, ... of its list; every 32-column block of
// every row tile of the M x n_pad matrix belongs to exactly one valid tile
static bool coverage()
{
    return for_grid([](const GsPlan &p, int64_t, int, int, int, int64_t) {
        const int64_t nb = p.n_pad / 32;
        std::vector<unsigned char> seen((size_t)(p.n_tiles_m * nb), 0);
        for (int64_t wg = 0; wg < p.n_wg; ++wg) {
            const int xcd = (int)(wg & 7);
            for (int64_t qv = wg >> 3; qv < p.q_virtual; qv += p.per_round) {
                const GsTile t = gs_tile_of(p.n_tiles_n, p.n_tiles_m, p.q_full, p.q_virtual, p.cols, p.half_cols, xcd, qv);
                if (!t.valid) continue;
                const int width = t.half ? p.half_cols : p.cols;
                CHECK(t.tm >= 0 && t.tm < p.n_tiles_m && t.n0 >= 0 && t.n0 % 32 == 0 && width > 0 && t.n0 + width <= p.n_pad,
                      "tile (%lld, %d) of width %d outside the matrix", (long long)t.tm, t.n0, width);
                for (int b = t.n0 / 32; b < (t.n0 + width) / 32; ++b) ++seen[(size_t)(t.tm * nb + b)];
            }
        }
        for (int64_t tm = 0; tm < p.n_tiles_m; ++tm)
            for (int64_t b = 0; b < nb; ++b)
                CHECK(seen[(size_t)(tm * nb + b)] == 1, "row tile %lld, columns %lld.. computed %d times", (long long)tm, (long long)b * 32,
                      (int)seen[(size_t)(tm * nb + b)]);
        return true;
    });
}

static bool resources()
{
    if (!for_grid([](const GsPlan &p, int64_t M, int, int N, int, int64_t) {
            CHECK(p.n_wg >= 1 && p.n_wg <= 8 * p.per_round, "n_wg %lld per_round %lld", (long long)p.n_wg, (long long)p.per_round);
            CHECK(p.lds == p.lds_loop + p.lds_epi + p.n_pad * 4 && p.lds <= 160 * 1024, "lds %lld", (long long)p.lds);
            CHECK(p.threads <= 512 && p.n_pad >= N && p.n_pad % p.cols == 0 && p.n_tiles_m * p.rows >= M, "tile shape");
            return true;
        }))
        return false;
    GsPlan p;
    const char *why = nullptr;
    CHECK(!gs_plan(9000, 768, 20000, GS_EPI_BIAS, GS_A_F32, false, false, false, 0, 256, &p, &why), "a bias row beyond the LDS was planned");
    CHECK(why && std::strstr(why, "does not fit the kernel's LDS plan"), "%s", why ? why : "(no message)");
    return true;
}

static bool split_k()
{
    return for_grid([](const GsPlan &p, int64_t M, int K, int N, int n_cu, int64_t ws) {
        CHECK(p.S >= 1 && p.k_len * p.S == K, "S %d k_len %d", p.S, p.k_len);
        if (ws == 0 || N % 4 != 0) CHECK(p.S == 1, "S %d without a workspace or with N %% 4 != 0", p.S);
        if (p.S > 1) {
            CHECK(K % (32 * p.S) == 0 && K / p.S >= 64, "slices of %d columns", K / p.S);
            CHECK((int64_t)p.S * M * N * 4 <= ws, "partial results beyond the workspace");
            CHECK(p.n_tiles_m * p.n_tiles_n * p.S <= 2 * (int64_t)n_cu, "%lld workgroups", (long long)(p.n_tiles_m * p.n_tiles_n * p.S));
        }
        return true;
    });
}

// two plans worked out by hand from the rules in gs_plan
static bool pinned()
{
    GsPlan p;
    const char *why = nullptr;
    // 384 frames of ViT-B, N = 768: 296 row tiles x 3 = 888 tiles of 256 x 256; 37 row tiles per XCD x 3 = 111 entries, 32 workgroups per
    // XCD: the last round holds 15 <= 16 entries, so they run as 30 half tiles
    CHECK(gs_plan(75648, 768, 768, GS_EPI_RESID, GS_A_PIECES, false, false, false, 0, 256, &p, &why), "%s", why);
    CHECK(p.tile == 1 && p.rows == 256 && p.cols == 256 && p.threads == 512 && p.half_cols == 128, "tile %d", p.tile);
    CHECK(p.n_tiles_m == 296 && p.n_tiles_n == 3 && p.n_tiles_m * p.n_tiles_n == 888, "tiles");
    CHECK(p.q_full == 96 && p.q_virtual == 126 && p.per_round == 32 && p.n_wg == 256 && p.S == 1 && p.k_len == 768, "q_full %lld q_virtual %lld n_wg %lld S %d",
          (long long)p.q_full, (long long)p.q_virtual, (long long)p.n_wg, p.S);
    // one frame, qkv: 9 big tiles on 256 CUs -> the 32 x 128 tile, 7 x 18 = 126 tiles; 4 slices are the most within 512 workgroups
    CHECK(gs_plan(197, 768, 2304, GS_EPI_BIAS, GS_A_F32, false, false, false, (int64_t)34 << 20, 256, &p, &why), "%s", why);
    CHECK(p.tile == 6 && p.rows == 32 && p.cols == 128 && p.threads == 256 && p.half_cols == 0, "tile %d", p.tile);
    CHECK(p.n_tiles_m == 7 && p.n_tiles_n == 18 && p.S == 4 && p.k_len == 192, "S %d k_len %d", p.S, p.k_len);
    CHECK(gs_plan(197, 768, 2304, GS_EPI_BIAS, GS_A_F32, false, false, false, 0, 256, &p, &why), "%s", why);
    CHECK(p.tile == 6 && p.S == 1 && p.k_len == 768, "without a workspace: S %d", p.S);
    return true;
}

// one input per argument rule
static bool rejected()
{
    struct Bad { const char *what; int64_t M; int K, N, epi, a_mode; bool c_pieces, ln_bufs, stats; const char *msg; };
    static const Bad bad[] = {
        {"K not a multiple of 32", 512, 100, 768, GS_EPI_BIAS, GS_A_F32, false, false, false, "K must be a multiple of 32"},
        {"piece output with N % 32", 512, 768, 100, GS_EPI_BIAS, GS_A_F32, true, false, false, "piece output needs N % 32 == 0"},
        {"residual epilogue with piece output", 512, 768, 768, GS_EPI_RESID, GS_A_F32, true, false, false, "the residual epilogue writes f32"},
        {"a_mode 2 with K % 128", 9000, 192, 768, GS_EPI_BIAS, GS_A_LN, true, true, false, "a_mode 2 reads rows of width"},
        {"a_mode 2 with an f32 output", 9000, 768, 768, GS_EPI_BIAS, GS_A_LN, false, true, false, "a_mode 2 reads rows of width"},
        {"statistics with N % 128", 9000, 768, 192, GS_EPI_RESID, GS_A_F32, false, true, true, "row statistics ride on"},
        {"LayerNorm mode without its buffers", 9000, 768, 768, GS_EPI_BIAS, GS_A_LN, true, false, false, "need both ln_stats_dev and ln_mu_dev"},
    };
    for (const Bad &b : bad) {
        GsPlan p;
        const char *why = nullptr;
        CHECK(!gs_plan(b.M, b.K, b.N, b.epi, b.a_mode, b.c_pieces, b.ln_bufs, b.stats, 0, 256, &p, &why), "%s was planned", b.what);
        CHECK(why && std::strstr(why, b.msg), "%s: %s", b.what, why ? why : "(no message)");
    }
    // and their valid neighbours
    GsPlan p;
    const char *why = nullptr;
    CHECK(gs_plan(9000, 768, 768, GS_EPI_BIAS, GS_A_LN, true, true, false, 0, 256, &p, &why) && p.tile == 1, "%s", why ? why : "tile");
    CHECK(gs_plan(999, 768, 768, GS_EPI_RESID, GS_A_F32, false, true, true, 0, 256, &p, &why) && p.tile == 1 && p.S == 1, "%s", why ? why : "tile");
    return true;
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    const bool ok = c == "coverage" ? coverage() : c == "resources" ? resources() : c == "split_k" ? split_k() : c == "pinned" ? pinned()
                    : c == "rejected" ? rejected() : false;
    if (ok) std::printf("ok %s\n", c.c_str());
    return ok ? 0 : 1;
}
