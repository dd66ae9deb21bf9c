// The weight-buffer ring of the split GEMM's DMA-scheduled tiles (csrc/gemm_split_plan.h: gs_w_ring, gs_ring_next / gs_ring_prev and the
// buffer index of gs_dma_lds_off / gs_frag_off) on the CPU — the functions the kernel itself calls.
// usage: gemm_ring_test <case>  -> "ok <case>", exit status 0
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

// (threads of a workgroup, weight rows of a chunk per piece): the 256 x 256 tile and its half-width form (a ring of three), the
// 128 x 128 tile and its half-width form (two buffers)
struct Shape { int nthr, wrows; };
static const Shape kShapes[] = {{512, 256}, {512, 128}, {256, 128}, {256, 64}};

// For every buffer of the ring: the DMA plan writes every byte of [buf, buf + 1) x gs_w_buf_bytes exactly once and nothing outside;
// the fragment reads of the wavefronts' lanes — every strip of 32 columns = two 16-row tiles, both pieces — read every 16-byte slot
// of the same range exactly once and nothing outside, and get the (piece, row, column) they are named for.
static bool image()
{
    CHECK(gs_w_ring(512) == 3 && gs_w_ring(256) == 2, "ring sizes %d %d", gs_w_ring(512), gs_w_ring(256));
    for (const Shape &sh : kShapes) {
        const int ring = gs_w_ring(sh.nthr), bb = gs_w_buf_bytes(sh.wrows), nld = gs_dma_count(sh.wrows, sh.nthr);
        CHECK(nld * sh.nthr * 16 == bb, "threads %d rows %d: a chunk is %d pieces of 16 bytes per thread", sh.nthr, sh.wrows, nld);
        struct Src { int piece, row, col; };
        std::vector<int> written(ring * bb, 0), read(ring * bb, 0);
        std::vector<Src> src(ring * bb / 16, Src{-1, -1, -1});
        for (int buf = 0; buf < ring; ++buf) {
            for (int j = 0; j < nld; ++j)
                for (int tid = 0; tid < sh.nthr; ++tid) {
                    const int dst = gs_dma_lds_off(sh.wrows, sh.nthr, buf, j, tid >> 6) + 16 * (tid & 63);
                    CHECK(dst % 16 == 0 && dst >= buf * bb && dst + 16 <= (buf + 1) * bb, "buffer %d: piece %d of thread %d lands at %d", buf, j, tid, dst);
                    for (int b = 0; b < 16; ++b) ++written[dst + b];
                    src[dst / 16] = Src{gs_dma_piece(sh.wrows, sh.nthr, j), gs_dma_row(sh.wrows, sh.nthr, j, tid), gs_dma_src_col(tid)};
                }
            for (int piece = 0; piece < 2; ++piece)
                for (int tile = 0; tile < sh.wrows / 16; ++tile)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int off = gs_frag_off(sh.wrows, buf, piece, 0, tile, lane);
                        CHECK(off % 16 == 0 && off >= buf * bb && off + 16 <= (buf + 1) * bb, "buffer %d piece %d tile %d lane %d reads at %d", buf, piece, tile, lane, off);
                        // the kernel's sum: the lane's part once per chunk, the buffer as a scalar, (piece, tile) as an immediate
                        CHECK(off == gs_frag_off(sh.wrows, 0, 0, 0, 0, lane) + buf * bb + gs_frag_off(sh.wrows, 0, piece, 0, tile, 0),
                              "buffer %d piece %d tile %d lane %d: the offset is not the sum of its parts", buf, piece, tile, lane);
                        for (int b = 0; b < 16; ++b) ++read[off + b];
                        const Src &s = src[off / 16];
                        CHECK(s.piece == piece && s.row == 16 * tile + (lane & 15) && s.col == (lane >> 4),
                              "threads %d rows %d buffer %d piece %d tile %d lane %d: got piece %d row %d column %d", sh.nthr, sh.wrows, buf, piece, tile,
                              lane, s.piece, s.row, s.col);
                    }
        }
        for (int a = 0; a < ring * bb; ++a)
            CHECK(written[a] == 1 && read[a] == 1, "threads %d rows %d: byte %d of buffer %d written %d times, read %d times", sh.nthr, sh.wrows, a % bb,
                  a / bb, written[a], read[a]);
    }
    return true;
}

// The LDS layout of every plan of a grid of shapes: [ring buffers][epilogue blocks][bias row], nothing overlapping, all below the limit —
// also for the half-width form of a tile, whose (smaller) buffers lie in the same allocation.
static bool layout()
{
    static const int kCus[] = {8, 64, 256};
    static const int64_t kM[] = {1, 197, 261, 512, 513, 1576, 8192, 8193, 75648, 151296};
    static const int kN[] = {4, 102, 768, 1024, 1280, 2304, 3072, 4096};
    static const int kK[] = {32, 64, 96, 608, 768, 4096};
    int tiles_seen = 0;
    for (int n_cu : kCus)
        for (int64_t M : kM)
            for (int N : kN)
                for (int K : kK)
                    for (int form = 0; form < 3; ++form) {      // f32 rows -> f32; LayerNorm in the load -> pieces; pieces -> residual + statistics
                        if (form == 1 && (K % 128 || K > 1024 || N % 32)) continue;
                        if (form == 2 && (N % 128 || N > 1024)) continue;
                        GsPlan p;
                        const char *why = nullptr;
                        const bool ok = form == 0   ? gs_plan(M, K, N, GS_EPI_BIAS, GS_A_F32, false, false, false, (int64_t)34 << 20, n_cu, &p, &why)
                                        : form == 1 ? gs_plan(M, K, N, GS_EPI_GELU, GS_A_LN, true, true, false, 0, n_cu, &p, &why)
                                                    : gs_plan(M, K, N, GS_EPI_RESID, GS_A_PIECES, false, true, true, 0, n_cu, &p, &why);
                        CHECK(ok, "M %lld K %d N %d form %d: %s", (long long)M, K, N, form, why);
                        tiles_seen |= 1 << p.tile;
                        CHECK(p.lds == p.lds_loop + p.lds_epi + 4 * p.n_pad && p.lds <= GS_LDS_MAX, "M %lld N %d: lds %lld", (long long)M, N, (long long)p.lds);
                        if (p.tile == 6) continue;              // the few-rows tile stages through registers: no DMA image
                        const int ring = gs_w_ring(p.threads);
                        CHECK(ring == (p.tile == 1 ? 3 : 2), "tile %d with %d buffers", p.tile, ring);
                        CHECK(p.lds_loop == (int64_t)ring * gs_w_buf_bytes(p.cols), "tile %d: lds_loop %lld", p.tile, (long long)p.lds_loop);
                        // two workgroups of the 128 x 128 tile per CU
                        if (p.tile == 3) CHECK(2 * p.lds <= GS_LDS_MAX, "tile 3 with N %d: %lld bytes, one workgroup per CU", N, (long long)p.lds);
                        for (int wrows : {p.cols, p.half_cols}) {
                            if (!wrows) continue;
                            const int64_t bb = gs_w_buf_bytes(wrows);
                            for (int buf = 0; buf < ring; ++buf) {
                                // what the DMAs and the fragment reads of buffer buf touch: [lo, hi)
                                const int64_t lo = gs_dma_lds_off(wrows, p.threads, buf, 0, 0);
                                const int64_t hi = gs_frag_off(wrows, buf, 1, 0, wrows / 16 - 1, 15) / (GS_KC * 2) * (GS_KC * 2) + GS_KC * 2;   // its last row's end
                                CHECK(lo == buf * bb && hi == (buf + 1) * bb, "buffer %d of %d rows: [%lld, %lld)", buf, wrows, (long long)lo, (long long)hi);
                                CHECK(hi <= p.lds_loop, "buffer %d of %d rows ends at %lld, in the epilogue blocks (from %lld)", buf, wrows, (long long)hi,
                                      (long long)p.lds_loop);
                            }
                        }
                    }
    CHECK(tiles_seen == ((1 << 1) | (1 << 3) | (1 << 6)), "the grid did not reach every tile: %x", tiles_seen);
    // the bias row that no longer fits beside three buffers is refused, with the message of the limit
    GsPlan p;
    const char *why = nullptr;
    CHECK(!gs_plan(9000, 768, 20000, GS_EPI_BIAS, GS_A_F32, false, false, false, 0, 256, &p, &why), "a bias row beyond the LDS was planned");
    CHECK(why && std::strstr(why, "bsc_enc_gemm_split: N does not fit the kernel's LDS plan (bias row)"), "%s", why ? why : "(no message)");
    CHECK(gs_plan(9000, 768, 7680, GS_EPI_BIAS, GS_A_F32, false, false, false, 0, 256, &p, &why) && p.lds == GS_LDS_MAX, "N = 7680 fills the LDS exactly");
    CHECK(!gs_plan(9000, 768, 7681, GS_EPI_BIAS, GS_A_F32, false, false, false, 0, 256, &p, &why), "N = 7681 was planned");
    return true;
}

// The schedule of the ring, walked as the kernel walks it: a workgroup's tiles of n chunks each, chained or not.  Chunk c is read from
// `ring`; its request (chunk c + 2, of the next tile where this one ends) goes to gs_ring_prev(ring).  At the time of the request that
// buffer holds a chunk already read (or nothing), never the chunk being read or the one that lands next; and every chunk is read from
// the buffer its request went to.
static bool schedule()
{
    for (int b = 0; b < 3; ++b)
        CHECK(gs_ring_next(b) == (b + 1) % 3 && gs_ring_prev(b) == (b + 2) % 3 && gs_ring_prev(gs_ring_next(b)) == b, "ring arithmetic at %d", b);
    for (int n = 1; n <= 8; ++n)
        for (int tiles = 1; tiles <= 4; ++tiles)
            for (int chain = 0; chain < 2; ++chain) {
                // holds[buf] = serial number of the chunk requested into buf (tile * n + c), -1: none; done[k]: chunk k was read
                int holds[3] = {-1, -1, -1}, par = 0;
                std::vector<int> done(tiles * n, 0);
                bool primed = false;
                for (int t = 0; t < tiles; ++t) {
                    const bool has_next = chain && t + 1 < tiles && n >= 2;
                    if (!primed) {
                        holds[par] = t * n;
                        if (n > 1) holds[gs_ring_next(par)] = t * n + 1;
                    }
                    int ring = par;
                    for (int c = 0; c < n; ++c) {
                        CHECK(holds[ring] == t * n + c, "n %d tile %d chunk %d reads buffer %d, which holds chunk %d", n, t, c, ring, holds[ring]);
                        const bool w_next = c + 2 >= n;
                        if (!w_next || has_next) {
                            const int dst = gs_ring_prev(ring), k = t * n + c + 2;
                            CHECK(dst != ring && dst != gs_ring_next(ring), "request into a buffer in use");
                            CHECK(holds[dst] < 0 || done[holds[dst]], "n %d tile %d chunk %d: buffer %d still holds unread chunk %d", n, t, c, dst, holds[dst]);
                            CHECK(holds[gs_ring_next(ring)] == k - 1, "chunk %d is not the one that lands next", k - 1);
                            holds[dst] = k;
                        }
                        done[t * n + c] = 1;
                        ring = gs_ring_next(ring);
                    }
                    par = ring;
                    primed = has_next;
                }
                for (int k = 0; k < tiles * n; ++k) CHECK(done[k], "chunk %d never read", k);
            }
    return true;
}

// plan M K N form n_cu -> one line: the tile a call takes, its tile count and how many tiles a persistent workgroup enters primed by the
// tile before (the kernel's has_next) — for the GPU tests, which assert the path a shape is meant to reach.  form: 0 f32 rows or
// pieces -> f32 or pieces, 1 LayerNorm in the load -> pieces, 2 pieces -> residual + statistics
static bool plan_line(int64_t M, int K, int N, int form, int n_cu)
{
    GsPlan p;
    const char *why = nullptr;
    const bool ok = form == 0   ? gs_plan(M, K, N, GS_EPI_BIAS, GS_A_F32, false, false, false, 0, n_cu, &p, &why)
                    : form == 1 ? gs_plan(M, K, N, GS_EPI_BIAS, GS_A_LN, true, true, false, 0, n_cu, &p, &why)
                                : gs_plan(M, K, N, GS_EPI_RESID, GS_A_PIECES, false, true, true, 0, n_cu, &p, &why);
    if (!ok) { std::printf("refused %s\n", why); return true; }
    int64_t tiles = 0, chained = 0, chained_half = 0;
    for (int64_t wg = 0; wg < p.n_wg; ++wg)
        for (int64_t qv = wg >> 3; qv < p.q_virtual; qv += p.per_round) {
            const GsTile cur = gs_tile_of(p.n_tiles_n, p.n_tiles_m, p.q_full, p.q_virtual, p.cols, p.half_cols, (int)(wg & 7), qv);
            const GsTile nxt = gs_tile_of(p.n_tiles_n, p.n_tiles_m, p.q_full, p.q_virtual, p.cols, p.half_cols, (int)(wg & 7), qv + p.per_round);
            if (!cur.valid) continue;
            ++tiles;
            if (nxt.valid && nxt.half == cur.half && p.tile != 6 && K / GS_KC >= 2) { ++chained; chained_half += cur.half; }
        }
    std::printf("tile %d ring %d n_wg %lld tiles %lld chained %lld chained_half %lld lds %lld\n", p.tile, gs_w_ring(p.threads), (long long)p.n_wg,
                (long long)tiles, (long long)chained, (long long)chained_half, (long long)p.lds);
    return true;
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "plan" && argc == 7) return plan_line(std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])) ? 0 : 1;
    bool ok = false;
    if (c == "image") ok = image();
    else if (c == "layout") ok = layout();
    else if (c == "schedule") ok = schedule();
    else std::printf("unknown case '%s'\n", c.c_str());
    if (ok) std::printf("ok %s\n", c.c_str());
    return ok ? 0 : 1;
}
