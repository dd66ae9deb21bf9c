// The LDS weight image and the fragment maps of the split GEMM's DMA-scheduled tiles (csrc/gemm_split_plan.h: gs_dma_*, gs_frag_off,
// gs_acc_*) on the CPU — the functions the kernel itself calls.  usage: gemm_frag_test <case>  -> "ok <case>", exit status 0
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

// (threads of a workgroup, weight rows of a chunk per piece): the 256 x 256 tile and its half-width form, the 128 x 128 tile and its
struct Shape { int nthr, wrows; };
static const Shape kShapes[] = {{512, 256}, {512, 128}, {256, 128}, {256, 64}};

// the lane groups one ds_read_b128 is served in (one LDS cycle each when the 16 lanes touch 16 different 16-byte slots of 256 bytes)
static const int kGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                   {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// what a byte of the image holds: piece, weight row of the chunk, byte of the row's 64
struct Src { int piece, row, byte, writes; };

// "where the DMA lands it" composed with "what the fragment read takes"
static bool image()
{
    for (const Shape &sh : kShapes) {
        const int bytes = 2 * gs_w_buf_bytes(sh.wrows);
        std::vector<Src> lds(bytes, Src{-1, -1, -1, 0});
        const int nld = gs_dma_count(sh.wrows, sh.nthr);
        CHECK(nld >= 2 && nld * sh.nthr * 16 == gs_w_buf_bytes(sh.wrows), "threads %d rows %d", sh.nthr, sh.wrows);
        for (int buf = 0; buf < 2; ++buf)
            for (int j = 0; j < nld; ++j)
                for (int tid = 0; tid < sh.nthr; ++tid) {
                    const int dst = gs_dma_lds_off(sh.wrows, sh.nthr, buf, j, tid >> 6) + 16 * (tid & 63);
                    const int piece = gs_dma_piece(sh.wrows, sh.nthr, j), row = gs_dma_row(sh.wrows, sh.nthr, j, tid), col = gs_dma_src_col(tid);
                    CHECK(piece >= 0 && piece < 2 && row >= 0 && row < sh.wrows && col >= 0 && col < 4, "j %d tid %d: piece %d row %d col %d", j, tid, piece, row, col);
                    CHECK(dst >= buf * gs_w_buf_bytes(sh.wrows) && dst + 16 <= (buf + 1) * gs_w_buf_bytes(sh.wrows) && dst % 16 == 0, "j %d tid %d lands at %d", j, tid, dst);
                    for (int b = 0; b < 16; ++b) {
                        Src &s = lds[dst + b];
                        s.piece = piece; s.row = row; s.byte = 16 * col + b;
                        ++s.writes;
                    }
                }
        for (int a = 0; a < bytes; ++a) CHECK(lds[a].writes == 1, "threads %d rows %d: byte %d written %d times", sh.nthr, sh.wrows, a, lds[a].writes);
        // every (piece, row, byte) of a chunk is there once per buffer
        for (int buf = 0; buf < 2; ++buf) {
            std::vector<int> seen(2 * sh.wrows * 64, 0);
            for (int a = 0; a < gs_w_buf_bytes(sh.wrows); ++a) {
                const Src &s = lds[buf * gs_w_buf_bytes(sh.wrows) + a];
                ++seen[(s.piece * sh.wrows + s.row) * 64 + s.byte];
            }
            for (int v : seen) CHECK(v == 1, "threads %d rows %d buffer %d: a source byte lands %d times", sh.nthr, sh.wrows, buf, v);
        }
        // lane (i, g) of tile t' reads weight row 16 t' + i, halfs 8 g .. 8 g + 7, in order — whatever strip the wavefront owns
        for (int buf = 0; buf < 2; ++buf)
            for (int piece = 0; piece < 2; ++piece)
                for (int strip = 0; strip < sh.wrows; strip += 64)
                    for (int tile = 0; tile < (sh.wrows - strip) / 16; ++tile)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int off = gs_frag_off(sh.wrows, buf, piece, strip, tile, lane);
                            CHECK(off >= 0 && off + 16 <= bytes && off % 16 == 0, "read at %d", off);
                            for (int b = 0; b < 16; ++b) {
                                const Src &s = lds[off + b];
                                CHECK(s.piece == piece && s.row == strip + 16 * tile + (lane & 15) && s.byte == 16 * (lane >> 4) + b,
                                      "threads %d rows %d buffer %d piece %d tile %d lane %d byte %d: got piece %d row %d byte %d", sh.nthr, sh.wrows, buf,
                                      piece, tile, lane, b, s.piece, s.row, s.byte);
                            }
                        }
    }
    return true;
}

// worst number of lanes of one ds_read_b128 group on one 16-byte slot (mod 256 bytes), over every tile, piece and buffer; `swz`
// replaces gs_w_swz in the read address (the image's rows are 64 bytes, its blocks multiples of 256)
template <class F> static int worst_group(const Shape &sh, F swz)
{
    int worst = 0;
    for (int buf = 0; buf < 2; ++buf)
        for (int piece = 0; piece < 2; ++piece)
            for (int tile = 0; tile < sh.wrows / 16; ++tile)
                for (const auto &grp : kGroups) {
                    int hits[16] = {0};
                    for (int lane : grp) {
                        const int row = 16 * tile + (lane & 15);
                        // gs_frag_off with the swizzle under test: its column term taken out, the candidate's put in
                        const int off = gs_frag_off(sh.wrows, buf, piece, 0, tile, lane) - 16 * gs_w_col(lane & 15, lane >> 4) + 16 * ((lane >> 4) ^ swz(row));
                        const int n = ++hits[(off / 16) % 16];
                        if (n > worst) worst = n;
                    }
                }
    return worst;
}

static bool banks()
{
    for (const Shape &sh : kShapes) {
        const int now = worst_group(sh, [](int row) { return gs_w_swz(row); });
        CHECK(now == 1, "threads %d rows %d: %d lanes of a group on one slot", sh.nthr, sh.wrows, now);
        // the swizzle of the 32-row fragment (global column c ^ ((row >> 2) & 3)) under the 16-row x 4-column read: must collide, or
        // this case could not see a wrong swizzle
        const int before = worst_group(sh, [](int row) { return (row >> 2) & 3; });
        CHECK(before >= 2, "threads %d rows %d: the earlier XOR shows no conflict (%d)", sh.nthr, sh.wrows, before);
        const int none = worst_group(sh, [](int) { return 0; });
        CHECK(none == 2, "threads %d rows %d: an unswizzled image is %d-way, expected 2 (two row blocks per column and group)", sh.nthr, sh.wrows, none);
    }
    for (int row = 0; row < 256; ++row)
        for (int c = 0; c < 4; ++c) CHECK(gs_w_col(row, gs_w_col(row, c)) == c, "row %d column %d: not an involution", row, c);
    return true;
}

// (lane, row half, tile, register) -> (row, column) covers the wavefront's 32 x NT 32 strip once; the four registers of a tile are four
// consecutive columns from a multiple of 4 on, so the float4 of bias values at register 0's column serves the quad
static bool epilogue()
{
    for (int NT : {8, 4, 2}) {
        const int cols = NT * 32;
        std::vector<int> seen(32 * cols, 0);
        for (int lane = 0; lane < 64; ++lane)
            for (int half = 0; half < 2; ++half)
                for (int tile = 0; tile < 2 * NT; ++tile)
                    for (int r = 0; r < 4; ++r) {
                        const int row = gs_acc_row(lane, half), col = gs_acc_col(lane, tile, r);
                        CHECK(row >= 0 && row < 32 && col >= 0 && col < cols, "lane %d half %d tile %d r %d -> (%d, %d)", lane, half, tile, r, row, col);
                        CHECK(col == gs_acc_col(lane, tile, 0) + r && gs_acc_col(lane, tile, 0) % 4 == 0, "lane %d tile %d: the quad's columns", lane, tile);
                        // the kernel stages quad q = 2 half + (tile & 1) of the 32-column tile (tile >> 1) at column gs_acc_col(lane, tile & 1, 0)
                        CHECK(col - 32 * (tile >> 1) == gs_acc_col(lane, tile & 1, r), "lane %d tile %d: column within the 32-column tile", lane, tile);
                        ++seen[row * cols + col];
                    }
        for (int e = 0; e < 32 * cols; ++e) CHECK(seen[e] == 1, "NT %d: element (%d, %d) held %d times", NT, e / cols, e % cols, seen[e]);
    }
    // the activation side of the same lane: rows i and i + 16, the weight fragment's k group — row half h of the accumulator is the
    // activation row half h
    for (int lane = 0; lane < 64; ++lane) CHECK(gs_acc_row(lane, 1) == gs_acc_row(lane, 0) + 16 && gs_acc_row(lane, 0) == (lane & 15), "lane %d", lane);
    return true;
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    bool ok = false;
    if (c == "image") ok = image();
    else if (c == "banks") ok = banks();
    else if (c == "epilogue") ok = epilogue();
    else std::printf("unknown case '%s'\n", c.c_str());
    if (ok) std::printf("ok %s\n", c.c_str());
    return ok ? 0 : 1;
}
