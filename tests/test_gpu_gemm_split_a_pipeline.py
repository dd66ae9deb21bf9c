"""The split GEMM's LayerNorm-row operand one chunk ahead of the MFMAs (csrc/encoder_gemm.hip, PIPE, GS_A_LN only): a chunk enters
with its fp16 pieces in registers and splits the NEXT chunk's rows under its own MFMAs; chunk 0 of every tile is split at the tile's
top with that tile's LayerNorm constants, and a tile's last chunk (which splits nothing) is a second copy of the loop body.  What can
go wrong: a chunk's pieces meeting the neighbouring chunk's weights, a chained tile starting from the previous tile's rows or
constants, the unconditional A request at the end of a tile that does not chain.  The plain f32-row forms (GS_A_F32) are not
pipelined; their chained tiles of one to four chunks — shapes the suite did not reach — are held to exact integers here.  Every case
goes through SplitLinear / bsc_enc_gemm_split_ws and takes the 256 x 256 tile.  Bars as in test_gpu_gemm_split_mfma16.py — within max(1e-5, 2 e32) of an fp64 evaluation and of PyTorch's f32 op, e32 = the f32
op's own error against fp64 — except the integer cases, which are exact."""
import pytest

pytestmark = pytest.mark.gpu

M_CHAIN, N_CHAIN = 8449, 2304        # 34 x 9 tiles on 256 CUs: a second tile in another row tile, a last round of half-width tiles


def _pieces_back(p, M, K, scale=1.0):
    """(M, 2K) fp16 pieces in the chunk-interleaved layout -> (M, K) float64 of h + l"""
    v = p.view(M, K // 32, 2, 32)
    return (v[:, :, 0].double() + v[:, :, 1].double()).reshape(M, K) / scale


def _linear(K, N, seed):
    import torch
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, N).cuda().float()
    torch.nn.init.trunc_normal_(lin.weight, std=0.02)
    return lin


def _layernorm(K):
    import torch
    ln = torch.nn.LayerNorm(K, eps=1e-6).cuda()
    torch.manual_seed(K)
    ln.weight.data.uniform_(0.5, 1.5)
    ln.bias.data.uniform_(-0.5, 0.5)
    return ln


def _ln_rows(M, K):
    """rows whose mean and scale differ strongly from row to row, and their exact two-pass records"""
    import torch
    from bsc_nav_amd import encoder
    x = torch.randn(M, K, device="cuda") * (0.2 + 5 * torch.rand(M, 1, device="cuda")) + 3 * torch.randn(M, 1, device="cuda")
    mean = x.mean(1)
    stats = torch.zeros(M, encoder.LN_REC, device="cuda")
    stats[:, 0] = mean
    stats[:, 3] = ((x - mean[:, None]) ** 2).sum(1)
    return x, mean, stats


def _digit_rows(rows, K, mult):
    """(rows, K) integers in [-3, 3]: the 8-k group number `grp` of row `r` holds the eight base-7 digits of
    ((r K/8 + grp) mult) mod 7^8 — mult is coprime to 7, so every (row, group) holds another eight values"""
    import torch
    idx = (torch.arange(rows * (K // 8), dtype=torch.int64) * mult) % (7 ** 8)
    digits = torch.stack([(idx // 7 ** d) % 7 for d in range(8)], dim=1) - 3
    assert len(set(map(tuple, digits.tolist()))) == rows * (K // 8)
    return digits.reshape(rows, K).float().cuda()


@pytest.mark.parametrize("K", [128, 256])
def test_layernorm_in_the_load_across_chained_tiles(K):
    """a_ln at (8449, 2304, K): the workgroups' second tile lies in another row tile, so its first chunk must be split with ITS rows'
    mean and scale — rows differ by orders of magnitude here, constants of the wrong tile miss the bar by as much — and the last round
    runs half-width.  Piece output, epilogues 0 and 3; ln_mu receives every row's mean exactly once and its 32 guard entries stay NaN;
    two calls on the same buffers with other data.  K = 128 is four chunks (top split, two pipelined, the last), K = 256 eight.  The
    entry point admits a_ln only at K = 128 .. 1024 in steps of 128, so K = 32, 64 and 96 are left out: no pipelined tile has fewer
    than four chunks or an odd count (one-, two- and three-chunk tiles exist only for plain f32 rows, below, which are not pipelined)."""
    import torch
    import torch.nn.functional as F
    from bsc_nav_amd import encoder
    M, N = M_CHAIN, N_CHAIN
    lin, ln = _linear(K, N, M + N + K), _layernorm(K)
    sll = encoder.SplitLinear(lin, ln)
    out = torch.empty(M, 2 * N, dtype=torch.float16, device="cuda")
    mu_all = torch.empty(M + 32, device="cuda")
    torch.manual_seed(K + 1)
    for call in range(2):
        xl, mean, stats = _ln_rows(M, K)
        lin64 = F.layer_norm(xl.double(), (K,), ln.weight.double(), ln.bias.double(), 1e-6) @ lin.weight.double().t() + lin.bias.double()
        lin32 = F.layer_norm(xl, (K,), ln.weight, ln.bias, 1e-6) @ lin.weight.t() + lin.bias
        for epilogue in (0, 3):
            ref64, ref32 = (lin64, lin32) if epilogue == 0 else (F.gelu(lin64), F.gelu(lin32))
            e32 = (ref32.double() - ref64).abs().max().item()
            mu_all.fill_(float("nan"))
            sll(xl, epilogue, a_ln=True, ln_stats=stats, ln_mu=mu_all[:M], c_pieces_scale=2.0, out=out)
            got = _pieces_back(out, M, N, 2.0)
            err, err32 = (got - ref64).abs().max().item(), (got - ref32.double()).abs().max().item()
            print(f"K={K} call={call} epilogue={epilogue}: err64={err:.3g} err32={err32:.3g} e32={e32:.3g}")
            assert err <= max(1e-5, 2.0 * e32)
            assert err32 <= max(1e-5, 2.0 * e32)
            assert torch.equal(mu_all[:M], mean)
            assert torch.isnan(mu_all[M:]).all()


@pytest.mark.parametrize("K", [32, 64, 96, 128])
def test_exact_integers_across_chained_tiles(K):
    """f32 rows in at (8449, 2304, K): A = small integers, W = small integers times 2^-5, integer bias — the low pieces are zero and
    every product and partial sum is an integer below 2^13 times 2^-5, so the result must EQUAL the exact product, as f32 and as
    pieces.  A chunk's pieces against the neighbouring chunk's weights, or a tile's first chunk taken from the tile before, is a
    mismatch at any tolerance.  K = 32 is one chunk (no chained tile), 64 two, 96 an odd count, 128 four.  These forms split a chunk's
    rows at the chunk's top (they are not pipelined); the chained A request across row tiles is the one they share with a_ln."""
    import torch
    from bsc_nav_amd import encoder
    M, N = M_CHAIN, N_CHAIN
    a = _digit_rows(M, K, 2654435761)
    lin = torch.nn.Linear(K, N).cuda().float()
    lin.weight.data.copy_(_digit_rows(N, K, 40503) / 32.0)
    lin.bias.data.copy_((torch.arange(N, device="cuda") % 128).float() - 64.0)
    sl = encoder.SplitLinear(lin)
    assert not sl.pieces[1].any()
    ref = a.double() @ lin.weight.double().t() + lin.bias.double()
    assert (32 * ref).abs().max().item() < 2 ** 13 and torch.equal(32 * ref, (32 * ref).round())         # exact in f32 many times over
    outs = {"f32 rows -> f32": sl(a, 0).double(), "f32 rows -> pieces": _pieces_back(sl(a, 0, c_pieces_scale=1.0), M, N)}
    for name, out in outs.items():
        wrong = (out != ref).nonzero()
        print(f"K={K} {name}: {wrong.shape[0]} wrong elements" + (f", first at {wrong[0].tolist()}" if wrong.shape[0] else ""))
        assert torch.equal(out, ref), name


@pytest.fixture(scope="module")
def edge_layer():
    from bsc_nav_amd import encoder
    lin, ln = _linear(128, 256, 4242), _layernorm(128)
    return lin, ln, encoder.SplitLinear(lin, ln)


@pytest.mark.parametrize("M", [1, 17, 33, 257])
def test_row_edges_under_a_ln(edge_layer, M):
    """a_ln at N = 256, K = 128, piece output, with M inside a row half (1), one row into the second half (17), one row into the next
    wavefront's strip (33) and one row into a second row tile (257): rows past M are clamped reads (their constants too) and nothing
    past M is written — the output and ln_mu carry 32 guard rows of NaN."""
    import torch
    import torch.nn.functional as F
    from bsc_nav_amd import encoder
    lin, ln, sll = edge_layer
    K, N = 128, 256
    torch.manual_seed(M)
    xl, mean, stats = _ln_rows(M, K)
    ref64 = F.layer_norm(xl.double(), (K,), ln.weight.double(), ln.bias.double(), 1e-6) @ lin.weight.double().t() + lin.bias.double()
    ref32 = F.layer_norm(xl, (K,), ln.weight, ln.bias, 1e-6) @ lin.weight.t() + lin.bias
    e32 = (ref32.double() - ref64).abs().max().item()
    out_all = torch.full((M + 32, 2 * N), float("nan"), dtype=torch.float16, device="cuda")
    mu_all = torch.full((M + 32,), float("nan"), device="cuda")
    sll(xl, 0, a_ln=True, ln_stats=stats, ln_mu=mu_all[:M], c_pieces_scale=2.0, out=out_all[:M])
    got = _pieces_back(out_all[:M], M, N, 2.0)
    err, err32 = (got - ref64).abs().max().item(), (got - ref32.double()).abs().max().item()
    print(f"M={M}: err64={err:.3g} err32={err32:.3g} e32={e32:.3g}")
    assert err <= max(1e-5, 2.0 * e32)
    assert err32 <= max(1e-5, 2.0 * e32)
    assert torch.equal(mu_all[:M], mean)
    assert torch.isnan(out_all[M:]).all() and torch.isnan(mu_all[M:]).all()
