"""The split GEMM's 256 x 256 tile on v_mfma_f32_16x16x32_f16 (csrc/encoder_gemm.hip; lane maps in csrc/gemm_split_plan.h): a lane holds
rows i and i + 16 of its wavefront's 32, eight k per chunk, and four consecutive columns per 16-column tile.  Every case goes
through SplitLinear / bsc_enc_gemm_split_ws and takes the 256 x 256 tile (ln_stats / a_ln take it at any M; without them M >= 8193).
Bars as in test_gpu_gemm_split_dma.py — within max(1e-5, 2 e32) of an fp64 evaluation and of PyTorch's f32 op, e32 = the f32 op's own
error against fp64 — except the integer case, which is exact."""
import pytest

pytestmark = pytest.mark.gpu


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


def _check_stats(stats, mu, u, Wd):
    import torch
    assert torch.equal(stats[:, 0], mu)
    sa = stats[:, 2::2].double().sum(1)
    sb = stats[:, 3::2].double().sum(1)
    mean = stats[:, 0].double() + sa / Wd
    var = sb / Wd - (sa / Wd) ** 2
    u64 = u.double()
    assert (mean - u64.mean(1)).abs().max().item() < 1e-5
    assert ((var - u64.var(1, unbiased=False)).abs() / u64.var(1, unbiased=False)).max().item() < 2e-6


def _digit_rows(rows, K, mult):
    """(rows, K) integers in [-3, 3]: the 8-k group number `grp` of row `r` holds the eight base-7 digits of
    ((r K/8 + grp) mult) mod 7^8 — mult is coprime to 7, so every (row, group) holds another eight values"""
    import torch
    idx = (torch.arange(rows * (K // 8), dtype=torch.int64) * mult) % (7 ** 8)
    digits = torch.stack([(idx // 7 ** d) % 7 for d in range(8)], dim=1) - 3
    assert len(set(map(tuple, digits.tolist()))) == rows * (K // 8)
    return digits.reshape(rows, K).float().cuda()


@pytest.mark.parametrize("K", [32, 64, 96])
def test_exact_integers(K):
    """A = small integers, W = small integers times 2^-5, integer bias: the low pieces are zero and every product and partial sum is
    an integer below 2^13 times 2^-5, so the result must EQUAL the exact product — a swapped row half, k group or column
    quad is a mismatch whatever the tolerance.  K = 32 is one chunk (no chained tile), 64 and 96 chain; N = 128 leaves the
    wavefront's column tiles 8 .. 15 beyond N; M = 8193 + 17: the last row tile holds 18 rows (row half 1 has two)."""
    import torch
    from bsc_nav_amd import encoder
    M, N = 8193 + 17, 128
    a = _digit_rows(M, K, 2654435761)
    lin = torch.nn.Linear(K, N).cuda().float()
    lin.weight.data.copy_(_digit_rows(N, K, 40503) / 32.0)
    lin.bias.data.copy_(torch.arange(N, device="cuda").float() - 64.0)
    sl = encoder.SplitLinear(lin)
    assert sl.scale == 64.0 and not sl.pieces[1].any()
    ref = a.double() @ lin.weight.double().t() + lin.bias.double()
    assert (32 * ref).abs().max().item() < 2 ** 13 and torch.equal(32 * ref, (32 * ref).round())         # exact in f32 many times over
    ap = encoder.split_rows(a, 1.0)
    assert torch.equal(_pieces_back(ap, M, K), a.double())
    outs = {"f32 rows -> f32": sl(a, 0).double(), "pieces -> f32": sl(ap, 0, a_scale=1.0, a_pieces=True).double(),
            "f32 rows -> pieces": _pieces_back(sl(a, 0, c_pieces_scale=1.0), M, N)}
    for name, out in outs.items():
        wrong = (out != ref).nonzero()
        print(f"K={K} {name}: {wrong.shape[0]} wrong elements" + (f", first at {wrong[0].tolist()}" if wrong.shape[0] else ""))
        assert torch.equal(out, ref), name


@pytest.fixture(scope="module")
def edge_layers():
    from bsc_nav_amd import encoder
    lins = {N: _linear(128, N, 1000 + N) for N in (128, 768)}
    return {N: (lin, encoder.SplitLinear(lin)) for N, lin in lins.items()}


@pytest.mark.parametrize("N", [128, 768])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 33, 255, 257])
def test_row_half_edges(edge_layers, M, N):
    """M around the row halves of a wavefront's strip (15 / 16 / 17), its end (31 / 33) and a row tile's end (255 / 257): u += a W^T + b
    in place with the row statistics, from f32 rows and from pieces, called twice on the same buffers with other data.  The output
    and statistics buffers carry 32 guard rows of NaN past M."""
    import torch
    from bsc_nav_amd import encoder
    K = 128
    lin, sl = edge_layers[N]
    torch.manual_seed(M * 1000 + N)
    nan = float("nan")
    u_all = torch.full((M + 32, N), nan, device="cuda")
    st_all = torch.full((M + 32, encoder.LN_REC), nan, device="cuda")
    u, stats = u_all[:M], st_all[:M]
    for pieces in (False, True):
        for call in range(2):
            a = torch.randn(M, K, device="cuda")
            r = torch.randn(M, N, device="cuda") * 4 + 2 * torch.randn(M, 1, device="cuda")
            ref64 = a.double() @ lin.weight.double().t() + lin.bias.double() + r.double()
            ref32 = a @ lin.weight.t() + lin.bias + r
            e32 = (ref32.double() - ref64).abs().max().item()
            u.copy_(r)
            stats.fill_(nan)
            stats[:, 2 + 2 * (N // 128):] = 0
            stats[:, 1] = 0
            mu = r.mean(1).contiguous()
            if pieces:
                sl(encoder.split_rows(a, 4.0), 2, resid=u, out=u, a_scale=4.0, a_pieces=True, ln_stats=stats, ln_mu=mu)
            else:
                sl(a, 2, resid=u, out=u, ln_stats=stats, ln_mu=mu)
            err64 = (u.double() - ref64).abs().max().item()
            err32 = (u - ref32).abs().max().item()
            print(f"M={M} N={N} pieces={pieces} call={call}: err64={err64:.3g} err32={err32:.3g} e32={e32:.3g}")
            assert err64 <= max(1e-5, 2.0 * e32)
            assert err32 <= max(1e-5, 2.0 * e32)
            _check_stats(stats, mu, u, N)
            assert torch.isnan(u_all[M:]).all() and torch.isnan(st_all[M:]).all()


@pytest.mark.parametrize("K", [128, 768])
def test_layernorm_in_the_load(K):
    """a_ln with the constants of both of a lane's rows: M = 8192 + 17 (the last row tile holds 17 rows: one in the second row half),
    N = 256, epilogues 0 and 3 (erf GELU) with piece output.  ln_mu gets the mean of every row below M exactly once — the record's
    shift plus nothing, as the records here are exact two-pass ones — and its guard entries stay as they were."""
    import torch
    import torch.nn.functional as F
    from bsc_nav_amd import encoder
    M, N = 8192 + 17, 256
    lin = _linear(K, N, M + N + K)
    ln = torch.nn.LayerNorm(K, eps=1e-6).cuda()
    torch.manual_seed(K)
    ln.weight.data.uniform_(0.5, 1.5)
    ln.bias.data.uniform_(-0.5, 0.5)
    xl = torch.randn(M, K, device="cuda") * (0.2 + 5 * torch.rand(M, 1, device="cuda")) + 3 * torch.randn(M, 1, device="cuda")
    mean = xl.mean(1)
    stats = torch.zeros(M, encoder.LN_REC, device="cuda")
    stats[:, 0] = mean
    stats[:, 3] = ((xl - mean[:, None]) ** 2).sum(1)
    sll = encoder.SplitLinear(lin, ln)
    lin64 = F.layer_norm(xl.double(), (K,), ln.weight.double(), ln.bias.double(), 1e-6) @ lin.weight.double().t() + lin.bias.double()
    lin32 = F.layer_norm(xl, (K,), ln.weight, ln.bias, 1e-6) @ lin.weight.t() + lin.bias
    for epilogue in (0, 3):
        ref64, ref32 = (lin64, lin32) if epilogue == 0 else (F.gelu(lin64), F.gelu(lin32))
        e32 = (ref32.double() - ref64).abs().max().item()
        mu_all = torch.full((M + 32,), float("nan"), device="cuda")
        got = _pieces_back(sll(xl, epilogue, a_ln=True, ln_stats=stats, ln_mu=mu_all[:M], c_pieces_scale=2.0), M, N, 2.0)
        err = (got - ref64).abs().max().item()
        print(f"K={K} epilogue={epilogue} LayerNorm in the load: err64={err:.3g} e32={e32:.3g}")
        assert err <= max(1e-5, 2.0 * e32)
        assert torch.equal(mu_all[:M], mean)
        assert torch.isnan(mu_all[M:]).all()


def test_chained_tiles_and_half_width_round():
    """(8449, 2304, 128) with piece output: 34 row tiles x 9 column tiles, so the workgroups take a second tile (its first weight chunk
    lands under the previous tile's last chunk) and the last round runs as half-width tiles (four column tiles of 16 x 2 per
    wavefront: one batch of weight fragments).  Two calls on the same buffers with other data."""
    import torch
    from bsc_nav_amd import encoder
    M, N, K = 8449, 2304, 128
    lin = _linear(K, N, M + N + K)
    sl = encoder.SplitLinear(lin)
    out = torch.empty(M, 2 * N, dtype=torch.float16, device="cuda")
    for call in range(2):
        x = torch.randn(M, K, device="cuda") * (1 + call)
        ref64 = x.double() @ lin.weight.double().t() + lin.bias.double()
        e32 = ((x @ lin.weight.t() + lin.bias).double() - ref64).abs().max().item()
        sl(x, 0, out=out, c_pieces_scale=2.0)
        err = (_pieces_back(out, M, N, 2.0) - ref64).abs().max().item()
        sl(encoder.split_rows(x, 4.0), 0, out=out, a_scale=4.0, a_pieces=True, c_pieces_scale=2.0)
        errp = (_pieces_back(out, M, N, 2.0) - ref64).abs().max().item()
        print(f"call={call}: err64 f32 rows {err:.3g}, pieces {errp:.3g}, e32={e32:.3g}")
        assert max(err, errp) <= max(1e-5, 2.0 * e32)
