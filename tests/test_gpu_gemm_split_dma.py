"""The split GEMM with its weight chunks going global -> LDS by DMA, the swizzle on the source address (csrc/encoder_gemm.hip): the
residual epilogue in place on the 256 x 256 tile, the piece-output and LayerNorm-in-the-load forms, a ragged weight matrix.  Reference: an fp64 torch evaluation; bars as in
test_gpu_encoder_f32.py — within max(1e-5, 2 e32) of fp64 and of PyTorch's f32 op, e32 = the f32 op's own error against fp64."""
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
    torch.nn.init.trunc_normal_(lin.weight, std=0.02)       # randn rows: every 16-byte K-slice of a row differs
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


# Which tile a call takes (bsc_enc_gemm_split_ws): with ln_stats always the 256 x 256 one; without, the few-rows tiles need
# M <= 8192, so M >= 8193 takes the 256 x 256 tile too (gs_plan, csrc/gemm_split_plan.h).
#   (8200, 128, 128)  n_pad = 256 > N: the wavefront's column tiles 4 .. 7 lie beyond N
#   (8200, 768, 64)   two chunks: the shortest loop whose tiles chain (the next tile's chunk 0 lands under the second, last chunk)
#   (999, 768, 768)   statistics only (999 rows without them are a few-rows call); last row tile partly filled
#   (8449, 1024, 96)  three chunks: the weight buffer's parity alternates from tile to tile; 8449 = 33 * 256 + 1: a one-row row tile
@pytest.mark.parametrize("M,N,K,forms", [(8200, 128, 128, (False, True)), (8200, 768, 64, (False, True)), (999, 768, 768, (True,)),
                                         (8449, 1024, 96, (False, True))])
def test_residual_epilogue_in_place_on_the_big_tile(M, N, K, forms):
    """u += a W^T + b in place (out is resid), without and with the row statistics, from f32 rows and from pieces; then a second
    call on the SAME buffers with other data — stale LDS contents or a missed wait show there, not in the first call."""
    import torch
    from bsc_nav_amd import encoder
    lin = _linear(K, N, M + N + K)
    sl = encoder.SplitLinear(lin)
    a = torch.randn(M, K, device="cuda")
    ap = encoder.split_rows(a, 4.0)
    lin64 = a.double() @ lin.weight.double().t() + lin.bias.double()
    lin32 = a @ lin.weight.t() + lin.bias
    u = torch.empty(M, N, device="cuda")
    stats = torch.empty(M, encoder.LN_REC, device="cuda")
    for with_stats in forms:
        for pieces in (False, True):
            for call in range(2):
                r = torch.randn(M, N, device="cuda") * 4 + 2 * torch.randn(M, 1, device="cuda")
                ref64, ref32 = lin64 + r.double(), lin32 + r
                e32 = (ref32.double() - ref64).abs().max().item()
                u.copy_(r)
                kw = {}
                if with_stats:
                    stats.fill_(float("nan"))
                    stats[:, 2 + 2 * (N // 128):] = 0
                    stats[:, 1] = 0
                    mu = r.mean(1).contiguous()
                    kw = dict(ln_stats=stats, ln_mu=mu)
                if pieces:
                    sl(ap, 2, resid=u, out=u, a_scale=4.0, a_pieces=True, **kw)
                else:
                    sl(a, 2, resid=u, out=u, **kw)
                err64 = (u.double() - ref64).abs().max().item()
                err32 = (u - ref32).abs().max().item()
                print(f"M={M} N={N} K={K} stats={with_stats} pieces={pieces} call={call}: err64={err64:.3g} err32={err32:.3g} e32={e32:.3g}")
                assert err64 <= max(1e-5, 2.0 * e32)
                assert err32 <= max(1e-5, 2.0 * e32)
                if with_stats:
                    _check_stats(stats, mu, u, N)


@pytest.mark.parametrize("M,N", [(8200, 256), (8449, 2304)])
@pytest.mark.parametrize("K", [128, 1024])
def test_piece_output_and_layernorm_load_with_dma_weights(M, N, K):
    """Bias / GELU with piece output from f32 rows, from pieces and with the LayerNorm in the operand load (K = 128: four chunks,
    K = 1024: thirty-two): a wrong source swizzle of the weight chunks gives wrong numbers, not merely bank conflicts.  M >= 8193:
    the 256 x 256 tile; N = 256 one column tile per row tile (every tile chains to another row tile), N = 2304 nine."""
    import torch
    import torch.nn.functional as F
    from bsc_nav_amd import encoder
    lin = _linear(K, N, M + N + K)
    ln = torch.nn.LayerNorm(K, eps=1e-6).cuda()
    ln.weight.data.uniform_(0.5, 1.5)
    ln.bias.data.uniform_(-0.5, 0.5)
    x = torch.randn(M, K, device="cuda")
    sl = encoder.SplitLinear(lin)
    for epilogue in (0, 1):
        ref64 = x.double() @ lin.weight.double().t() + lin.bias.double()
        ref32 = x @ lin.weight.t() + lin.bias
        if epilogue == 1:
            ref64, ref32 = F.gelu(ref64, approximate="tanh"), F.gelu(ref32, approximate="tanh")
        e32 = (ref32.double() - ref64).abs().max().item()
        tol = max(1e-5, 2.0 * e32)
        got = _pieces_back(sl(x, epilogue, c_pieces_scale=2.0), M, N, 2.0)
        gotp = _pieces_back(sl(encoder.split_rows(x, 4.0), epilogue, a_scale=4.0, a_pieces=True, c_pieces_scale=2.0), M, N, 2.0)
        out = sl(x, epilogue)
        errs = [(got - ref64).abs().max().item(), (gotp - ref64).abs().max().item(), (out.double() - ref64).abs().max().item()]
        print(f"M={M} N={N} K={K} epilogue={epilogue}: errors vs fp64 {errs}, e32={e32:.3g}")
        assert max(errs) <= tol
        assert (out - ref32).abs().max().item() <= tol
    # LayerNorm in the load: statistics records as the embedding kernel writes them (exact two-pass mean and centred sum of squares)
    xl = x * (0.2 + 5 * torch.rand(M, 1, device="cuda")) + 3 * torch.randn(M, 1, device="cuda")
    mean = xl.mean(1)
    stats = torch.zeros(M, encoder.LN_REC, device="cuda")
    stats[:, 0] = mean
    stats[:, 3] = ((xl - mean[:, None]) ** 2).sum(1)
    mu = torch.zeros(M, device="cuda")
    sll = encoder.SplitLinear(lin, ln)
    for epilogue in (0, 1):
        ref64 = F.layer_norm(xl.double(), (K,), ln.weight.double(), ln.bias.double(), 1e-6) @ lin.weight.double().t() + lin.bias.double()
        ref32 = F.layer_norm(xl, (K,), ln.weight, ln.bias, 1e-6) @ lin.weight.t() + lin.bias
        if epilogue == 1:
            ref64, ref32 = F.gelu(ref64, approximate="tanh"), F.gelu(ref32, approximate="tanh")
        e32 = (ref32.double() - ref64).abs().max().item()
        got = _pieces_back(sll(xl, epilogue, a_ln=True, ln_stats=stats, ln_mu=mu, c_pieces_scale=2.0), M, N, 2.0)
        err = (got - ref64).abs().max().item()
        print(f"M={M} N={N} K={K} epilogue={epilogue} LayerNorm in the load: err64={err:.3g} e32={e32:.3g}")
        assert err <= max(1e-5, 2.0 * e32)


def test_weight_rows_not_a_multiple_of_256():
    """N = 2304 + 32: the weight planes are padded to 2560 rows of zeros; the bias output has 2336 columns and nothing of the
    padding appears — neither in the rows (every row's last columns are followed by the next row's first) nor behind the matrix."""
    import torch
    from bsc_nav_amd import encoder
    M, N, K = 8200, 2336, 128
    lin = _linear(K, N, 5)
    sl = encoder.SplitLinear(lin)
    assert sl.pieces.shape[1] == 2560 and not sl.pieces[:, N:].any()
    x = torch.randn(M, K, device="cuda")
    ref64 = x.double() @ lin.weight.double().t() + lin.bias.double()
    ref32 = x @ lin.weight.t() + lin.bias
    e32 = (ref32.double() - ref64).abs().max().item()
    flat = torch.full((M * N + 4096,), 12345.0, device="cuda")
    out = flat[:M * N].view(M, N)
    sl(x, 0, out=out)
    err = (out.double() - ref64).abs().max().item()
    print(f"N={N}: err64={err:.3g} e32={e32:.3g}")
    assert err <= max(1e-5, 2.0 * e32)
    assert (out - ref32).abs().max().item() <= max(1e-5, 2.0 * e32)
    assert (flat[M * N:] == 12345.0).all()
    flat16 = torch.full((M * 2 * N + 4096,), 77.0, dtype=torch.float16, device="cuda")
    cp = flat16[:M * 2 * N].view(M, 2 * N)
    sl(x, 0, out=cp, c_pieces_scale=2.0)
    assert (_pieces_back(cp, M, N, 2.0) - ref64).abs().max().item() <= max(1e-5, 2.0 * e32)
    assert (flat16[M * 2 * N:] == 77.0).all()
