"""The split GEMM's 256 x 256 tile with its weight chunks in a ring of three LDS buffers, requested two chunks ahead
(csrc/encoder_gemm.hip, RING3): chunk counts that leave the ring unfilled, fill it and wrap it, an odd count, partial row and column
tiles, and persistent workgroups that enter a tile primed by the tile before with fewer chunks than the ring is deep.  Reference: an
fp64 torch evaluation; bars as in test_gpu_gemm_split_dma.py — within max(1e-5, 2 e32) of fp64, e32 = PyTorch's f32 op's own error.

Every shape runs in those of the forward's four forms that the kernel's plan admits (gs_plan, csrc/gemm_split_plan.h):
  ln       LayerNorm in the load -> pieces (qkv)                 needs K % 128 == 0, K <= 1024
  ln_gelu  the same + GELU (erf) -> pieces (fc1)                 the same
  st16     pieces in (a_scale 16) + residual + statistics (proj) needs N % 128 == 0, N <= 1024
  st4      the same at a_scale 4 (fc2)                           the same
Where a rule refuses a form the test asserts that the plan refuses it and runs the nearest form the shape admits through the same main loop: f32 rows
-> pieces with the same epilogue for ln / ln_gelu, pieces in + residual without statistics for st16 / st4.  The path a shape takes — the
256 x 256 tile, three buffers, chained tiles — is asserted from the plan itself, computed by tests/host/gemm_ring_main.cpp on the CPU.
(8448, 2048, 96) takes 272 tiles, but its second round runs as half-width tiles and a full tile never primes a half tile: no tile of
it is chained.  (8448, 2560, 96), 330 whole tiles, is the shape with chained tiles of three chunks; (25500, 1024, 128), 400 tiles, the
one that chains in all four forms."""
import os
import subprocess

import pytest

from test_gpu_gemm_split_dma import _check_stats, _linear, _pieces_back

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gemm_ring_plan") / "gemm_ring_test"
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "host", "gemm_ring_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def plan(M, K, N, form):
        import torch
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        out = subprocess.run([str(exe), "plan", str(M), str(K), str(N), str(form), str(n_cu)], capture_output=True, text=True, timeout=60).stdout.split()
        if out[0] == "refused":
            return None
        return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}
    return plan


def _ln_records(x):
    import torch
    from bsc_nav_amd import encoder
    mean = x.mean(1)
    stats = torch.zeros(x.shape[0], encoder.LN_REC, device="cuda")
    stats[:, 0] = mean
    stats[:, 3] = ((x - mean[:, None]) ** 2).sum(1)
    return stats, torch.zeros(x.shape[0], device="cuda")


def _run_forms(plan_of, M, N, K, chained):
    import torch
    import torch.nn.functional as F
    from bsc_nav_amd import encoder
    lin = _linear(K, N, M + N + K)
    ln = torch.nn.LayerNorm(K, eps=1e-6).cuda()
    ln.weight.data.uniform_(0.5, 1.5)
    ln.bias.data.uniform_(-0.5, 0.5)
    x = torch.randn(M, K, device="cuda")
    # ---- the two piece-output forms -------------------------------------------------------------------------------------------------
    p_ln = plan_of(M, K, N, 1)
    assert (p_ln is not None) == (K % 128 == 0 and K <= 1024 and N % 32 == 0)
    p = p_ln or plan_of(M, K, N, 0)
    assert p["tile"] == 1 and p["ring"] == 3 and (p["chained"] > 0) == chained, p
    if p_ln:
        xl = x * (0.2 + 5 * torch.rand(M, 1, device="cuda")) + 3 * torch.randn(M, 1, device="cuda")
        stats, mu = _ln_records(xl)
        sl = encoder.SplitLinear(lin, ln)
        lin64 = F.layer_norm(xl.double(), (K,), ln.weight.double(), ln.bias.double(), 1e-6) @ lin.weight.double().t() + lin.bias.double()
        lin32 = F.layer_norm(xl, (K,), ln.weight, ln.bias, 1e-6) @ lin.weight.t() + lin.bias
    else:
        sl = encoder.SplitLinear(lin)
        lin64 = x.double() @ lin.weight.double().t() + lin.bias.double()
        lin32 = x @ lin.weight.t() + lin.bias
    if N % 32 == 0:
        for epilogue in (0, 3):
            ref64, ref32 = (lin64, lin32) if epilogue == 0 else (F.gelu(lin64), F.gelu(lin32))
            e32 = (ref32.double() - ref64).abs().max().item()
            for call in range(2):       # the second call on warm buffers: stale LDS contents or a missed wait show there
                got = sl(xl, epilogue, a_ln=True, ln_stats=stats, ln_mu=mu, c_pieces_scale=2.0) if p_ln else sl(x, epilogue, c_pieces_scale=2.0)
                err = (_pieces_back(got, M, N, 2.0) - ref64).abs().max().item()
                print(f"M={M} N={N} K={K} {'LayerNorm in the load' if p_ln else 'f32 rows'} epilogue={epilogue} call={call}: err64={err:.3g} e32={e32:.3g}")
                assert err <= max(1e-5, 2.0 * e32)
        del ref64, ref32
    else:                                # piece output needs N % 32 == 0: the f32-output form of the same loop
        e32 = (lin32.double() - lin64).abs().max().item()
        out = encoder.SplitLinear(lin)(x, 0)
        err = (out.double() - lin64).abs().max().item()
        print(f"M={M} N={N} K={K} f32 rows -> f32: err64={err:.3g} e32={e32:.3g}")
        assert err <= max(1e-5, 2.0 * e32)
    del lin64, lin32
    # ---- the two residual forms -----------------------------------------------------------------------------------------------------
    p_st = plan_of(M, K, N, 2)
    assert (p_st is not None) == (N % 128 == 0 and N <= 1024)
    assert p_st is None or (p_st["tile"] == 1 and p_st["ring"] == 3 and (p_st["chained"] > 0) == chained), p_st
    sl = encoder.SplitLinear(lin)
    a64 = x.double() @ lin.weight.double().t() + lin.bias.double()
    a32 = x @ lin.weight.t() + lin.bias
    u = torch.empty(M, N, device="cuda")
    stats = torch.empty(M, encoder.LN_REC, device="cuda")
    for a_scale in (16.0, 4.0):
        xp = encoder.split_rows(x, a_scale)
        for call in range(2):
            r = torch.randn(M, N, device="cuda") * 4 + 2 * torch.randn(M, 1, device="cuda")
            ref64, ref32 = a64 + r.double(), a32 + r
            e32 = (ref32.double() - ref64).abs().max().item()
            u.copy_(r)
            kw = {}
            if p_st:
                stats.fill_(float("nan"))
                stats[:, 2 + 2 * (N // 128):] = 0
                stats[:, 1] = 0
                mu = r.mean(1).contiguous()
                kw = dict(ln_stats=stats, ln_mu=mu)
            sl(xp, 2, resid=u, out=u, a_scale=a_scale, a_pieces=True, **kw)
            err64 = (u.double() - ref64).abs().max().item()
            err32 = (u - ref32).abs().max().item()
            print(f"M={M} N={N} K={K} residual a_scale={a_scale} stats={bool(p_st)} call={call}: err64={err64:.3g} err32={err32:.3g} e32={e32:.3g}")
            assert err64 <= max(1e-5, 2.0 * e32)
            assert err32 <= max(1e-5, 2.0 * e32)
            if p_st:
                _check_stats(stats, mu, u, N)


@pytest.mark.parametrize("K", [32, 64, 96, 128])
def test_ring_not_filled_filled_wrapped(plan_of, K):
    """1, 2, 3, 4 chunks: one chunk primed and nothing requested; two primed; the first request goes to the third buffer; the ring wraps.
    M = 8200: 33 row tiles, the last of 8 rows; N = 768: the statistics epilogue is admitted."""
    _run_forms(plan_of, 8200, 768, K, chained=False)


def test_odd_chunk_count(plan_of):
    """K = 608: 19 chunks, the ring wraps six times and a tile ends one buffer further on than it began."""
    _run_forms(plan_of, 8200, 768, 608, chained=False)


def test_partial_row_and_column_tile(plan_of):
    """M = 8193 + 17: a last row tile of 18 rows; N = 272: the second column tile holds 16 columns of 256 (no piece output: N % 32)."""
    _run_forms(plan_of, 8193 + 17, 272, 128, chained=False)


def test_more_tiles_than_workgroups_with_three_chunks(plan_of):
    """M = 8448, N = 2048, K = 96: 264 tile positions on 256 workgroups; the plan runs the second round as half-width tiles, which a whole
    tile does not prime — every tile of this shape has its own prologue, some workgroups a second one (of the half-width form)."""
    _run_forms(plan_of, 8448, 2048, 96, chained=False)


def test_chained_tiles_shorter_than_the_ring(plan_of):
    """N = 2560: 330 whole tiles, 74 of them primed by the tile before — whose three chunks request the next tile's first two from its
    second and third chunk on, one chunk after its own prologue."""
    _run_forms(plan_of, 8448, 2560, 96, chained=True)


def test_chained_tiles_in_all_four_forms(plan_of):
    """400 tiles of four chunks on 256 workgroups, 144 chained; K = 128 and N = 1024 admit the LayerNorm load and the statistics."""
    _run_forms(plan_of, 25500, 1024, 128, chained=True)


def test_the_128_tile_keeps_two_buffers(plan_of):
    """M = 1576 takes the 128 x 128 tile, which was not changed: two buffers, requested at the chunk's top."""
    p = plan_of(1576, 768, 768, 0)
    assert p["tile"] == 3 and p["ring"] == 2 and 2 * p["lds"] <= 160 * 1024, p
