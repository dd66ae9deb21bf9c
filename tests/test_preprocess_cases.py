"""The generated preprocessing cases (tests/preprocess_cases.py) are sharp before any GPU sees them: the ladder sits on the
kernels' limits, the fp64 reference equals PyTorch's own fp64 resize, a torch f32 model of the kernels' arithmetic stays inside
the limit max(2 e32, 2e-6), and every mutated reference — shifted taps, clipped taps not renormalised, no antialiasing, eight taps,
a centre without the half pixel, swapped channels, another unfold order, exchanged axes — leaves it at every ladder entry where it
applies."""
import functools

import pytest
import torch

import preprocess_cases as PC

ENTRIES = [(S, p, H, W) for S, p in PC.CONFIGS for H, W in PC.ladder(S, p)]
IDS = [f"S{S}-{H}x{W}" for S, p, H, W in ENTRIES]


@functools.lru_cache(maxsize=None)
def _case(family, S, p, H, W):
    img = PC.frames(family, H, W, seed=H * 1000 + W + S)
    ref = PC.reference(img, S, p)
    e32, limit = PC.limit_of(img, S, p, ref)
    return img, ref, limit


def _err(img, ref, S, p, **mut):
    return (PC.reference(img, S, p, **mut) - ref).abs().max().item()


def test_boundary_sizes_are_the_documented_ones():
    """The sizes derived from p f + 2 support + 3 <= 48 | 64 and factor <= 5.5, written out, and the constants against the kernel
    source: a change of PPT_MAXH, PPT_MAXW or PP_TAPS has to change these."""
    assert (PC.last_tiled(64, 16, PC.PPT_MAXH), PC.last_tiled(64, 16, PC.PPT_MAXW)) == (160, 216)
    assert (PC.last_tiled(56, 14, PC.PPT_MAXH), PC.last_tiled(56, 14, PC.PPT_MAXW)) == (157, 213)
    assert PC.largest_supported(64) == 352 and PC.largest_supported(56) == 308
    assert PC.rejected_sizes(64) == [(353, 64), (64, 353)]
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bsc-nav_amd", "csrc", "encoder_ops.hip")).read()
    for name, value in (("PP_TAPS", PC.PP_TAPS), ("PPT_MAXH", PC.PPT_MAXH), ("PPT_MAXW", PC.PPT_MAXW)):
        assert re.search(rf"#define {name} (\d+)", src).group(1) == str(value), name


def test_ladder_covers_every_kernel_and_edge():
    kinds = {(S, PC.kernel_of(H, W, S, p, 4)) for S, p, H, W in ENTRIES}
    assert kinds == {(S, k) for S in (64, 56) for k in ("generic", "tiled8", "tiled12")}
    assert all(PC.kernel_of(H, W, S, p, 3) == "generic" for S, p, H, W in ENTRIES)
    for S, p in PC.CONFIGS:
        lad = PC.ladder(S, p)
        th, tw = PC.last_tiled(S, p, PC.PPT_MAXH), PC.last_tiled(S, p, PC.PPT_MAXW)
        assert PC.kernel_of(th, tw, S, p, 4) == "tiled12" and (th, tw) in lad
        assert PC.kernel_of(th + 1, tw, S, p, 4) == "generic" and (th + 1, tw) in lad
        assert PC.kernel_of(th, tw + 1, S, p, 4) == "generic" and (th, tw + 1) in lad
        # factor exactly 3.0 is the last one on 8 column taps, the next size up the first on 12: both run in the tiled kernel
        assert PC.kernel_of(2 * S, 3 * S, S, p, 4) == "tiled8" and (2 * S, 3 * S) in lad
        assert PC.kernel_of(3 * S, 3 * S, S, p, 4) == "generic" and (3 * S, 3 * S) in lad
        assert {(S - 1, S), (S, S), (S + 1, S - 1)} <= set(lad)
        assert PC.kernel_of(2 * S, 3 * S + 1, S, p, 4) == "tiled12" and (2 * S, 3 * S + 1) in lad
        factors = [max(H, W) / S for H, W in lad]
        assert min(min(H, W) / S for H, W in lad) < 0.5 and max(factors) == 5.5 and 4.5 in factors and 2.0 in factors
        # 9 to 12 taps per row or column are reached
        assert any(int((PC.weights(H, S) > 0).sum(1).max()) >= 11 for H, W in lad)
    assert all(PC.frames(f, 31, 45, 1).shape == (2, 31, 45, 4) for f in PC.FAMILIES)


@pytest.mark.parametrize("S,p,H,W", ENTRIES, ids=IDS)
def test_reference_equals_pytorch_fp64(S, p, H, W):
    for family in PC.FAMILIES:
        img, ref, _ = _case(family, S, p, H, W)
        d = (PC.torch_resize(img, S, p, torch.float64) - ref).abs().max().item()
        assert d <= 1e-12, (family, d)
        assert not torch.equal(img[0], img[1]) and img[..., 3].float().std() > 50     # two images, a random alpha


@pytest.mark.parametrize("S,p,H,W", ENTRIES, ids=IDS)
def test_f32_model_of_the_kernels_stays_inside_the_limit(S, p, H, W):
    for family in PC.FAMILIES:
        img, ref, limit = _case(family, S, p, H, W)
        err = (PC.model_f32(img, S, p).double() - ref).abs().max().item()
        print(f"model_f32 S={S} {H}x{W} {family}: {err:.2e} / limit {limit:.2e} = {err / limit:.3f}")
        assert err <= limit, (family, err, limit)


@pytest.mark.parametrize("S,p,H,W", ENTRIES, ids=IDS)
def test_mutants_leave_the_limit(S, p, H, W):
    fy, fx = H / S, W / S
    checks = [("shifted taps", "random", dict(shift=1), True),
              ("clipped taps not renormalised", "impulse", dict(renorm=False), fy != 1 or fx != 1),
              ("no antialiasing", "stripes", dict(antialias=False), fy > 1 or fx > 1),
              ("eight taps", "random", dict(max_taps=8), fy > 4 or fx > 4),        # a ninth tap needs 2 f > 8
              ("centre scale * o", "random", dict(half=0.0), True),
              ("centre scale * o", "impulse", dict(half=0.0), True),
              ("channels swapped", "ramp", dict(channels=(1, 0, 2)), True),
              ("channels swapped", "ramp", dict(channels=(0, 2, 1)), True),
              ("unfold (py, px, channel)", "ramp", dict(order="yxc"), True),
              ("unfold (py, px, channel)", "random", dict(order="yxc"), True),
              ("H and W taps exchanged", "random", dict(swap_hw=True), H != W),
              ("H and W taps exchanged", "ramp", dict(swap_hw=True), H != W)]
    for name, family, mut, applies in checks:
        img, ref, limit = _case(family, S, p, H, W)
        err = _err(img, ref, S, p, **mut)
        if applies:
            assert err > 100 * limit, (name, family, err, limit)
        else:
            assert err <= 1e-12, (name, family, err)


def test_border_outputs_carry_the_unrenormalised_mutant():
    """The mutant with clipped taps not renormalised differs on border outputs only: the impulses at the corners and edge
    mid-points are what sees it."""
    S, p, H, W = 64, 16, 137, 183
    img, ref, limit = _case("impulse", S, p, H, W)
    d = (PC.reference(img, S, p, renorm=False) - ref).abs()
    g = S // p
    d = d.view(2, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(2, 3, S, S)
    assert d[:, :, 0, 0].max() > 100 * limit and d[:, :, -1, -1].max() > 100 * limit
    assert d[:, :, 3:-3, 3:-3].max() <= 1e-12


def test_other_output_forms():
    v = torch.randn(2, 16, 588) * 2
    bits = PC.pieces_bits(v, 14)
    assert bits.shape == (2, 16, 2 * 608)
    c = bits.view(torch.float16).view(2, 16, 19, 2, 32)
    h, l = c[:, :, :, 0].reshape(2, 16, 608), c[:, :, :, 1].reshape(2, 16, 608)
    assert (h[..., 588:] == 0).all() and (l[..., 588:] == 0).all()
    assert ((h.double() + l.double())[..., :588] - v.double()).abs().max() <= 2.0 ** -21 * v.abs().max()
    assert torch.equal(PC.bf16_bits(v).view(torch.bfloat16), v.bfloat16())
