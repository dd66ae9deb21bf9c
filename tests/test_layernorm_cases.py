"""The generated cases of the bf16 row kernels (tests/layernorm_cases.py) are sharp before any GPU sees them: a torch f32 model
of the kernels' arithmetic, in the kernels' summation order and in torch's, stays inside the derived elementwise bound on every
case and every element, and every mutated reference — variance over width - 1, no eps or 1e-5, gamma and beta one group to the
right, a row offset of one, pos on the register rows, pos[r] for the patch rows, a repeated row in a group of four, bias_sum
rounded to bf16 — leaves it."""
import functools
import zlib

import pytest
import torch

import layernorm_cases as LC

OPS = (("add", LC.ADD_ROWS), ("embed", LC.EMBED_SHAPES), ("final", LC.FINAL_SHAPES), ("bias", LC.BIAS_SHAPES))


def seed_of(*a):
    return zlib.crc32(" ".join(map(str, a)).encode())


def rows_of(op, z, shape, dtype=torch.float64, **mut):
    if op == "add":
        return LC.rows_add(z, **mut)
    if op == "embed":
        return LC.rows_embed(z, shape, **mut)
    if op == "final":
        return LC.rows_final(z, shape, **mut)
    return LC.rows_bias(z, shape, dtype=dtype, **mut)


@functools.lru_cache(maxsize=None)
def _case(op, family, shape, width):
    z = LC.make(op, family, shape, width, seed_of(op, family, shape, width))
    v = rows_of(op, z, shape)
    ref, bound = LC.layernorm64(v, z["gamma"], z["beta"])
    return z, shape, v, ref, bound


@pytest.mark.parametrize("width", LC.WIDTHS)
@pytest.mark.parametrize("op,shapes", OPS, ids=[o for o, _ in OPS])
def test_f32_model_stays_inside_the_bound(op, shapes, width):
    for family in LC.FAMILIES:
        worst = 0.0
        for shape in shapes:
            z, shape, v, ref, bound = _case(op, family, shape, width)
            v32 = rows_of(op, z, shape, dtype=torch.float32)
            assert v32.dtype == torch.float32 and (op == "bias" or torch.equal(v32.double(), v.double()))
            for order in ("kernel", "torch"):
                y = LC.model32(v32, z["gamma"], z["beta"], order)
                r = LC.worst_ratio(y, ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (op, family, shape, width, order, r)
            if family == "const":
                assert float(((v.double() - v.double()[:, :1]) != 0).sum()) == 0          # variance 0
                assert torch.equal(LC.model32(v32, z["gamma"], z["beta"]), z["beta"].expand_as(v32))
        print(f"model32 {op} width {width} {family}: worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("width", LC.WIDTHS)
def test_inputs_are_what_the_families_say(width):
    for family in LC.FAMILIES:
        z, _, v, ref, bound = _case("add", family, 5, width)
        for k in ("x", "delta", "gamma", "beta"):
            assert torch.equal(z[k], LC.bf16(z[k])), k
        assert len({tuple(r.tolist()) for r in z["x"]}) == 5                # every row different
        var = v.double().var(-1, unbiased=False)
        if family == "tiny":
            assert 0.3e-6 < var.min() and var.max() < 3e-6                  # about eps
        if family == "mean30":
            assert (v.mean(-1) - 30).abs().max() < 1 and (var - 1).abs().max() < 0.3
        if family == "gamma0":
            small = z["gamma"].abs() < 0.01
            assert small.sum() == width // 4 and (z["gamma"] == 0).sum() == width // 8
    b = LC.make("bias", "randn", (2, 6, 1), width, 3)["bias_sum"]
    assert not torch.equal(b, LC.bf16(b))


@pytest.mark.parametrize("width", LC.WIDTHS)
def test_statistics_mutants_leave_the_bound(width):
    """variance over width - 1 (randn, on the very cases the GPU test runs: every row has elements where beta nearly cancels the
    normalised value, the only place where a relative change of 1 / (2 width) shows under one bf16 rounding), eps omitted or 1e-5
    (tiny), gamma and beta one group of four to the right (every family; on constant rows it is y = beta alone that moves)"""
    for op, shapes in OPS:
        for shape in shapes:
            z, shape, v, ref, bound = _case(op, "randn", shape, width)
            out = LC.outside(LC.layernorm64(v, z["gamma"], z["beta"], ddof=1)[0], ref, bound)
            assert out.all(), (op, shape, "variance over width - 1 stays inside the bound", int(out.sum()), out.numel())
    for op, shapes in OPS:
        for shape in shapes:
            z, shape, v, ref, bound = _case(op, "tiny", shape, width)
            for eps in (0.0, 1e-5):
                assert LC.outside(LC.layernorm64(v, z["gamma"], z["beta"], eps=eps)[0], ref, bound).all(), (op, shape, eps)
            for family in LC.FAMILIES:
                z, shape, v, ref, bound = _case(op, family, shape, width)
                assert LC.outside(LC.layernorm64(v, z["gamma"], z["beta"], group_shift=1)[0], ref, bound).all(), (op, family, shape)


@pytest.mark.parametrize("width", LC.WIDTHS)
@pytest.mark.parametrize("family", [f for f in LC.FAMILIES if f != "const"])
def test_row_index_mutants_leave_the_bound(family, width):
    """Every row holds other data: a row read one further, pos where it does not belong or from another row, a repeated row."""
    for op, shapes in (("final", LC.FINAL_SHAPES), ("bias", LC.BIAS_SHAPES)):
        for shape in shapes:
            z, shape, v, ref, bound = _case(op, family, shape, width)
            B, T, skip = shape
            bad = LC.layernorm64(rows_of(op, z, shape, row_off=1), z["gamma"], z["beta"])[0]
            out = LC.outside(bad, ref, bound).view(B, T - skip)
            assert out[:, :-1].all() and out[:-1].all(), (op, shape)      # all but the very last row (its read is clamped)
            rep = LC.outside(LC.repeat_in_groups(ref), ref, bound)
            n = B * (T - skip)
            want = torch.tensor([(i % 4 == 3 or i == n - 1) and i % 4 != 0 for i in range(n)])
            assert torch.equal(rep, want), (op, shape)
    for shape in LC.EMBED_SHAPES:
        z, shape, v, ref, bound = _case("embed", family, shape, width)
        B, T, R = shape
        if R:
            out = LC.outside(LC.layernorm64(LC.rows_embed(z, shape, pos_on_registers=True), z["gamma"], z["beta"])[0], ref, bound).view(B, T)
            assert out[:, 1:1 + R].all() and not out[:, 0].any() and not out[:, 1 + R:].any(), shape
            out = LC.outside(LC.layernorm64(LC.rows_embed(z, shape, pos_by_row=True), z["gamma"], z["beta"])[0], ref, bound).view(B, T)
            assert out[:, 1 + R:].all() and not out[:, :1 + R].any(), shape


@pytest.mark.parametrize("width", LC.WIDTHS)
def test_bias_rounded_to_bf16_leaves_the_bound(width):
    for family in ("randn", "mean30", "gamma0"):
        for shape in LC.BIAS_SHAPES:
            z, shape, v, ref, bound = _case("bias", family, shape, width)
            bad = LC.layernorm64(LC.rows_bias(z, shape, round_bias=True), z["gamma"], z["beta"])[0]
            assert LC.outside(bad, ref, bound).any(), (family, shape)
