"""The generated attention cases (tests/attention_cases.py) are sharp before any GPU sees them: the CPU model of the bf16
kernels stays inside the derived bound for every family, the conditions that give the families their meaning hold, and a
reference that drops the last key, lets a padded key into the softmax or reads another item's data leaves twice the bound
in every row."""
import functools

import pytest
import torch

import attention_cases as AC

B, H = 2, 3
LENGTHS = [1, 17, 33, 193, 224, 257, 288]


@functools.lru_cache(maxsize=None)
def _case(family, T):
    q, k, v = AC.make(family, B, T, H, seed=1000 + T)
    ref, A, p = AC.reference(q, k, v)
    return q, k, v, ref, A, p, AC.bf16_bound(ref, A)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("family", AC.FAMILIES)
def test_inputs_are_bf16_numbers_and_items_differ(family, T):
    q, k, v = _case(family, T)[:3]
    for x in (q, k, v):
        assert x.shape == (B, H, T, 64) and x.dtype == torch.float32 and torch.equal(x, x.bfloat16().float())
    qkv = AC.pack(q, k, v)
    assert qkv.shape == (B, T, 3, H, 64) and qkv.is_contiguous()
    assert torch.equal(qkv[1, :, 2, 1], v[1, 1]) and torch.equal(qkv[0, :, 0, 2], q[0, 2]) and torch.equal(qkv[1, :, 1, 0], k[1, 0])
    items = torch.cat([q, k, v], -1).reshape(B * H, -1)
    for a in range(B * H):
        for b in range(a + 1, B * H):
            assert not torch.equal(items[a], items[b]), (a, b)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("family", AC.FAMILIES)
def test_bf16_model_stays_inside_the_bound(family, T):
    q, k, v, ref, A, _, bound = _case(family, T)
    ratio = ((AC.emulate_bf16(q, k, v).double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"emulate_bf16 {family} T={T}: worst |out - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("T", LENGTHS)
def test_match_has_one_key_per_query(T):
    q, k, v, ref, _, p, _ = _case("match", T)
    perm = AC.match_perm(B, T, H, seed=1000 + T)
    top = p.topk(min(2, T), dim=-1)
    assert torch.equal(top.indices[..., 0], perm)
    if T > 1:
        assert top.values[..., 1].max().item() < 1e-9
    want = torch.gather(v, 2, perm.unsqueeze(-1).expand_as(v))
    assert torch.equal(ref.float().bfloat16(), want.bfloat16())
    assert torch.equal(AC.emulate_bf16(q, k, v), want)


@pytest.mark.parametrize("T", LENGTHS)
def test_negative_logits_are_far_below_zero(T):
    q, k = _case("negative", T)[:2]
    assert (q.double() @ k.double().transpose(-1, -2) / 8.0).max().item() < -12.0


@pytest.mark.parametrize("T", LENGTHS)
def test_uniform_probabilities_are_one_over_t(T):
    p = _case("uniform", T)[5]
    assert torch.equal(p, torch.full_like(p, 1.0 / T))


@pytest.mark.parametrize("T", [T for T in LENGTHS if T > 1])
def test_a_dropped_last_key_is_caught(T):
    q, k, v, ref, _, _, bound = _case("uniform", T)
    assert AC.rows_outside(AC.drop_last_key(q, k, v), ref, bound, 2.0).all()


@pytest.mark.parametrize("T", LENGTHS)
def test_a_leaked_padded_key_is_caught(T):
    q, k, v, ref, _, _, bound = _case("negative", T)
    assert AC.rows_outside(AC.leak_padded_key(q, k, v), ref, bound, 2.0).all()


@pytest.mark.parametrize("T", LENGTHS)
def test_swapped_items_are_caught(T):
    """Two items exchanged: every row of both; and every item shifted to its neighbour's data: every row."""
    q, k, v, ref, _, _, bound = _case("random", T)
    a, b = 1, 5                                                     # (b, h) = (0, 1) and (1, 2)
    out = AC.rows_outside(AC.swap_items(ref, a, b), ref, bound, 2.0).view(B * H, T)
    assert out[a].all() and out[b].all() and not out[[0, 2, 3, 4]].any()
    rolled = ref.reshape(B * H, T, 64).roll(1, 0).view_as(ref)
    assert AC.rows_outside(rolled, ref, bound, 2.0).all()
