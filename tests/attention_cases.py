"""Inputs, an fp64 reference, a derived error bound and a CPU model of the in-tree attention kernels (k_attention,
k_attention32 in csrc/encoder_ops.hip; k_attention_split in csrc/encoder_gemm.hip), shared by tests/test_attention_cases.py
(CPU: the cases are sharp — a dropped key, a leaked padded key, a swapped item leave the bound) and tests/test_gpu_attention.py.

torch only, no GPU needed to import.  q, k, v are (B, H, T, 64) f32 tensors whose values are already bf16 numbers (both
kernels then see the same inputs; the split kernel's l pieces of them are zero — `random_f32` is the one family that is not
rounded, for the split kernel alone).  Every (b, h) item holds different data.

    random     randn * 1.5 for q, k, v: the inputs of the older tests
    uniform    q = 0, so every probability is exactly 1 / T; v[t, d] = 1 + (t + item) % 5 where d == t % 64, else 0: a
               dropped or doubled key moves one output element by a whole term (k is random, it does not matter)
    negative   one random +-1 vector s per item; q = 1.5 s + 0.25 randn, k = -1.5 s + 0.25 randn, v = randn + 2: every real
               logit is about -16 (-18 +- 0.5), so a padded key that enters the softmax with logit 0 takes all the weight
    match      k rows are random +-3 sign vectors, q[t] = k[perm[t]], v = 2 randn: the self logit is 72, the others at most
               about 40 — the output is v[perm[t]], exactly so after the rounding to bf16: |v| >= 2^-6, so the other keys'
               share (probabilities below 1e-9) is far below half a unit in the last place of every element
"""
import torch

FAMILIES = ("random", "uniform", "negative", "match")
D = 64


def _bf16(x):
    return x.bfloat16().float()


def _make(family, B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, H, T, D)
    rn = lambda *s: torch.randn(*s, generator=g)
    perm = None
    if family in ("random", "random_f32"):
        q, k, v = rn(*shape) * 1.5, rn(*shape) * 1.5, rn(*shape) * 1.5
    elif family == "uniform":
        q, k = torch.zeros(shape), rn(*shape) * 1.5
        t = torch.arange(T).view(1, 1, T, 1)
        item = torch.arange(B * H).view(B, H, 1, 1)
        d = torch.arange(D).view(1, 1, 1, D)
        v = torch.where(d == t % D, 1.0 + ((t + item) % 5).float(), torch.zeros(()))
    elif family == "negative":
        s = torch.randint(0, 2, (B, H, 1, D), generator=g).float() * 2 - 1
        q, k, v = 1.5 * s + 0.25 * rn(*shape), -1.5 * s + 0.25 * rn(*shape), rn(*shape) + 2
    elif family == "match":
        k = torch.randint(0, 2, shape, generator=g).float() * 6 - 3
        perm = torch.stack([torch.randperm(T, generator=g) for _ in range(B * H)]).view(B, H, T)
        q = torch.gather(k, 2, perm.unsqueeze(-1).expand(shape))
        v = 2 * rn(*shape)
        v = torch.where(v.abs() < 2.0 ** -6, torch.full_like(v, 2.0 ** -6).copysign(v), v)    # no zeros: see the module's text
    else:
        raise ValueError(family)
    if family != "random_f32":
        q, k, v = _bf16(q), _bf16(k), _bf16(v)
    return q, k, v, perm


def make(family, B, T, H, seed):
    """q, k, v: (B, H, T, 64) f32, bf16 numbers (random_f32 excepted)."""
    return _make(family, B, T, H, seed)[:3]


def match_perm(B, T, H, seed):
    """(B, H, T) int64: the key that query t of make("match", ...) equals — its output row is v[perm[t]]."""
    return _make("match", B, T, H, seed)[3]


def pack(q, k, v):
    """(B, T, 3, H, 64), contiguous: the layout the qkv GEMM leaves and the kernels read."""
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous()


def reference(q, k, v, want_p=True):
    """float64, on the device of the inputs: ref = softmax(q k^T / 8) v, A = softmax(..) |v|, the probabilities."""
    q, k, v = q.double(), k.double(), v.double()
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return p @ v, p @ v.abs(), (p if want_p else None)


# ---- the bf16 kernels' error against the fp64 reference, derived ---------------------------------------------------------------
# Scores, their maximum and the row sum are f32.  P = exp(s - m) is rounded to bf16 by round-to-nearest-even (pack_bf16) before
# P.V: every probability moves by at most u p, u = 2^-8 being the unit roundoff of bf16's 8-bit significand (half the spacing
# 2^-7), so the output by at most u sum_t p_t |v_t| = u A.  The result is rounded the same way: u |ref| (its size up to the
# first term).  What is done in f32 — the score accumulation over 64 exact products (|s| of a few hundred at most: 2^-24 of
# that, / 8, is the relative error of a probability), v_exp_f32 (1 ulp), the row sum and the P.V accumulation over <= 288 terms
# (2^-24 each) — stays below 2^-16 A.
#
# Measured on an MI355X (256 CUs) against the fp64 reference — never against another run of a kernel —, the worst over every
# launch of tests/test_gpu_attention.py (tile edges, up to 1281 items of 288 tokens, ticket and stride).
# Worst |out - ref| / bf16_bound:          random  uniform  negative  match
#   k_attention32<7, 7>   (T <= 224)        0.857    0.437     0.694      0
#   k_attention<18, 8>    (T > 224)         0.717    0.437     0.555      0
# k_attention_split, worst max|out - ref| / its limit max(2 e32, 2^-20 max(1, max|ref|)) (e32: torch's f32 op against fp64):
#                            random            random_f32        uniform           negative          match
#   <14, 7>                  2.5e-6 / 4.4e-6   4.3e-6 / 6.1e-6   4.2e-8 / 9.5e-7   1.5e-6 / 4.0e-6   9.5e-7 / 7.8e-6
#   <18, 8>                  2.2e-6 / 4.2e-6   3.5e-6 / 6.1e-6   5.3e-9 / 9.5e-7   1.5e-6 / 4.1e-6   9.5e-7 / 8.0e-6
#   e32 of those launches: 2.1e-6 .. 4.9e-6 (random, random_f32, negative), 1.2e-8 (uniform), below 1e-13 (match).
def bf16_bound(ref, A):
    return 2.0 ** -8 * (A + ref.abs()) + 2.0 ** -16 * A


def emulate_bf16(q, k, v):
    """The arithmetic of k_attention / k_attention32 in torch: f32 scores, exp of the f32 difference to the row maximum, the
    row sum of the unrounded values, P rounded to bf16, an f32 product with V, the division, the result rounded to bf16."""
    s = q @ k.transpose(-1, -2)
    e = torch.exp((s - s.amax(-1, keepdim=True)) * 0.125)
    o = (_bf16(e) @ v) / e.sum(-1, keepdim=True)
    return _bf16(o)


# ---- mutated references: what a subtly wrong kernel would compute --------------------------------------------------------------
def drop_last_key(q, k, v):
    return reference(q, k[:, :, :-1], v[:, :, :-1])[0]


def leak_padded_key(q, k, v):
    """One zero key with a zero value enters the softmax with logit 0 (a padded LDS row that missed its -inf)."""
    z = torch.zeros_like(k[:, :, :1])
    return reference(q, torch.cat([k, z], 2), torch.cat([v, z], 2))[0]


def swap_items(x, a, b):
    """x (B, H, T, 64) with the (b, h) items a and b (flat indices) exchanged."""
    B, H = x.shape[:2]
    y = x.reshape(B * H, *x.shape[2:]).clone()
    y[[a, b]] = y[[b, a]]
    return y.view_as(x)


def rows_outside(got, ref, bound, factor=1.0):
    """bool per row (all but the last axis): some element of the row is further than factor * bound from ref."""
    return ((got - ref).abs() > factor * bound).any(-1)
