"""Inputs, fp64 references, a derived elementwise bound, a torch f32 model and mutated references for the bf16 row kernels of
csrc/encoder_ops.hip (k_add_layernorm, k_embed_layernorm, k_final_layernorm, k_bias_layernorm; entry points bsc_enc_add_layernorm,
_embed_layernorm, _final_layernorm, _bias_layernorm), shared by tests/test_layernorm_cases.py (CPU) and
tests/test_gpu_encoder_rows.py.  torch only, no GPU needed to import; every function works on the device of its inputs.

Every input is an f32 tensor whose values are bf16 numbers (bias_sum excepted: it is f32).  What the four kernels normalise,
as rows `v` of `width` values:
    add     s = bf16(x + delta), also written to xout bit for bit; without delta, x itself
    embed   row 0 of an image bf16(cls + pos[0]); rows 1..R the register tokens as they are; row r > R
            bf16(patch[b, r - 1 - R] + pos[r - R]); written to xout bit for bit
    final   s = bf16(x + delta) on rows [skip, T) of every image, the output dense
    bias    v = u + bias_sum, one f32 addition, nothing rounded to bf16; rows [skip, T) of every image
and y = bf16((v - mean) rstd gamma + beta), mean and the biased variance over the row, rstd = 1 / sqrt(var + eps).

The bound, elementwise:  |y - ref| <= 2^-8 |ref| + c 2^-24 (max_row|v| rstd |gamma| + |beta|),  c = 5 NG + 34,  NG = width / 256.
  2^-8 |ref| is the one rounding of the result to bf16 (8 significant bits, round to nearest even).  The rest is the f32 work, in
  units of u = 2^-24, m = max_row |v|:
    mean   a lane adds its 4 NG values in NG + 2 dependent additions, six butterfly steps follow, then the division by the width:
           every rounding is at most u times a partial sum of at most width m, so the mean is off by at most (NG + 9) u m;
    v      the bias kernel's u + bias_sum is rounded once: u m, which also moves the mean by at most u m more (2 in all; 0 for the
           other three kernels, whose v is exact);
    d      v - mean is rounded (u |d|, |d| <= 2 m) and carries the mean's error;
    rstd   every d^2 is off by 3 u relative, a lane's 4 NG additions and the six butterfly steps by u each, the division, the
           addition of eps and rsqrtf (1 ulp) by 4 u more: (4 NG + 13) u on var + eps, half of that on rstd, relative;
    y      d rstd, times gamma, plus beta: three more roundings, u each relative to at most |d| rstd |gamma| + |beta|.
  Together: u rstd |gamma| [ (NG + 11) m + 2 m (1 + (4 NG + 13) / 2 + 3) ] + u |beta| <= (5 NG + 34) u (m rstd |gamma| + |beta|).
  The error of the error (the bound evaluated with fp64 m and rstd) is of second order and inside the integer slack of c.

Measured on an MI355X against the fp64 reference, worst |y - ref| / bound over every width 256 .. 2048, row count and family of
tests/test_gpu_encoder_rows.py (the test prints the figure of every launch):
                        randn  mean30   tiny  const  gamma0
  k_add_layernorm       0.995   0.989  0.995      0   0.995
  k_embed_layernorm     0.993   0.985  0.994      0   0.995
  k_final_layernorm     0.993   0.984  0.994      0   0.994
  k_bias_layernorm      0.995   0.990  0.994      0   0.993
  (the rounding of the result to bf16 alone reaches 1 - 2^-8 where a value sits half way just above a power of two; const: the
  output is beta exactly.)  xout and the f32 form of the output were bit-exact everywhere.
"""
import torch

EPS = 1e-6
WIDTHS = tuple(range(256, 2049, 256))
FAMILIES = ("randn", "mean30", "tiny", "const", "gamma0")
ADD_ROWS = (1, 3, 4, 5, 1001)
EMBED_SHAPES = ((1, 2, 0), (2, 6, 4), (3, 17, 0), (2, 21, 4))                       # (B, T, R); T = 2 + R is the smallest accepted
FINAL_SHAPES = ((1, 2, 1), (3, 7, 5), (2, 17, 1), (1, 6, 1), (1, 7, 1))             # (B, T, skip)
BIAS_SHAPES = FINAL_SHAPES + ((5, 9, 0),)
BLN_RPW = 4                                                                         # rows per wavefront of k_bias_layernorm


def bf16(x):
    return x.bfloat16().float()


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def rows(family, n, width, gen, part=0):
    """(n, width) f32 of bf16 numbers, every row different.  `part` 0 is the stream (x, u, patch, cls, reg), 1 what is added to
    it (delta, pos): a tenth of the size, so that the sum keeps the family's character."""
    rn = torch.randn(n, width, generator=gen)
    if family in ("randn", "gamma0"):
        x = rn * (1.5 if part == 0 else 0.5)
    elif family == "mean30":
        x = rn + 30.0 if part == 0 else rn * 0.1
    elif family == "tiny":
        x = rn * (1e-3 if part == 0 else 1e-4)
    elif family == "const":         # multiples of 1 / 8 up to 8: every partial sum of a row is exact in f32, the variance is 0
        x = (torch.randint(-64, 65, (n, 1), generator=gen).float() / 8).expand(n, width)
        x = x + (torch.arange(n).view(n, 1) % 7).float() / 8 if part == 0 else x / 4
    else:
        raise ValueError(family)
    return bf16(x).contiguous()


def affine(family, width, gen):
    """gamma, beta (width,) f32 of bf16 numbers; gamma0: gamma within 1e-3 of zero (some exactly zero) in a quarter of the columns"""
    gamma = (0.5 + torch.rand(width, generator=gen)) * (torch.randint(0, 2, (width,), generator=gen) * 2 - 1)
    beta = torch.rand(width, generator=gen) - 0.5
    if family == "gamma0":
        q = torch.arange(width) % 4 == 1
        small = torch.randn(width, generator=gen) * 1e-3
        small[torch.arange(width) % 8 == 1] = 0.0
        gamma = torch.where(q, small, gamma)
    return bf16(gamma), bf16(beta)


def bias_vector(family, width, gen):
    """f32, NOT bf16 numbers (the sum of a stack's biases); const: 0.25 everywhere, so that u + bias_sum stays constant and exact"""
    if family == "const":
        return torch.full((width,), 0.25)
    scale = {"tiny": 1e-3, "mean30": 2.0}.get(family, 2.0)
    return (torch.randn(width, generator=gen) * scale).contiguous()


def make(op, family, shape, width, seed, device="cpu"):
    """The inputs of one launch as a dict of tensors on `device`.  shape: rows (add) or (B, T, R | skip)."""
    gen = torch.Generator().manual_seed(seed)
    z = {}
    z["gamma"], z["beta"] = affine(family, width, gen)
    if op == "add":
        z["x"], z["delta"] = rows(family, shape, width, gen), rows(family, shape, width, gen, 1)
    elif op == "embed":
        B, T, R = shape
        z["patch"] = rows(family, B * (T - 1 - R), width, gen)
        z["cls"] = rows(family, 1, width, gen)[0]
        z["reg"] = rows(family, max(R, 1), width, gen)
        z["pos"] = rows(family, T - R, width, gen, 1)
    elif op == "final":
        B, T, skip = shape
        z["x"], z["delta"] = rows(family, B * T, width, gen), rows(family, B * T, width, gen, 1)
    elif op == "bias":
        B, T, skip = shape
        z["u"], z["bias_sum"] = rows(family, B * T, width, gen), bias_vector(family, width, gen)
    else:
        raise ValueError(op)
    return {k: v.to(device) for k, v in z.items()}


# ---- the rows a kernel normalises (exact: f32 holds them), with the mutants as keyword arguments ---------------------------------
def picked(B, T, skip, device, row_off=0):
    """input row of every output row: rows [skip, T) of every image; row_off = 1 is the mutant that starts one row late"""
    b = torch.arange(B, device=device).view(B, 1)
    r = torch.arange(skip, T, device=device).view(1, T - skip)
    return (b * T + r + row_off).clamp_max(B * T - 1).reshape(-1)


def rows_add(z, with_delta=True):
    return bf16(z["x"] + z["delta"]) if with_delta else z["x"]


def rows_embed(z, shape, pos_on_registers=False, pos_by_row=False):
    B, T, R = shape
    np_, width = T - 1 - R, z["cls"].shape[0]
    pos, patch = z["pos"], z["patch"].view(B, np_, width)
    out = torch.empty((B, T, width), dtype=torch.float32, device=patch.device)
    out[:, 0] = bf16(z["cls"] + pos[0])
    # a mutant's read past the table's T - R rows finds other data: the table again, its columns rolled
    far = torch.cat([pos, pos.roll(7, 1).repeat(R, 1)[:R]])
    if R and pos_on_registers:      # pos[r] added to register row r
        out[:, 1:1 + R] = bf16(z["reg"][:R] + far[1:1 + R])
    elif R:
        out[:, 1:1 + R] = z["reg"][:R]
    if pos_by_row:          # pos[r] instead of pos[r - R]: the table read R rows further down
        out[:, 1 + R:] = bf16(patch + far[1 + R:T])
    else:
        out[:, 1 + R:] = bf16(patch + pos[1:])
    return out.view(B * T, width)


def rows_final(z, shape, row_off=0):
    B, T, skip = shape
    idx = picked(B, T, skip, z["x"].device, row_off)
    return bf16(z["x"][idx] + z["delta"][idx])


def rows_bias(z, shape, row_off=0, round_bias=False, dtype=torch.float64):
    """u + bias_sum: in fp64 for the reference (exact), in f32 for the model (the kernel's one rounding)"""
    B, T, skip = shape
    idx = picked(B, T, skip, z["u"].device, row_off)
    bs = bf16(z["bias_sum"]) if round_bias else z["bias_sum"]
    return z["u"][idx].to(dtype) + bs.to(dtype)


# ---- reference, bound, model ---------------------------------------------------------------------------------------------------
def layernorm64(v, gamma, beta, eps=EPS, ddof=0, group_shift=0):
    """fp64 LayerNorm of rows v -> ref, bound (both (rows, width) fp64).  eps, ddof (variance over width - ddof) and group_shift
    (gamma and beta read so many groups of four columns to the right, wrapping) are the mutants."""
    v, gamma, beta = v.double(), gamma.double(), beta.double()
    width = v.shape[-1]
    if group_shift:
        gamma, beta = gamma.roll(-4 * group_shift), beta.roll(-4 * group_shift)
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).sum(-1, keepdim=True) / (width - ddof)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = (v - mean) * rstd * gamma + beta
    c = 5 * (width // 256) + 34
    bound = 2.0 ** -8 * ref.abs() + c * 2.0 ** -24 * (v.abs().amax(-1, keepdim=True) * rstd * gamma.abs() + beta.abs())
    return ref, bound


def model32(v, gamma, beta, order="kernel", eps=EPS):
    """The kernels' arithmetic in torch f32 on rows v (f32) -> y (f32 of bf16 numbers).  order "kernel": a lane holds columns
    4 (lane + 64 g) + k, adds (v0 + v1) + (v2 + v3) per group g in turn, then the xor butterfly 32, 16, .. 1; "torch": torch.sum."""
    n, width = v.shape
    ng = width // 256
    v = v.float()

    def total(t):           # t (n, width) -> (n, 1)
        if order == "torch":
            return t.sum(-1, keepdim=True)
        q = t.view(n, ng, 64, 4)
        lane = torch.zeros((n, 64), dtype=torch.float32, device=t.device)
        for g in range(ng):
            lane = lane + ((q[:, g, :, 0] + q[:, g, :, 1]) + (q[:, g, :, 2] + q[:, g, :, 3]))
        ar = torch.arange(64, device=t.device)
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, ar ^ o]
        return lane[:, :1]

    def total_sq(d):        # the variance adds its squares one by one
        if order == "torch":
            return (d * d).sum(-1, keepdim=True)
        q = (d * d).view(n, ng, 64, 4)
        lane = torch.zeros((n, 64), dtype=torch.float32, device=d.device)
        for g in range(ng):
            for k in range(4):
                lane = lane + q[:, g, :, k]
        ar = torch.arange(64, device=d.device)
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, ar ^ o]
        return lane[:, :1]

    mean = total(v) / float(width)
    d = v - mean
    rstd = torch.rsqrt(total_sq(d) / float(width) + eps)
    return bf16(d * rstd * gamma.float() + beta.float())


def repeat_in_groups(y):
    """The mutant of BLN_RPW's clamp leaking into the store: in every group of four output rows, the last row present (when the
    group has more than one) holds a copy of the row before it."""
    y = y.clone()
    n = y.shape[0]
    for first in range(0, n, BLN_RPW):
        last = min(first + BLN_RPW, n) - 1
        if last > first:
            y[last] = y[last - 1]
    return y


def worst_ratio(got, ref, bound):
    return ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


def outside(got, ref, bound):
    """bool per row: some element further from ref than the bound"""
    return ((got.double() - ref).abs() > bound).any(-1)
