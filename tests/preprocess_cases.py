"""Frames, an fp64 reference, the limit and mutated references for the fused preprocessing kernels of csrc/encoder_ops.hip
(k_preprocess_patches, k_pp_taps, k_preprocess_patches_tiled<8 | 12>; entry point bsc_enc_preprocess_patches_typed), shared by
tests/test_preprocess_cases.py (CPU: the reference equals PyTorch's fp64 resize, every mutant leaves the limit) and
tests/test_gpu_preprocess.py.  torch only, no GPU needed to import; every function works on the device of its inputs.

The operation: u8 frames (B, H, W, C >= 3) -> / 255 -> antialiased bilinear resize to (S, S) -> (x - mean) / std -> unfolded
patch matrix (B, g^2, 3 p^2), columns in (channel, py, px) order, g = S / p.  The reference builds dense fp64 weight matrices
Wy (S x H), Wx (S x W) from the filter rule alone — scale = in / out, support = max(scale, 1), centre c = scale (o + 1/2), taps
[int(c - support + 1/2) clipped at 0, int(c + support + 1/2) clipped at in), weights max(0, 1 - |i + 1/2 - c| / max(scale, 1))
normalised to sum 1 — and evaluates Wy (img / 255) Wx^T.

The ladder of frame sizes is derived from the kernel's documented limits, not copied from its code paths:
    factor <= (PP_TAPS - 1) / 2 = 5.5 on either axis, above that the entry point refuses;
    RGBA frames take the tiled kernel when p f + 2 support + 3 <= PPT_MAXH (48) vertically and <= PPT_MAXW (64) horizontally,
    every other frame the generic kernel; the tiled kernel evaluates 8 column taps up to a horizontal factor of 3.0, 12 above.

The limit of the f32 output (mode 1) is that of tests/test_gpu_encoder_f32.py: max |out - ref| <= max(2 e32, 2e-6), e32 the
distance of PyTorch's own f32 evaluation (/ 255, F.interpolate(bilinear, antialias), normalise) of the same frames, on the same
device, from the fp64 reference.  S = 64 makes every scale, centre and tap bound exact in f32 (multiples of 1 / 128); S = 56 does
not, there the f32 rounding of the tap centre is part of e32 and of the kernel's error alike.

Measured on an MI355X against the fp64 reference, the worst over every ladder entry and family (tests/test_gpu_preprocess.py
prints the figure of every case):
Worst max|out - ref| / limit, mode 1 (f32):          random  impulse  stripes  ramp
  k_preprocess_patches (RGB; RGBA past the window)    0.643    0.525    0.599   0.758
  k_preprocess_patches_tiled<8>                       0.593    0.512    0.571   0.758
  k_preprocess_patches_tiled<12>                      0.520    0.525    0.517   0.742
  either side of the 8 -> 12 tap switch, RGBA (tiled):
    factor 3.0, tiled<8>   128 x 192 (S = 64)         0.593    0.097    0.348   0.687
                           112 x 168 (S = 56)         0.508    0.097    0.348   0.758
    one above, tiled<12>   128 x 193 (S = 64)         0.433    0.084    0.376   0.534
                           112 x 169 (S = 56)         0.520    0.500    0.476   0.742
  e32 of those launches: 1.4e-7 .. 1.7e-6 at S = 64, up to 1.9e-5 at S = 56 (57 x 55 stripes: PyTorch's f32 tap centres);
  the kernels' own largest error 1.8e-6 at S = 64 and 1.9e-5 at S = 56, on that same case (0.51 of its limit).  Modes 0 and 2
  are bit for bit functions of the mode 1 value; against fp64 they were at most 7.9e-3 (one bf16 rounding of |v| <= 2.64) and
  1.9e-5 (the two fp16 pieces add 2^-22 |v|).
"""
from fractions import Fraction

import torch
import torch.nn.functional as F

PP_TAPS = 12                    # taps per axis the kernels hold: factor <= (PP_TAPS - 1) / 2
PPT_MAXH, PPT_MAXW = 48, 64     # LDS window of the tiled kernel, rows x columns
MAX_FACTOR = Fraction(PP_TAPS - 1, 2)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FLOOR = 2e-6
FAMILIES = ("random", "impulse", "stripes", "ramp")
BATCH = 2


# ---- the ladder ---------------------------------------------------------------------------------------------------------------
def fits_window(n_in, S, p, limit):
    """p f + 2 support + 3 <= limit, in exact arithmetic (f = n_in / S)."""
    f = Fraction(n_in, S)
    return p * f + 2 * max(f, Fraction(1)) + 3 <= limit


def last_tiled(S, p, limit):
    """The largest input size of an axis that the tiled kernel's window still holds."""
    n = 1
    while fits_window(n + 1, S, p, limit):
        n += 1
    return n


def largest_supported(S):
    """The largest input size whose factor is at most (PP_TAPS - 1) / 2."""
    return int(MAX_FACTOR * S)


def kernel_of(H, W, S, p, C):
    """Which kernel the documented limits give a frame: "generic", "tiled8" or "tiled12"."""
    if C != 4 or p * p > 256 or not fits_window(H, S, p, PPT_MAXH) or not fits_window(W, S, p, PPT_MAXW):
        return "generic"
    return "tiled8" if Fraction(W, S) <= 3 else "tiled12"


def ladder(S, p):
    """(H, W) pairs for one of CONFIGS: up-sampling, around the identity, exact 2.0, the workload's ratios, 3.0 and the
    next size up (both inside the tiled kernel's window: its 8 and its 12 column taps), the last tiled / first generic size of
    both limits, the tiled 12-tap kernel, 4.5, 5.5; factors mixed."""
    r = lambda num: int(round(Fraction(num, 224) * S))          # a workload size at S = 224, scaled to S
    up = int(round(Fraction(27, 64) * S))
    th, tw = last_tiled(S, p, PPT_MAXH), last_tiled(S, p, PPT_MAXW)
    top = largest_supported(S)
    out = [(up, up), (S - 1, S), (S, S), (S + 1, S - 1), (2 * S, 2 * S), (r(480), r(640)), (r(680), r(680)),
           (3 * S, 3 * S), (2 * S, 3 * S), (2 * S, 3 * S + 1), (th, tw), (th + 1, tw), (th, tw + 1), (S + S // 2 + 4, tw),
           (9 * S // 2, 9 * S // 2), (top, top)]
    if S == 64:         # further mixes of the factors, once
        out += [(3 * S + 1, 3 * S), (9 * S // 2, r(480)), (up, top), (S, top), (top, up + 13)]
    assert len(set(out)) == len(out) and all(max(h, w) <= 352 for h, w in out)
    return out


def rejected_sizes(S):
    """One size above the largest supported factor, on either axis."""
    top = largest_supported(S)
    return [(top + 1, S), (S, top + 1)]


CONFIGS = ((64, 16), (56, 14))          # (S, p), both g = 4


# ---- frames -------------------------------------------------------------------------------------------------------------------
def frames(family, H, W, seed, device="cpu"):
    """(BATCH, H, W, 4) u8, different data per image; the alpha channel is random (the kernels must ignore it)."""
    g = torch.Generator().manual_seed(seed)
    B = BATCH
    img = torch.zeros((B, H, W, 3), dtype=torch.int64)
    if family == "random":
        img = torch.randint(0, 256, (B, H, W, 3), generator=g)
    elif family == "impulse":
        # corners, edge mid-points, one interior point; image 1 lights one channel per point and moves the interior point
        pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
        for b in range(B):
            for i, (y, x) in enumerate(pts + [(H // 3 + b, (2 * W) // 3 - b)]):
                if b == 0:
                    img[b, y, x, :] = 255
                else:
                    img[b, y, x, i % 3] = 255
    elif family == "stripes":
        yy = torch.arange(H).view(H, 1, 1)
        xx = torch.arange(W).view(1, W, 1)
        img[0] = ((xx % 2) * 255).expand(H, W, 3)                       # period-2 columns
        img[1] = ((yy % 2) * 255).expand(H, W, 3)                       # period-2 rows
        img[1, :, :, 1] = 255 - img[1, :, :, 1]
    elif family == "ramp":
        yy = torch.arange(H, dtype=torch.float64).view(H, 1) / max(H - 1, 1)
        xx = torch.arange(W, dtype=torch.float64).view(1, W) / max(W - 1, 1)
        for b in range(B):
            for c, (sy, sx) in enumerate(((200, 40), (30, 180), (110, 110))):
                v = sy * yy + sx * xx + 5 * c
                img[b, :, :, c] = (v if b == 0 else 250 - v).round().long()
    else:
        raise ValueError(family)
    alpha = torch.randint(0, 256, (B, H, W, 1), generator=g)
    return torch.cat([img, alpha], -1).to(torch.uint8).to(device)


# ---- the fp64 reference and its mutants -----------------------------------------------------------------------------------------
def weights(n_in, n_out, device="cpu", scale=None, shift=0, renorm=True, antialias=True, max_taps=None, half=0.5):
    """Dense (n_out, n_in) fp64 resize matrix from the filter rule.  The keyword arguments are the mutants: `scale` another
    axis' factor, `shift` the taps read `shift` pixels further right, `renorm=False` taps clipped at the border keep the weight
    they have in the unclipped window, `antialias=False` support 1 when down-sampling, `max_taps` at most so many taps,
    `half` the centre offset."""
    scale = n_in / n_out if scale is None else scale
    support = scale if (scale >= 1.0 and antialias) else 1.0
    o = torch.arange(n_out, dtype=torch.float64, device=device).view(-1, 1)
    pad = 16                                                                # room for the unclipped window
    i = torch.arange(-pad, n_in + pad, dtype=torch.float64, device=device).view(1, -1)
    c = scale * (o + half)
    lo, hi = torch.trunc(c - support + 0.5).clamp_min(0), torch.trunc(c + support + 0.5).clamp_max(n_in)
    if max_taps is not None:
        hi = torch.minimum(hi, lo + max_taps)
    tri = (1.0 - (i + 0.5 - c).abs() / support).clamp_min(0)
    w = tri * ((i >= lo) & (i < hi))
    if renorm:
        w = w / w.sum(1, keepdim=True)
    else:
        w = w / tri.sum(1, keepdim=True)            # the whole triangle, the part outside the frame included
    w = torch.nan_to_num(w[:, pad:pad + n_in])      # an empty window (a mutant's only) weighs nothing
    if shift:
        moved = torch.zeros_like(w)
        moved[:, shift:] = w[:, :-shift]
        moved[:, -1] += w[:, -shift:].sum(1)                                # clamped at the border
        w = moved
    return w


def unfold(x, p, order="cyx"):
    """(B, 3, S, S) -> (B, g^2, 3 p^2), columns (channel, py, px); order "yxc" is the mutant (py, px, channel)."""
    B, _, S, _ = x.shape
    g = S // p
    x = x.reshape(B, 3, g, p, g, p)
    x = x.permute(0, 2, 4, 1, 3, 5) if order == "cyx" else x.permute(0, 2, 4, 3, 5, 1)
    return x.reshape(B, g * g, 3 * p * p)


def reference(img, S, p, swap_hw=False, channels=(0, 1, 2), order="cyx", **mut):
    """fp64 patch matrix of u8 frames (B, H, W, >= 3), on their device.  swap_hw, channels, order and **mut (see weights) give
    the mutated references."""
    B, H, W, _ = img.shape
    dev = img.device
    sy, sx = (W / S, H / S) if swap_hw else (None, None)
    wy = weights(H, S, dev, scale=sy, **mut)
    wx = weights(W, S, dev, scale=sx, **mut)
    x = img[..., list(channels)].permute(0, 3, 1, 2).double() / 255.0
    x = wy @ x @ wx.t()
    mean = torch.tensor(MEAN, dtype=torch.float64, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64, device=dev).view(1, 3, 1, 1)
    return unfold((x - mean) / std, p, order)


def torch_resize(img, S, p, dtype):
    """PyTorch's own evaluation in `dtype` (the project's RandomViT.preprocess, then the unfold): f32 gives e32, f64 is what the
    reference must equal."""
    x = img[..., :3].permute(0, 3, 1, 2).to(dtype) / 255
    if x.shape[-2:] != (S, S):
        x = F.interpolate(x, size=(S, S), mode="bilinear", antialias=True, align_corners=False)
    mean = torch.tensor(MEAN, dtype=dtype, device=img.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=img.device).view(1, 3, 1, 1)
    return unfold((x - mean) / std, p)


def limit_of(img, S, p, ref):
    """-> e32, max(2 e32, FLOOR) for these frames on their device."""
    e32 = (torch_resize(img, S, p, torch.float32).double() - ref).abs().max().item()
    return e32, max(2.0 * e32, FLOOR)


def model_f32(img, S, p):
    """The kernels' arithmetic in torch f32: scale, centre, tap bounds and weights in f32 as aa_taps has them (at most PP_TAPS
    taps, normalised by a multiplication with 1 / total), f32 row sums then column sums, * (1 / 255), - mean, / std.  The order
    of the additions inside a sum is torch's, not the kernels'."""
    B, H, W, _ = img.shape
    f32 = torch.float32

    def taps(n_in):
        scale = torch.tensor(n_in, dtype=f32) / torch.tensor(S, dtype=f32)
        support = scale if scale >= 1 else torch.ones((), dtype=f32)
        inv = 1 / scale if scale >= 1 else torch.ones((), dtype=f32)
        o = torch.arange(S, dtype=f32).view(-1, 1)
        c = scale * (o + 0.5)
        lo = torch.trunc(c - support + 0.5).clamp_min(0)
        hi = torch.minimum(torch.trunc(c + support + 0.5).clamp_max(n_in), lo + PP_TAPS)
        i = torch.arange(n_in, dtype=f32).view(1, -1)
        w = (1 - ((i - c + 0.5) * inv).abs()).clamp_min(0) * ((i >= lo) & (i < hi))
        return w * (1 / w.sum(1, keepdim=True))

    x = img[..., :3].permute(0, 3, 1, 2).to(f32)
    x = taps(H) @ (x @ taps(W).t())
    mean = torch.tensor(MEAN, dtype=f32).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=f32).view(1, 3, 1, 1)
    return unfold((x * torch.tensor(1 / 255, dtype=f32) - mean) / std, p)


# ---- the other output forms, from the f32 one ------------------------------------------------------------------------------------
def bf16_bits(v):
    """round-to-nearest-even bf16 of an f32 tensor, as int16 bits"""
    return v.bfloat16().view(torch.int16)


def pieces_bits(v, p):
    """(B, rows, 3 p^2) f32 -> (B, rows, 2 Kp) int16: h = fp16(v), l = fp16(v - h), [32 h | 32 l] per 32-column chunk, the columns
    padded with zeros to Kp, the next multiple of 32."""
    B, rows, K = v.shape
    Kp = (K + 31) // 32 * 32
    vp = torch.zeros((B, rows, Kp), dtype=torch.float32, device=v.device)
    vp[..., :K] = v
    h = vp.half()
    l = (vp - h.float()).half()
    return torch.stack([h.view(B, rows, Kp // 32, 32), l.view(B, rows, Kp // 32, 32)], 3).reshape(B, rows, 2 * Kp).view(torch.int16)
