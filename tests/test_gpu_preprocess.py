"""The fused preprocessing kernels (csrc/encoder_ops.hip: k_preprocess_patches, k_pp_taps, k_preprocess_patches_tiled<8 | 12>)
through bsc_enc_preprocess_patches_typed against the fp64 reference of tests/preprocess_cases.py, on its ladder of frame sizes:
up-sampling, the identity and its neighbours, the workload's ratios, factor 3.0 where the tiled kernel goes from 8 to 12 column
taps, the last tiled and the first generic size of both window limits, 4.5, 5.5 (12 taps), and the refusal above that.

f32 output (mode 1), RGB and RGBA: max |out - ref| <= max(2 e32, 2e-6), e32 the distance of PyTorch's own f32 evaluation of the
same frames on the GPU from fp64 (the yardstick of tests/test_gpu_encoder_f32.py).  The other forms are functions of the f32
value and are held bit for bit: RGB == RGBA, mode 0 == RNE bf16, mode 2 == (fp16(v), fp16(v - h)) in [32 h | 32 l] chunks with zero
pad columns.  64 sentinel rows before and after every output stay untouched; rejected arguments write nothing."""
import ctypes as C
import functools

import pytest

import preprocess_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5A
BSC_E_INVALID = -1
ENTRIES = [(S, p, H, W) for S, p in PC.CONFIGS for H, W in PC.ladder(S, p)]
IDS = [f"S{S}-{H}x{W}" for S, p, H, W in ENTRIES]


def row_shorts(p, mode):
    """int16 words per output row"""
    K = 3 * p * p
    return {0: K, 1: 2 * K, 2: 2 * ((K + 31) // 32 * 32)}[mode]


def launch(img, S, p, mode, Cc=None, H=None, W=None, rgb_null=False, out_null=False, mean_null=False, std_null=False):
    """One call into an output with GUARD sentinel rows on either side -> status, the whole buffer (int16, guards included)."""
    import torch
    from bsc_nav_amd import _lib
    B = img.shape[0]
    H = img.shape[1] if H is None else H
    W = img.shape[2] if W is None else W
    Cc = img.shape[3] if Cc is None else Cc
    g = max(S // p, 1)
    buf = torch.full((B * g * g + 2 * GUARD, row_shorts(p, min(max(mode, 0), 2))), SENTINEL, dtype=torch.int16, device="cuda")
    mean, std = (C.c_float * 3)(*PC.MEAN), (C.c_float * 3)(*PC.STD)
    st = _lib.load().bsc_enc_preprocess_patches_typed(
        None if rgb_null else C.c_void_p(img.data_ptr()), B, H, W, Cc, S, p, None if out_null else C.c_void_p(buf[GUARD:].data_ptr()),
        mode, None if mean_null else mean, None if std_null else std, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, buf


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def body(buf, B, g):
    return buf[GUARD:-GUARD].reshape(B, g * g, -1)


@functools.lru_cache(maxsize=8)
def case(family, S, p, H, W):
    """Frames on the GPU, the fp64 reference and the limit, computed once."""
    img4 = PC.frames(family, H, W, seed=H * 1000 + W + S, device="cuda")
    ref = PC.reference(img4, S, p)
    e32, limit = PC.limit_of(img4, S, p, ref)
    return img4, img4[..., :3].contiguous(), ref, e32, limit


@pytest.mark.parametrize("S,p,H,W", ENTRIES, ids=IDS)
def test_every_output_form_against_fp64(S, p, H, W):
    import torch
    g, B = S // p, PC.BATCH
    K = 3 * p * p
    for family in PC.FAMILIES:
        img4, img3, ref, e32, limit = case(family, S, p, H, W)
        f32 = {}
        for img in (img3, img4):
            Cc = img.shape[3]
            kernel = PC.kernel_of(H, W, S, p, Cc)
            outs = {}
            for mode in (1, 0, 2):
                st, buf = launch(img, S, p, mode)
                assert st == 0 and guards_intact(buf), (family, Cc, mode, st)
                outs[mode] = body(buf, B, g)
            v = outs[1].contiguous().view(torch.float32)
            err = (v.double() - ref).abs().max().item()
            pieces = outs[2].contiguous().view(torch.float16).view(B, g * g, -1, 2, 32).double().sum(3).reshape(B, g * g, -1)
            print(f"preprocess S={S} {H}x{W} C={Cc} {kernel} {family}: mode 1 {err:.3e} / limit {limit:.3e} = {err / limit:.3f}"
                  f" (e32 {e32:.3e}); mode 0 {(outs[0].view(torch.bfloat16).double() - ref).abs().max().item():.3e};"
                  f" mode 2 {(pieces[..., :K] - ref).abs().max().item():.3e}")
            assert err <= limit, (family, Cc, kernel, err, limit)
            assert torch.equal(outs[0], PC.bf16_bits(v)), (family, Cc, "mode 0 is not the RNE bf16 of mode 1")
            assert torch.equal(outs[2], PC.pieces_bits(v, p)), (family, Cc, "mode 2 is not (fp16(v), fp16(v - h)), zero pads")
            f32[Cc] = v
        assert torch.equal(f32[3], f32[4]), (family, "RGB and RGBA differ")


@pytest.mark.parametrize("S,p", PC.CONFIGS)
def test_rejected_arguments_write_nothing(S, p):
    import torch
    img = PC.frames("random", 80, 90, seed=5, device="cuda")
    g = S // p
    bad = [dict(frame=PC.frames("random", h, w, seed=7, device="cuda")) for h, w in PC.rejected_sizes(S)]     # a factor above 5.5
    bad += [dict(S=S + 1), dict(Cc=2), dict(mode=3), dict(mode=-1),
            dict(rgb_null=True), dict(out_null=True), dict(mean_null=True), dict(std_null=True)]
    for kw in bad:
        for Cc in (3, 4):
            for mode in (0, 1, 2):
                a = dict(Cc=Cc, mode=mode, S=S, frame=img)
                a.update(kw)
                S_, frame = a.pop("S"), a.pop("frame")
                if a["Cc"] == 3:
                    frame = frame[..., :3].contiguous()
                st, buf = launch(frame, S_, p, a.pop("mode"), **a)
                assert st == BSC_E_INVALID, (kw, Cc, mode, st)
                assert bool((buf == SENTINEL).all()), (kw, Cc, mode)
    # pieces need whole 32-column chunks per channel plane: patch^2 >= 32
    for small in (4, 5):
        st, buf = launch(img, 40, small, 2)
        assert st == BSC_E_INVALID and bool((buf == SENTINEL).all())
        st, buf = launch(img, 40, small, 1)
        assert st == 0 and guards_intact(buf)
        v = body(buf, PC.BATCH, 40 // small).contiguous().view(torch.float32)
        ref = PC.reference(img, 40, small)
        assert (v.double() - ref).abs().max().item() <= PC.limit_of(img, 40, small, ref)[1]
    # the largest supported factor itself is served
    top = PC.largest_supported(S)
    big = PC.frames("random", top, top, seed=6, device="cuda")
    assert launch(big, S, p, 1)[0] == 0
