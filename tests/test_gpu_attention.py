"""The in-tree attention kernels (csrc/encoder_ops.hip: k_attention32, k_attention; csrc/encoder_gemm.hip: k_attention_split)
against an fp64 reference on the generated cases of tests/attention_cases.py: every key-tile and mask edge, launches that
give a workgroup a second and later (image, head) item — with the ticket pair and with the static stride —, the ticket
pair's re-arming, guard rows around the output and rejected arguments.

bf16 kernels: |out - ref| <= bf16_bound elementwise (attention_cases.bf16_bound, derived from the kernels' arithmetic).
split kernel: max|out - ref| <= max(2 e32, 2^-20 max(1, max|ref|)), e32 the error of PyTorch's own f32
scaled_dot_product_attention against fp64 (the yardstick of tests/test_gpu_encoder_f32.py); the floor is what two fp16
pieces hold (22 bits) with a factor of two."""
import ctypes as C
import functools
import zlib

import pytest

import attention_cases as AC

pytestmark = pytest.mark.gpu

GUARD = 64                  # sentinel rows before and after every output
SENTINEL = 0x5A5A
EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 160, 161, 191, 192, 193, 208, 209, 223, 224,
         225, 239, 240, 241, 255, 256, 257, 271, 272, 273, 287, 288]
COUNTS = ["n_cu-1", "n_cu", "n_cu+1", "2n_cu+3", "5n_cu+1"]


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def items_of(count):
    """(B, H) for a named item count: H = 1 hits the count exactly (fewer than, exactly, ... one item per workgroup), H = 3
    takes the smallest B that reaches or passes it."""
    n = n_cu()
    want, H = {"n_cu-1": (n - 1, 1), "n_cu": (n, 1), "n_cu+1": (n + 1, 3), "2n_cu+3": (2 * n + 3, 3), "5n_cu+1": (5 * n + 1, 3)}[count]
    return (want + H - 1) // H, H


@functools.lru_cache(maxsize=6)
def case(family, B, T, H):
    """Inputs on the GPU, the fp64 reference and both criteria's limits, computed once and shared."""
    import torch
    import torch.nn.functional as F
    seed = zlib.crc32(f"{family} {B} {T} {H}".encode())
    q, k, v = (x.cuda() for x in AC.make(family, B, T, H, seed))
    ref, A, _ = AC.reference(q, k, v, want_p=False)
    z = dict(q=q, k=k, v=v, qkv=AC.pack(q, k, v), ref=ref, bound=AC.bf16_bound(ref, A))
    ref32 = F.scaled_dot_product_attention(q, k, v)
    e32 = (ref32.double() - ref).abs().max().item()
    if family in ("random", "random_f32"):
        z["ref32"] = ref32
    z["e32"], z["limit"] = e32, max(2.0 * e32, 2.0 ** -20 * max(1.0, ref.abs().max().item()))
    if family == "match":
        perm = AC.match_perm(B, T, H, seed).cuda()
        z["want"] = torch.gather(v, 2, perm.unsqueeze(-1).expand_as(v))
    return z


def launch(kernel, qkv, B, T, H, work, head_dim=64, entry=None):
    """One launch into an output with GUARD sentinel rows on either side.  qkv: (B, T, 3, H, 64) f32 on the GPU; work: an int32
    pair on the GPU or None (the static stride).  -> status, the whole buffer as int16 (guards included)."""
    import torch
    from bsc_nav_amd import _lib, encoder
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wp = C.c_void_p(work.data_ptr()) if work is not None else None
    rows = B * min(T, 288)
    if kernel == "bf16":
        x = qkv.bfloat16()
        buf = torch.full((rows + 2 * GUARD, H * 64), SENTINEL, dtype=torch.int16, device="cuda")
        op = C.c_void_p(buf[GUARD:].data_ptr())
        if entry == "static":
            st = L.bsc_enc_attention(C.c_void_p(x.data_ptr()), B, T, H, head_dim, op, stream)
        else:
            st = L.bsc_enc_attention_dyn(C.c_void_p(x.data_ptr()), B, T, H, head_dim, op, wp, stream)
    else:
        x = encoder.split_rows(qkv.view(B * T, 3 * H * 64), 1.0)
        buf = torch.full((rows + 2 * GUARD, 2 * H * 64), SENTINEL, dtype=torch.int16, device="cuda")
        st = L.bsc_enc_attention_split(C.c_void_p(x.data_ptr()), B, T, H, head_dim, C.c_void_p(buf[GUARD:].data_ptr()), 16.0, wp, stream)
    torch.cuda.synchronize()
    return st, buf


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def decode(kernel, body, B, T, H):
    """The output rows (int16 bits) -> (B, H, T, 64): f32 of the bf16 values / f64 of h + l over out_scale."""
    import torch
    if kernel == "bf16":
        return body.view(torch.bfloat16).float().view(B, T, H, 64).permute(0, 2, 1, 3)
    p = body.view(torch.float16).view(B * T, H * 2, 2, 32)
    return ((p[:, :, 0].double() + p[:, :, 1].double()) / 16.0).reshape(B, T, H, 64).permute(0, 2, 1, 3)


def item_bits(kernel, body, B, T, H, item):
    b, h = divmod(item, H)
    w = body.shape[1] // H
    return body.view(B, T, H * w)[b, :, h * w:(h + 1) * w]


def check(kernel, B, T, H, family, work, samples=(), label=""):
    """The one checking function: launch, guard rows, the ticket pair back at [0, 0], the kernel's criterion against the fp64
    reference, and `samples` — items recomputed alone (B = 1, H = 1), bit for bit equal to their slice of this launch.
    -> the output rows as int16 bits."""
    import torch
    z = case(family, B, T, H)
    st, buf = launch(kernel, z["qkv"], B, T, H, work)
    assert st == 0, st
    assert guards_intact(buf), "rows outside the output were written"
    if work is not None:
        assert work.tolist() == [0, 0], f"ticket pair left at {work.tolist()}"
    body = buf[GUARD:-GUARD]
    out = decode(kernel, body, B, T, H)
    assert torch.isfinite(out).all()
    err = (out.double() - z["ref"]).abs()
    how = "ticket" if work is not None else "stride"
    if kernel == "bf16":
        ratio = (err / z["bound"].clamp_min(1e-300)).max().item()
        print(f"ATT bf16 {family} B={B} T={T} H={H} {how} {label} ratio={ratio:.4f}")
        assert ratio <= 1.0, (ratio, family, B, T, H)
        if family == "match":
            assert torch.equal(out.bfloat16(), z["want"].bfloat16())
    else:
        worst = err.max().item()
        print(f"ATT split {family} B={B} T={T} H={H} {how} {label} err={worst:.3e} limit={z['limit']:.3e} e32={z['e32']:.3e}")
        assert worst <= z["limit"], (worst, z["limit"], z["e32"], family, B, T, H)
        if "ref32" in z:                                            # random inputs: within 1e-5 of the f32 op itself as well
            assert (out - z["ref32"].double()).abs().max().item() <= 1e-5
    for item in samples:
        b, h = divmod(item, H)
        st, one = launch(kernel, z["qkv"][b:b + 1, :, :, h:h + 1].contiguous(), 1, T, 1, None)
        assert st == 0 and guards_intact(one)
        assert torch.equal(one[GUARD:-GUARD], item_bits(kernel, body, B, T, H, item)), f"item {item} differs from the same item computed alone"
    return body


def families_of(kernel):
    return AC.FAMILIES + (("random_f32",) if kernel == "split" else ())


# ---- tile and mask edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", EDGES)
@pytest.mark.parametrize("kernel", ["bf16", "split"])          # (the last decorator varies fastest: both kernels share a case)
def test_tile_and_mask_edges(kernel, T):
    """Every length at which a key tile ends or the -inf mask changes form (16 (NT - 2): 192 | 193, 256 | 257; 32-key tiles:
    160 | 161), and the shortest and longest lengths, one launch each."""
    import torch
    work = torch.zeros(2, dtype=torch.int32, device="cuda")
    for family in families_of(kernel):
        check(kernel, 1, T, 2, family, work)


# ---- second and later items -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [17, 193, 288])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("family", ["random", "negative"])
@pytest.mark.parametrize("kernel", ["bf16", "split"])
def test_second_and_later_items(kernel, T, count, family):
    """Fewer items than workgroups, as many, one more, and up to six per workgroup: the loop past its first pass, the ticket
    fetch, the LDS barrier between items, the prefetch that re-reads the last item; the same launch with the ticket pair and
    with the static stride.  The kernels are deterministic: an item that differs from itself computed alone took state from
    another item."""
    import torch
    B, H = items_of(count)
    n, items = n_cu(), B * H
    samples = sorted({i for i in (0, 1, n - 2, n - 1, n, n + 1, items // 2, 2 * n, 3 * n + 1, items - 2, items - 1) if 0 <= i < items})
    work = torch.zeros(2, dtype=torch.int32, device="cuda")
    a = check(kernel, B, T, H, family, work, samples, label=count)
    b = check(kernel, B, T, H, family, None, label=count)
    assert torch.equal(a, b)


# ---- the ticket pair ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["bf16", "split"])
def test_ticket_pair_is_rearmed_between_launches(kernel):
    """Three launches in a row on one pair — fewer items than workgroups, more, fewer again — with different inputs: each meets
    its criterion and leaves the pair at [0, 0] (check asserts it after every ticketed launch)."""
    import torch
    n = n_cu()
    work = torch.zeros(2, dtype=torch.int32, device="cuda")
    for B, T, H, family in [(max(1, n // 6), 33, 3, "random"), (n + 5, 193, 1, "negative"), (max(1, n // 2 - 1), 257, 1, "match")]:
        check(kernel, B, T, H, family, work, label="pair")
        assert work.tolist() == [0, 0]


# ---- guard rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 17, 193, 225])
@pytest.mark.parametrize("kernel", ["bf16", "split"])
def test_guard_rows_stay_untouched(kernel, T):
    """n_cu + 1 items: 64 sentinel rows before and after the output are as they were (check asserts it for every launch of
    this file; these are the lengths at which the last strip is nearly empty)."""
    import torch
    B = n_cu() + 1
    for work in (torch.zeros(2, dtype=torch.int32, device="cuda"), None):
        check(kernel, B, T, 1, "random", work, label="guard")


# ---- rejected arguments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,head_dim", [(289, 64), (64, 32)])
def test_rejected_arguments_launch_nothing(T, head_dim):
    import torch
    qkv = torch.zeros(1, T, 3, 2, 64, device="cuda")
    work = torch.zeros(2, dtype=torch.int32, device="cuda")
    for kernel, entry in (("bf16", "static"), ("bf16", "dyn"), ("split", None)):
        st, buf = launch(kernel, qkv, 1, T, 2, work, head_dim=head_dim, entry=entry)
        assert st == -1, (kernel, entry, st)                        # BSC_E_INVALID
        assert bool((buf == SENTINEL).all()) and work.tolist() == [0, 0]
