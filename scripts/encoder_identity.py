"""Two builds of libbscnav.so in ONE process: the encoder kernels' outputs must be bit-identical (torch.equal) — the split GEMM on
the forward's four GEMM calls (qkv, fc1 with the LayerNorm in the load; proj, fc2 with the residual epilogue + row statistics) and
on the edge shapes of tests/test_gpu_gemm_split_dma.py, the attention launches (bsc_enc_attention_dyn, bsc_enc_attention_split) at
T = 197 and 261 with a few more items than CUs, with the ticket pair and without.  Then the four calls, and the f32 forward at
`frames` frames, are timed with the two builds alternating (after 2 s of warm load; median, minimum and spread per build).
--bars: for two builds whose GEMMs sum a chunk in another order (another MFMA shape) and so are not bit-identical.  The GEMM checks
become the bars of the tests — each build's four calls within max(1e-5, 2 e32) of an fp64 evaluation, e32 = PyTorch's f32 op's own
error against it; each build's forward no further from an fp64 forward of the first frames than PyTorch's f32 forward is, x1.5 — and
the verdict becomes: this build's forward median below the other's MINIMUM by more than four times the other's spread.  The edge
shapes are left to tests/test_gpu_gemm_split_*.py, which hold one build to the same bars; the attention launches stay bit-identical.
usage: encoder_identity.py OTHER_LIB.so [frames] [turns] [--bars]   (the build under test is the one _lib loads: BSC_LIB_PATH or the product)"""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bsc_nav_amd import encoder, _lib

BARS = "--bars" in sys.argv
sys.argv = [a for a in sys.argv if a != "--bars"]
new = _lib.load()
old = C.CDLL(sys.argv[1])
for name, (res, args) in _lib.SIGNATURES.items():
    fn = getattr(old, name)
    fn.restype, fn.argtypes = res, args
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 768
SL = encoder.SplitLinear
bad = 0


def use(lib):
    _lib._lib = lib


def both(fn):
    """fn() -> tensors, under either build"""
    use(new); a = fn()
    use(old); b = fn()
    use(new)
    return a, b


def same(name, a, b):
    global bad
    ok = all(torch.equal(x.view(torch.int16) if x.dtype == torch.float16 else x.view(torch.int32), y.view(torch.int16) if y.dtype == torch.float16 else y.view(torch.int32))
             for x, y in zip(a, b))
    bad += not ok
    print(f"{'identical' if ok else 'DIFFERENT'}  {name}", flush=True)


def pieces_back(p, scale):
    """(M, 2N) fp16 pieces in the chunk-interleaved layout -> (M, N) float64 of (h + l) / scale"""
    v = p.view(p.shape[0], -1, 2, 32)
    return (v[:, :, 0].double() + v[:, :, 1].double()).reshape(p.shape[0], -1) / scale


def bars(name, outs, ref64, ref32):
    """each build's output (float64) against the fp64 evaluation: within max(1e-5, 2 e32)"""
    global bad
    e32 = (ref32.double() - ref64).abs().max().item()
    errs = [(o - ref64).abs().max().item() for o in outs]
    ok = max(errs) <= max(1e-5, 2.0 * e32)
    bad += not ok
    print(f"{'within the bars' if ok else 'OUTSIDE THE BARS'}  {name}: error against fp64, this build {errs[0]:.3g}, other build {errs[1]:.3g}; e32 {e32:.3g}", flush=True)


def lin(K, N, seed):
    torch.manual_seed(seed)
    l = torch.nn.Linear(K, N).cuda().float()
    torch.nn.init.trunc_normal_(l.weight, std=0.02)
    return l


def resid_call(sl, a, r, pieces, stats_on, sc=4.0):
    M, N = r.shape
    u = r.clone()
    st = torch.zeros(M, encoder.LN_REC, device="cuda")
    mu = r.mean(1).contiguous()
    kw = dict(ln_stats=st, ln_mu=mu) if stats_on else {}
    if pieces:
        sl(a, 2, resid=u, out=u, a_scale=sc, a_pieces=True, **kw)
    else:
        sl(a, 2, resid=u, out=u, **kw)
    return (u, st)


def ln_records(x):
    M = x.shape[0]
    mean = x.mean(1)
    st = torch.zeros(M, encoder.LN_REC, device="cuda")
    st[:, 0] = mean
    st[:, 3] = ((x - mean[:, None]) ** 2).sum(1)
    return st, torch.zeros(M, device="cuda")


# ---- edge shapes -----------------------------------------------------------------------------------------------------------------
for M, N, K, forms in () if BARS else ((8200, 128, 128, (False, True)), (8200, 768, 64, (False, True)), (999, 768, 768, (True,)), (8449, 1024, 96, (False, True))):
    sl = SL(lin(K, N, M + N + K))
    a = torch.randn(M, K, device="cuda")
    ap = encoder.split_rows(a, 4.0)
    r = torch.randn(M, N, device="cuda") * 4
    for st_on in forms:
        same(f"residual M={M} N={N} K={K} stats={st_on} f32 rows", *both(lambda: resid_call(sl, a, r, False, st_on)))
        same(f"residual M={M} N={N} K={K} stats={st_on} pieces", *both(lambda: resid_call(sl, ap, r, True, st_on)))
for M, N in () if BARS else ((8200, 256), (8449, 2304), (8200, 2336)):
    for K in (128, 1024):
        l = lin(K, N, M + N + K)
        lnk = torch.nn.LayerNorm(K, eps=1e-6).cuda()
        lnk.weight.data.uniform_(0.5, 1.5)
        sl, sll = SL(l), SL(l, lnk)
        x = torch.randn(M, K, device="cuda") + 1.0
        xp = encoder.split_rows(x, 4.0)
        st, mu = ln_records(x)
        for epi in (0, 1, 3):
            same(f"M={M} N={N} K={K} epilogue={epi} f32 rows -> f32 / pieces, pieces -> pieces",
                 *both(lambda: (sl(x, epi), sl(x, epi, c_pieces_scale=2.0), sl(xp, epi, a_scale=4.0, a_pieces=True, c_pieces_scale=2.0))))
            same(f"M={M} N={N} K={K} epilogue={epi} LayerNorm in the load", *both(lambda: (sll(x, epi, a_ln=True, ln_stats=st, ln_mu=mu, c_pieces_scale=2.0),)))

# ---- attention ---------------------------------------------------------------------------------------------------------------------
def attention(kind, x, B, T, H, ticket):
    lib = _lib.load()
    work = torch.zeros(2, dtype=torch.int32, device="cuda") if ticket else None
    wp = C.c_void_p(work.data_ptr()) if ticket else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros(B * T, (1 if kind == "dyn" else 2) * H * 64, dtype=torch.int16, device="cuda")
    if kind == "dyn":
        _lib.check(lib.bsc_enc_attention_dyn(C.c_void_p(x.data_ptr()), B, T, H, 64, C.c_void_p(out.data_ptr()), wp, stream))
    else:
        _lib.check(lib.bsc_enc_attention_split(C.c_void_p(x.data_ptr()), B, T, H, 64, C.c_void_p(out.data_ptr()), 16.0, wp, stream))
    torch.cuda.synchronize()
    return (out.view(torch.float16),) + ((work.to(torch.float32),) if ticket else ())


n_cu = torch.cuda.get_device_properties(0).multi_processor_count
for T in (197, 261):
    H = 3
    B = (n_cu + 5 + H - 1) // H
    torch.manual_seed(T)
    qkv = torch.randn(B, T, 3, H, 64, device="cuda") * 1.5
    xb = qkv.bfloat16().contiguous()
    xs = encoder.split_rows(qkv.view(B * T, 3 * H * 64), 1.0)
    for ticket in (True, False):
        same(f"bsc_enc_attention_dyn T={T} items={B * H} ticket={ticket}", *both(lambda: attention("dyn", xb, B, T, H, ticket)))
        same(f"bsc_enc_attention_split T={T} items={B * H} ticket={ticket}", *both(lambda: attention("split", xs, B, T, H, ticket)))

# ---- the forward's four calls ------------------------------------------------------------------------------------------------------
M, Wd = frames * 197, 768
u0 = torch.randn(M, Wd, device="cuda")
st, mu = ln_records(u0)
lnw = torch.nn.LayerNorm(Wd, eps=1e-6).cuda()
calls = []
RB = 16384          # rows per block of the fp64 evaluations
for name, N, epi, cps in (("qkv", 2304, 0, 1.0), ("fc1", 3072, 3, 4.0)):
    l = lin(Wd, N, N)
    sll = SL(l, lnw)
    out = torch.empty(M, 2 * N, dtype=torch.float16, device="cuda")
    fn = (lambda sll=sll, epi=epi, cps=cps, out=out: (sll(u0, epi, a_ln=True, ln_stats=st, ln_mu=mu, c_pieces_scale=cps, out=out),))
    a, b = both(lambda: tuple(t.clone() for t in fn()))
    if BARS:
        F = torch.nn.functional
        act = (lambda t: t) if epi == 0 else F.gelu
        for r0 in range(0, M, 4 * RB):          # (every fourth block: the fp64 product of all rows is a minute of the device's time)
            x = u0[r0:r0 + RB]
            ref64 = act(F.layer_norm(x.double(), (Wd,), lnw.weight.double(), lnw.bias.double(), 1e-6) @ l.weight.double().t() + l.bias.double())
            ref32 = act(F.layer_norm(x, (Wd,), lnw.weight, lnw.bias, 1e-6) @ l.weight.t() + l.bias)
            bars(f"{name} rows {r0}..{r0 + x.shape[0]}", [pieces_back(t[0][r0:r0 + RB], cps) for t in (a, b)], ref64, ref32)
    else:
        same(f"{name} M={M}", a, b)
    del a, b
    calls.append((name, fn))
for name, K, sc in (("proj", 768, 16.0), ("fc2", 3072, 4.0)):
    l = lin(K, Wd, K)
    sl = SL(l)
    af = torch.randn(M, K, device="cuda")
    ap = encoder.split_rows(af, sc)
    a, b = both(lambda: resid_call(sl, ap, u0, True, True, sc))
    if BARS:
        for r0 in range(0, M, 4 * RB):
            x = af[r0:r0 + RB]
            ref64 = x.double() @ l.weight.double().t() + l.bias.double() + u0[r0:r0 + RB].double()
            ref32 = x @ l.weight.t() + l.bias + u0[r0:r0 + RB]
            bars(f"{name} rows {r0}..{r0 + x.shape[0]}", [t[0][r0:r0 + RB].double() for t in (a, b)], ref64, ref32)
    else:
        same(f"{name} M={M}", a, b)
    del a, b, af
    u = u0.clone()
    st2, mu2 = st.clone(), mu.clone()
    calls.append((name, lambda sl=sl, ap=ap, sc=sc, u=u, st2=st2, mu2=mu2: sl(ap, 2, resid=u, out=u, a_scale=sc, a_pieces=True, ln_stats=st2, ln_mu=mu2)))
print(("ALL WITHIN THE BARS" if BARS else "ALL IDENTICAL") if not bad else f"{bad} DIFFERENT", flush=True)


def timeit(fn, reps=10):
    fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3


def warm(fn, seconds=2.0):
    """warm load before a timed series: the two builds alternating for `seconds` of device time"""
    spent = 0.0
    while spent < seconds * 1e6:
        for lib in (old, new):
            use(lib)
            spent += timeit(fn, 4) * 5


def stat(v):
    return f"median {sorted(v)[len(v) // 2]:9.1f}  min {min(v):9.1f}  spread {max(v) - min(v):7.1f}"


turns = int(sys.argv[3]) if len(sys.argv) > 3 else 5
for name, fn in calls:
    t = {"new": [], "old": []}
    warm(fn)
    for _ in range(turns):
        for key, lib in (("old", old), ("new", new)):
            use(lib)
            t[key].append(timeit(fn))
    use(new)
    print(f"{name}: other build {' '.join(f'{v:7.1f}' for v in t['old'])} us | this build {' '.join(f'{v:7.1f}' for v in t['new'])} us", flush=True)
    print(f"{name} us: other build {stat(t['old'])} | this build {stat(t['new'])}", flush=True)

# ---- the f32 forward, the two builds alternating: turns of about a second; the other build's own spread is the noise of this run --------
vit = encoder.RandomViT("vit_b16", image_size=224, seed=0, dtype=torch.float32).cuda()
rgb = torch.randint(0, 255, (frames, 480, 640, 4), dtype=torch.uint8, device="cuda")
outs = both(lambda: (vit.patch_tokens(rgb).clone(),))
if BARS:
    nf = min(frames, 8)
    vit.split_gemm = False
    f32 = vit.patch_tokens(rgb[:nf])
    vit.split_gemm = True
    v64 = encoder.RandomViT("vit_b16", image_size=224, seed=0, dtype=torch.float64).cuda()
    v64.load_state_dict({k: v.double() for k, v in vit.state_dict().items()})
    v64.fused = False
    c = v64.forward_features(v64.preprocess(rgb[:nf]).double())["x_norm_patchtokens"].reshape(f32.shape)
    e_torch = (f32.double() - c).abs().max().item()
    errs = [(o[0][:nf].double() - c).abs().max().item() for o in outs]
    ok = max(errs) <= max(1.5 * e_torch, 5e-6)
    bad += not ok
    print(f"{'within the bars' if ok else 'OUTSIDE THE BARS'}  f32 forward, {frames} frames, the first {nf} against fp64: this build {errs[0]:.3g}, "
          f"other build {errs[1]:.3g}; PyTorch f32 {e_torch:.3g}; the builds differ by {(outs[0][0] - outs[1][0]).abs().max().item():.3g}", flush=True)
    del v64, c, f32
else:
    same(f"f32 forward, {frames} frames", *outs)
del outs
use(new)
per = timeit(lambda: vit.patch_tokens(rgb), 2)
reps = max(2, int(round(1e6 / per)))
warm(lambda: vit.patch_tokens(rgb))
t = {"new": [], "old": []}
for _ in range(turns):
    for key, lib in (("old", old), ("new", new)):
        use(lib)
        t[key].append(timeit(lambda: vit.patch_tokens(rgb), reps) / 1e3)
use(new)
med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
spread = max(t["old"]) - min(t["old"])
print(f"forward {frames} frames, {turns} turns of {reps} forwards, ms: other build {' '.join(f'{v:.3f}' for v in t['old'])} | this build "
      f"{' '.join(f'{v:.3f}' for v in t['new'])}", flush=True)
print(f"forward medians: other build {med['old']:.3f} ms, this build {med['new']:.3f} ms; spread of the other build's turns {spread:.3f} ms -> "
      f"{'within the spread' if med['new'] - med['old'] <= spread else 'SLOWER by more than the spread'}", flush=True)
print(f"forward ms: other build {stat(t['old'])} | this build {stat(t['new'])}", flush=True)
slow = med["new"] - med["old"] > spread
if BARS:
    # the bar a change of the MFMA shape is kept by: clear of the other build's best turn by four times its own spread
    gain = min(t["old"]) - med["new"]
    slow = gain <= 4 * spread
    print(f"this build's median is {gain:.3f} ms below the other build's minimum; four times its spread are {4 * spread:.3f} ms -> "
          f"{'CLEARS the bar' if not slow else 'does NOT clear the bar'}", flush=True)
sys.exit(1 if bad or slow else 0)
