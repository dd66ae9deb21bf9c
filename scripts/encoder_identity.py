"""Two builds of libbscnav.so in ONE process: the encoder kernels' outputs must be bit-identical (torch.equal) — the split GEMM on
the forward's four GEMM calls (qkv, fc1 with the LayerNorm in the load; proj, fc2 with the residual epilogue + row statistics) and
on the edge shapes of tests/test_gpu_gemm_split_dma.py, the attention launches (bsc_enc_attention_dyn, bsc_enc_attention_split) at
T = 197 and 261 with a few more items than CUs, with the ticket pair and without.  Then the four calls, and the f32 forward at
`frames` frames, are timed with the two builds alternating.
usage: encoder_identity.py OTHER_LIB.so [frames] [turns]   (the build under test is the one _lib loads: BSC_LIB_PATH or the product)"""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bsc_nav_amd import encoder, _lib

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
for M, N, K, forms in ((8200, 128, 128, (False, True)), (8200, 768, 64, (False, True)), (999, 768, 768, (True,)), (8449, 1024, 96, (False, True))):
    sl = SL(lin(K, N, M + N + K))
    a = torch.randn(M, K, device="cuda")
    ap = encoder.split_rows(a, 4.0)
    r = torch.randn(M, N, device="cuda") * 4
    for st_on in forms:
        same(f"residual M={M} N={N} K={K} stats={st_on} f32 rows", *both(lambda: resid_call(sl, a, r, False, st_on)))
        same(f"residual M={M} N={N} K={K} stats={st_on} pieces", *both(lambda: resid_call(sl, ap, r, True, st_on)))
for M, N in ((8200, 256), (8449, 2304), (8200, 2336)):
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
for name, N, epi, cps in (("qkv", 2304, 0, 1.0), ("fc1", 3072, 3, 4.0)):
    sll = SL(lin(Wd, N, N), lnw)
    out = torch.empty(M, 2 * N, dtype=torch.float16, device="cuda")
    fn = (lambda sll=sll, epi=epi, cps=cps, out=out: (sll(u0, epi, a_ln=True, ln_stats=st, ln_mu=mu, c_pieces_scale=cps, out=out),))
    same(f"{name} M={M}", *both(lambda: tuple(t.clone() for t in fn())))
    calls.append((name, fn))
for name, K, sc in (("proj", 768, 16.0), ("fc2", 3072, 4.0)):
    sl = SL(lin(K, Wd, K))
    ap = encoder.split_rows(torch.randn(M, K, device="cuda"), sc)
    same(f"{name} M={M}", *both(lambda: resid_call(sl, ap, u0, True, True, sc)))
    u = u0.clone()
    st2, mu2 = st.clone(), mu.clone()
    calls.append((name, lambda sl=sl, ap=ap, sc=sc, u=u, st2=st2, mu2=mu2: sl(ap, 2, resid=u, out=u, a_scale=sc, a_pieces=True, ln_stats=st2, ln_mu=mu2)))
print("ALL IDENTICAL" if not bad else f"{bad} DIFFERENT", flush=True)


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


for name, fn in calls:
    t = {"new": [], "old": []}
    for _ in range(3):
        for key, lib in (("old", old), ("new", new)):
            use(lib)
            t[key].append(timeit(fn))
    use(new)
    print(f"{name}: other build {' '.join(f'{v:7.1f}' for v in t['old'])} us | this build {' '.join(f'{v:7.1f}' for v in t['new'])} us", flush=True)

# ---- the f32 forward, the two builds alternating: turns of about a second; the other build's own spread is the noise of this run --------
turns = int(sys.argv[3]) if len(sys.argv) > 3 else 5
vit = encoder.RandomViT("vit_b16", image_size=224, seed=0, dtype=torch.float32).cuda()
rgb = torch.randint(0, 255, (frames, 480, 640, 4), dtype=torch.uint8, device="cuda")
outs = both(lambda: (vit.patch_tokens(rgb).clone(),))
same(f"f32 forward, {frames} frames", *outs)
del outs
use(new)
per = timeit(lambda: vit.patch_tokens(rgb), 2)
reps = max(2, int(round(1e6 / per)))
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
slow = med["new"] - med["old"] > spread
sys.exit(1 if bad or slow else 0)
