"""Two builds of libbscnav.so in ONE process: the split GEMM's outputs must be bit-identical (torch.equal) on the forward's four
GEMM calls (qkv, fc1 with the LayerNorm in the load; proj, fc2 with the residual epilogue + row statistics) and on the edge shapes
of tests/test_gpu_gemm_split_dma.py; then the four calls are timed, the two builds alternating.
usage: gemm_dma_identity.py OTHER_LIB.so [frames]      (the build under test is the one _lib loads: BSC_LIB_PATH or the product)"""
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
sys.exit(1 if bad else 0)
