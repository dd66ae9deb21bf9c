"""One encoder GEMM shape through bsc_enc_gemm_split, in a loop, for rocprofv3 counters and the phase stamps.
usage: gemm_split_prof.py [qkv|proj|fc1|fc2|qkv_ln|fc1_ln|proj_st|fc2_st] [reps] [frames]
The plain names read pieces (qkv, fc1: bias / GELU to f32; proj, fc2: residual); the forms the forward runs are *_ln (LayerNorm in the
load, pieces out: k_gemm_split<1,8,8,1,{0,3},2,true,false>) and *_st (pieces in, residual + row statistics: <1,8,8,1,2,1,false,true>)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsc_nav_amd import encoder
name = sys.argv[1] if len(sys.argv) > 1 else "qkv"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
base, _, form = name.partition("_")
K, N, epi = {"qkv": (768, 2304, 0), "proj": (768, 768, 2), "fc1": (768, 3072, 3 if form == "ln" else 1), "fc2": (3072, 768, 2)}[base]
M = (int(sys.argv[3]) if len(sys.argv) > 3 else 384) * 197
lin = torch.nn.Linear(K, N).cuda().float()
torch.nn.init.trunc_normal_(lin.weight, std=0.02)
A = torch.randn(M, K, device="cuda")
R = torch.randn(M, N, device="cuda")
stats = torch.zeros(M, encoder.LN_REC, device="cuda")
mu = torch.zeros(M, device="cuda")
if form == "ln":
    ln = torch.nn.LayerNorm(K, eps=1e-6).cuda()
    mean = A.mean(1)
    stats[:, 0] = mean
    stats[:, 3] = ((A - mean[:, None]) ** 2).sum(1)
    sl = encoder.SplitLinear(lin, ln)
    for _ in range(reps):
        sl(A, epi, a_ln=True, ln_stats=stats, ln_mu=mu, c_pieces_scale=1.0)
else:
    sl = encoder.SplitLinear(lin)
    Ap = encoder.split_rows(A, 1.0)
    kw = dict(ln_stats=stats, ln_mu=mu) if form == "st" else {}
    for _ in range(reps):
        sl(Ap, epi, resid=R if epi == 2 else None, a_pieces=True, **kw)
torch.cuda.synchronize()
