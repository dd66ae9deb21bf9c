"""Timings of bsc_score_map beside bsc_localize_regions(K=100) on the same inputs (the numbers of DESIGN.md section 4c).

usage: score_map_time.py [--logv 20] [--dim 768] [--gs 256] [--q 1 8 256] [--reps 15]

A dense map of 2^logv rows x dim in a gs^3 grid; per Q the call without regions and with radius 30 around Q different centres.
Medians of `--reps` host-timed calls after a warm-up call, synchronised; beside each the scan's own HIP-event time per call
(bsc_kernel_stats(1)) and its share of the call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsc_nav_amd as B  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--logv", type=int, default=20)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--gs", type=int, default=256)
ap.add_argument("--q", type=int, nargs="*", default=[1, 8, 256])
ap.add_argument("--reps", type=int, default=15)
a = ap.parse_args()
V, D, gs, K = 1 << a.logv, a.dim, a.gs, 100
gen = torch.Generator(device="cuda").manual_seed(5)
codes = torch.randperm(gs ** 3, device="cuda", generator=gen)[:V]
keys = torch.stack([codes // (gs * gs), (codes // gs) % gs, codes % gs], dim=1).to(torch.int32).contiguous()
rows = torch.randn((V, D), device="cuda", generator=gen)
eng = B.VoxelEngine(48, 64, gs, 0.1, -gs * 0.05, gs * 0.05, 16, D, mode="mean", voxel_capacity=V + 8, max_points=4096)
eng.dense_replace(keys, rows, torch.ones(V, dtype=torch.int32, device="cuda"))
print(f"dense map: {V} rows x {D} ({V * D * 4 / 1e9:.1f} GB) in {gs}^3, {torch.cuda.get_device_name(0)}")


def timed(fn):
    fn()
    eng.kernel_stats(1, reset=True)
    lat = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t)
    st = eng.kernel_stats(1)
    return statistics.median(lat) * 1e3, st["ms"] / max(1, st["launches"])


rng = np.random.RandomState(3)
for Q in a.q:
    q = torch.randn(Q, D, device="cuda", generator=gen)
    centres = rng.randint(40, gs - 40, size=(Q, 3))
    for name, kw in (("no region", {}), ("radius 30, Q centres", dict(radius=30.0, curr=centres))):
        m_ms, m_scan = timed(lambda: eng.score_map(q, **kw))
        n_ms, n_scan = timed(lambda: eng.score_map(q, heights=False, **kw))
        l_ms, l_scan = timed(lambda: eng.localize_regions(q, K=K, **kw))
        print(f"Q={Q:4d} {name:22s} score_map {m_ms:8.3f} ms (scan {m_scan:7.3f} ms, {100 * m_scan / m_ms:5.1f} %)   "
              f"without heights {n_ms:8.3f} ms   localize_regions(K={K}) {l_ms:8.3f} ms (scan {l_scan:7.3f} ms, "
              f"{100 * l_scan / l_ms:5.1f} %)")
eng.close()
