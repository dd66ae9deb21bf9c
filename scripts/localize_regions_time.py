"""Timings of bsc_localize_regions against bsc_localize (the numbers of DESIGN.md, localize section).

usage: localize_regions_time.py [--map dense|store] [--logv 20] [--q 1 8 256] [--sweep]

  (a) localize, one shared region of radius 30 around the grid centre (and unrestricted)
  (b) localize_regions, that region for every query
  (c) localize_regions, radius 30 around Q different centres
  no-tax pair: localize_regions with every region disabled against localize unrestricted
  --sweep: Q = 8, shared centre, a sweep of radii, BSC_REGION_PRUNE=never against =always (the pruning threshold's crossover)
Medians of `--reps` host-timed calls after a warm-up call, synchronised; the scan's own HIP-event time beside them."""
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
ap.add_argument("--map", default="dense", choices=["dense", "store"])
ap.add_argument("--logv", type=int, default=20)
ap.add_argument("--q", type=int, nargs="*", default=[1, 8, 256])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--sweep", action="store_true")
a = ap.parse_args()
V, D, gs, K = 1 << a.logv, 1024, 512, 100
gen = torch.Generator(device="cuda").manual_seed(5)
codes = torch.randperm(gs ** 3, device="cuda", generator=gen)[:V]
keys = torch.stack([codes // (gs * gs), (codes // gs) % gs, codes % gs], dim=1).to(torch.int32).contiguous()
if a.map == "dense":
    rows = torch.randn((V, D), device="cuda", generator=gen)
    eng = B.VoxelEngine(48, 64, gs, 0.1, -25.6, 25.6, 16, D, mode="mean", voxel_capacity=V + 8, max_points=4096)
    eng.dense_replace(keys, rows, torch.ones(V, dtype=torch.int32, device="cuda"))
    n_rows = V
else:
    cnt = torch.randint(1, 11, (V,), device="cuda", generator=gen, dtype=torch.int32)
    T = int(cnt.sum().item())
    eng = B.VoxelEngine(48, 64, gs, 0.1, -25.6, 25.6, 16, D, mode="exact", iter_size=256, voxel_capacity=V + 8,
                        token_capacity=T, max_points=4096)
    kk = keys.cpu().numpy()
    eng.import_rgb(kk, np.zeros((V, 3), np.uint8), np.ones(V, np.float32))
    rows_h = torch.empty((T, D), dtype=torch.float32)
    for s in range(0, T, 1 << 19):                            # host rows in slices: the device copy is the library's
        rows_h[s:s + (1 << 19)] = torch.randn((min(1 << 19, T - s), D), device="cuda", generator=gen).cpu()
    eng.import_store(kk, cnt.cpu().numpy(), rows_h.numpy(), np.zeros(T, np.float32))
    del rows_h
    n_rows = T
print(f"map {a.map}: {V} voxels, {n_rows} rows x {D} ({n_rows * D * 4 / 1e9:.1f} GB), {torch.cuda.get_device_name(0)}")


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
    n = max(1, st["launches"])
    return statistics.median(lat) * 1e3, st["ms"] / n, st["bytes"] / n


centre = [gs // 2] * 3
rng = np.random.RandomState(3)
for Q in a.q:
    q = torch.randn(Q, D, device="cuda", generator=gen)
    centres = rng.randint(40, gs - 40, size=(Q, 3))
    cases = [
        ("localize unrestricted", lambda: eng.localize(q, K=K)),
        ("(a) localize r=30 shared", lambda: eng.localize(q, K=K, radius=30.0, curr=centre)),
        ("no-tax localize_regions, all disabled", lambda: eng.localize_regions(q, K=K)),
        ("(b) localize_regions r=30 shared", lambda: eng.localize_regions(q, K=K, radius=30.0, curr=centre)),
        ("(c) localize_regions r=30, Q centres", lambda: eng.localize_regions(q, K=K, radius=30.0, curr=centres)),
    ]
    for name, fn in cases:
        ms, scan, nbytes = timed(fn)
        print(f"Q={Q:4d} {name:40s} call {ms:8.3f} ms   scan {scan:7.3f} ms   {nbytes / (D * 4.0 + 4.0 * Q):10.0f} rows streamed")
if a.sweep:
    Q = 8
    q = torch.randn(Q, D, device="cuda", generator=gen)
    k64 = keys.to(torch.int64)
    for radius in (30, 60, 100, 140, 170, 200, 230, 260, 300, 360):
        share = float((((k64 - torch.tensor(centre, device="cuda")) ** 2).sum(1) <= radius * radius).double().mean().item())
        out = []
        for knob in ("never", "always"):
            os.environ["BSC_REGION_PRUNE"] = knob
            out.append(timed(lambda: eng.localize_regions(q, K=K, radius=float(radius), curr=centre))[0])
        del os.environ["BSC_REGION_PRUNE"]
        print(f"sweep Q=8 radius {radius:4d}: visible share {share:6.3f}   full scan {out[0]:8.3f} ms   pruned {out[1]:8.3f} ms")
eng.close()
