"""Timings of bsc_topdown_slices beside the way the same map was had before it: export_rgb() and a vectorised NumPy reduction on
the host (the numbers of DESIGN.md section 4d).

usage: topdown_time.py [--logv 20] [--gs 256] [--s 1 8 64] [--reps 15]

2^logv random distinct voxels in a gs^3 grid (a dense map of 4-D rows: only positions and colours matter here); per S bands of
random bounds.  Medians of `--reps` host-timed calls after a warm-up call, synchronised; the host way is timed `--reps` / 5 times,
at least twice, and both results are compared before anything is printed."""
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
ap.add_argument("--gs", type=int, default=256)
ap.add_argument("--s", type=int, nargs="*", default=[1, 8, 64])
ap.add_argument("--reps", type=int, default=15)
a = ap.parse_args()
V, gs, D = 1 << a.logv, a.gs, 4
nh = gs
gen = torch.Generator(device="cuda").manual_seed(5)
codes = torch.randperm(gs * gs * nh, device="cuda", generator=gen)[:V]
keys = torch.stack([codes // (gs * nh), (codes // nh) % gs, codes % nh], dim=1).to(torch.int32).contiguous()
colours = torch.randint(1, 256, (V, 3), device="cuda", generator=gen).to(torch.uint8)
eng = B.VoxelEngine(48, 64, gs, 0.1, 0.0, 0.0, 16, D, mode="mean", voxel_capacity=V + 8, max_points=4096, min_h=0, max_h=nh)
eng.dense_replace(keys, torch.ones((V, D), device="cuda"), torch.ones(V, dtype=torch.int32, device="cuda"), colours,
                  torch.ones(V, device="cuda"))
print(f"{V} voxels in {gs} x {gs} x {nh}, mask scratch {gs * gs * ((nh + 63) // 64) * 8 / 1e6:.1f} MB, {torch.cuda.get_device_name(0)}")


def timed(fn, reps):
    fn()
    lat = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t)
    return statistics.median(lat) * 1e3


def host_way(bands):
    """What a caller did before: every voxel to the host, then per band the highest voxel of each column."""
    pos, rgb, _ = eng.export_rgb()
    order = np.argsort(pos[:, 2], kind="stable")
    cell, h, col = (pos[:, 0].astype(np.int64) * gs + pos[:, 1])[order], pos[order, 2], rgb[order]
    out = np.zeros((len(bands), gs * gs, 3), np.uint8)
    for s, (lo, hi) in enumerate(bands):
        sel = (h >= lo) & (h <= hi)
        out[s][cell[sel]] = col[sel]                             # ascending h: the highest voxel of a column is written last
    return out.reshape(len(bands), gs, gs, 3)


rng = np.random.RandomState(3)
for S in a.s:
    bands = [tuple(sorted(int(v) for v in rng.randint(0, nh, size=2))) for _ in range(S)]
    got = eng.topdown_slices(bands)
    assert np.array_equal(got["rgb"].cpu().numpy(), host_way(bands)), "the two ways disagree"
    d_all = timed(lambda: eng.topdown_slices(bands), a.reps)
    d_rgb = timed(lambda: eng.topdown_slices(bands, heights=False, counts=False), a.reps)
    h_ms = timed(lambda: host_way(bands), max(2, a.reps // 5))
    print(f"S={S:3d}  topdown_slices {d_all:8.3f} ms   colours only {d_rgb:8.3f} ms   export_rgb + NumPy on the host {h_ms:9.2f} ms")
rb = timed(lambda: eng.rebuild_topdown(), a.reps)
print(f"rebuild_topdown() {rb:8.3f} ms")
eng.close()
