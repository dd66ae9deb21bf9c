"""Timings of bsc_render_views (the numbers of DESIGN.md section 4e).

usage: render_time.py [--logv 20] [--gs 256] [--views 1 8 64] [--reps 15] [--frames 16]

Two scenes: "random" — 2^logv random distinct voxels in a gs^3 grid, the memory of scripts/topdown_time.py, seen from random
orientations at its centre; "room" — `--frames` synthetic 640x480 frames of a walk through the room of bsc_nav_amd.synthetic,
ingested every pixel, seen from the poses of the walk.  Per scene 1 / 8 / 64 views of 640x480 and of 160x120: the median of `--reps`
host-timed calls after a warm-up call, each synchronised (the call itself returns after its work has completed), all three outputs
and the id image alone.  Host times of whole calls: the brick pass and the transfer of the transforms are inside."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsc_nav_amd as B  # noqa: E402
from bsc_nav_amd import synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--logv", type=int, default=20)
ap.add_argument("--gs", type=int, default=256)
ap.add_argument("--views", type=int, nargs="*", default=[1, 8, 64])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--frames", type=int, default=16)
a = ap.parse_args()
SIZES = [(480, 640), (120, 160)]


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


def report(eng, scene, transforms):
    for H, W in SIZES:
        kinv = np.linalg.inv(B.cam_mat_fov(H, W, 90))
        for V in a.views:
            T = transforms[np.arange(V) % len(transforms)]
            got = eng.render_views(T, size=(H, W), kinv=kinv)
            hit = float((got["voxel"] >= 0).float().mean())
            d_all = timed(lambda: eng.render_views(T, size=(H, W), kinv=kinv), a.reps)
            d_id = timed(lambda: eng.render_views(T, size=(H, W), kinv=kinv, want=("voxel",)), a.reps)
            print(f"{scene:6s} {W}x{H} V={V:3d}  render_views {d_all:8.3f} ms   ids only {d_id:8.3f} ms   "
                  f"{V * H * W / d_all / 1e3:8.1f} Mrays/s   {100 * hit:5.1f} % of the rays hit")


# ---- random voxels -----------------------------------------------------------------------------------------------------------
V, gs, D = 1 << a.logv, a.gs, 4
nh = gs
gen = torch.Generator(device="cuda").manual_seed(5)
codes = torch.randperm(gs * gs * nh, device="cuda", generator=gen)[:V]
keys = torch.stack([codes // (gs * nh), (codes // nh) % gs, codes % nh], dim=1).to(torch.int32).contiguous()
colours = torch.randint(1, 256, (V, 3), device="cuda", generator=gen).to(torch.uint8)
eng = B.VoxelEngine(480, 640, gs, 0.1, 0.0, 0.0, 16, D, mode="mean", voxel_capacity=V + 8, max_points=4096, min_h=0, max_h=nh)
eng.dense_replace(keys, torch.ones((V, D), device="cuda"), torch.ones(V, dtype=torch.int32, device="cuda"), colours,
                  torch.ones(V, device="cuda"))
bricks = ((gs + 3) // 4) ** 2 * ((nh + 3) // 4)
print(f"random: {V} voxels in {gs} x {gs} x {nh}, brick scratch {bricks * 8 / 1e6:.1f} MB, t in ({eng.cfg.min_depth}, {eng.cfg.max_depth}), "
      f"{torch.cuda.get_device_name(0)}")
rot = R.random(64, random_state=7).as_matrix()
Ts = np.tile(np.eye(4), (64, 1, 1))
Ts[:, :3, :3] = rot
Ts[:, :3, 3] = (0.33, -0.21, 0.1 * nh / 2 + 0.04)
report(eng, "random", Ts)
eng.close()

# ---- a room, ingested ---------------------------------------------------------------------------------------------------------
F, H, W, g = a.frames, 480, 640, 16
rgb, depth, poses = synthetic.make_frames(7, F, H, W, "room")
eng = B.VoxelEngine(H, W, gs, 0.1, -2.0, 4.4, g, 32, mode="mean", voxel_capacity=1 << 20, max_points=H * W)
chain = B.PoseChain()
tokens = torch.rand((1, g, g, 32), device="cuda")
for f in range(F):
    eng.ingest(depth[f:f + 1], rgb[f:f + 1], tokens, chain.pc_transform(poses[f])[None])
eng.sync()
n = eng.counters()["max_id"]
bricks = ((gs + 3) // 4) ** 2 * ((eng.nh + 3) // 4)
print(f"room: {n} voxels from {F} frames in {gs} x {gs} x {eng.nh}, brick scratch {bricks * 8 / 1e6:.1f} MB")
report(eng, "room", np.stack([chain.transform_of(p) for p in poses]))
eng.close()
