"""Timings of the retrieval chain localize -> cluster centres for a batch of queries (the numbers of DESIGN.md section 4b).

usage: retrieve_batch_time.py [--logv 20] [--q 1 8 256] [--reps 25]

On the dense 2^20 x 1024 map, radius-30 regions around Q different centres, K = 100, DBSCAN(eps 10, min_samples 5):
  (a) localize_regions alone
  (b) localize_regions + a Python loop of cluster_centers(query_index=i) over the queries that found something
  (c) localize_regions + cluster_centers_batch() on the resident results
  (c') the same with BSC_CLUSTER_BITROWS=0: the recompute form of the kernel instead of the bit rows
and the two clustering steps on their own (the resident results stay put between calls).
Legs (a) and (b) need nothing this script's commit added: the script runs unchanged on older commits, where (c) is skipped.
Medians of `--reps` host-timed repetitions after warm-up calls, bsc_sync + device synchronize on both sides."""
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
ap.add_argument("--q", type=int, nargs="*", default=[1, 8, 256])
ap.add_argument("--reps", type=int, default=25)
a = ap.parse_args()
V, D, gs, K = 1 << a.logv, 1024, 512, 100
gen = torch.Generator(device="cuda").manual_seed(5)
codes = torch.randperm(gs ** 3, device="cuda", generator=gen)[:V]
keys = torch.stack([codes // (gs * gs), (codes // gs) % gs, codes % gs], dim=1).to(torch.int32).contiguous()
rows = torch.randn((V, D), device="cuda", generator=gen)
eng = B.VoxelEngine(48, 64, gs, 0.1, -25.6, 25.6, 16, D, mode="mean", voxel_capacity=V + 8, max_points=4096)
eng.dense_replace(keys, rows, torch.ones(V, dtype=torch.int32, device="cuda"))
has_batch = hasattr(eng, "cluster_centers_batch")
print(f"dense map: {V} voxels x {D} ({V * D * 4 / 1e9:.1f} GB), {torch.cuda.get_device_name(0)}, "
      f"cluster_centers_batch {'present' if has_batch else 'absent'}")


def both_sync():
    eng.sync()
    torch.cuda.synchronize()


def timed(fn, warm=3):
    for _ in range(warm):
        fn()
    lat = []
    for _ in range(a.reps):
        both_sync()
        t = time.perf_counter()
        fn()
        both_sync()
        lat.append(time.perf_counter() - t)
    return statistics.median(lat) * 1e3, min(lat) * 1e3


rng = np.random.RandomState(3)
for Q in a.q:
    q = torch.randn(Q, D, device="cuda", generator=gen)
    centres = rng.randint(40, gs - 40, size=(Q, 3))

    def localize():
        return eng.localize_regions(q, K=K, radius=30.0, curr=centres)

    def loop(n):
        return [eng.cluster_centers(K=int(n[i]), query_index=i) for i in range(Q) if n[i] > 0]

    def leg_b():
        loop(localize()[2])

    def leg_c():
        localize()
        eng.cluster_centers_batch()

    n = localize()[2]
    found = sum(len(r[2]) for r in loop(n))
    print(f"Q={Q:4d} results per query {int(n.min())}..{int(n.max())}, {found} clusters in the batch")
    legs = [("(a) localize_regions", lambda: localize()), ("(b) + loop of cluster_centers", leg_b)]
    if has_batch:
        legs.append(("(c) + cluster_centers_batch", leg_c))
    for name, fn in legs:
        med, best = timed(fn)
        print(f"Q={Q:4d} {name:42s} median {med:9.3f} ms   min {best:9.3f} ms")
    if has_batch:
        os.environ["BSC_CLUSTER_BITROWS"] = "0"
        med, best = timed(leg_c)
        del os.environ["BSC_CLUSTER_BITROWS"]
        print(f"Q={Q:4d} {'(c`) the same, recompute form':42s} median {med:9.3f} ms   min {best:9.3f} ms")
    localize()
    steps = [("clustering alone: loop", lambda: loop(n))]
    if has_batch:
        steps.append(("clustering alone: batch", lambda: eng.cluster_centers_batch()))
    for name, fn in steps:
        med, best = timed(fn)
        print(f"Q={Q:4d} {name:42s} median {med:9.3f} ms   min {best:9.3f} ms")
    if has_batch:
        os.environ["BSC_CLUSTER_BITROWS"] = "0"
        med, best = timed(lambda: eng.cluster_centers_batch())
        del os.environ["BSC_CLUSTER_BITROWS"]
        print(f"Q={Q:4d} {'clustering alone: batch, recompute form':42s} median {med:9.3f} ms   min {best:9.3f} ms")
eng.close()
