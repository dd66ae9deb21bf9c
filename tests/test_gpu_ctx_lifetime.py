"""A context's memory over its whole life: every entry point that allocates, grows or releases device / pinned-host memory of
a context (csrc/ctx_mem.cpp owns all of it), called in one sequence that ends with bsc_destroy, three times in one process.
Every call returns BSC_OK (the wrapper raises otherwise) and every output of cycles 2 and 3 equals cycle 1 bit for bit."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, G, D, GS, F = 48, 64, 16, 16, 128, 4
ITER, CS = 64, 4


def _cycle(mode):
    import torch
    import bsc_nav_amd as B
    import synth
    exact = mode == "exact"
    random.seed(5)                                   # the draws of the distance flush come from Python's generator
    out = []

    def keep(*arrays):
        out.extend(a.cpu().numpy() if hasattr(a, "cpu") else np.array(a) for a in arrays)

    rgb, depth, poses = synth.make_frames(13, F, H, W, "room")
    tokens = synth.make_tokens(13, F, G, D)
    chain = B.PoseChain()
    Ts = np.stack([chain.pc_transform(p) for p in poses])
    d, c, t = (torch.from_numpy(a).cuda() for a in (depth, rgb, tokens))

    def engine():
        # token_capacity 8 < iter_size: the first flush and import_store have to grow the pool
        return B.VoxelEngine(H, W, GS, 0.1, -2.0, 4.4, G, D, mode=mode, iter_size=ITER, cache_size=CS,
                             token_capacity=8 if exact else None, max_points=H * W)

    def keep_top(res):                               # (pos, sim, counts) of a localize call: what each query found
        pos, sim, cnt = res
        keep(cnt, *(pos[i, :cnt[i]] for i in range(len(cnt))), *(sim[i, :cnt[i]] for i in range(len(cnt))))

    def ingest(f):
        eng.ingest(d[f:f + 1], c[f:f + 1], t[f:f + 1], Ts[f:f + 1])

    def keep_log():
        cells, recs = eng.point_log()
        cells, recs = cells.cpu().numpy(), recs.cpu().numpy()
        # What the log promises is every voxel's points in their order of ingestion; inside a block of points the cells follow
        # each other in the order of the slots they won in the block's hash table, which differs from run to run.  Compared
        # here: the cells and records grouped by cell, stably (-1 marks the unused tail of a block, whose records are not written)
        order = np.flatnonzero(cells >= 0)
        order = order[np.argsort(cells[order], kind="stable")]
        keep(np.int64(len(cells)), cells[order], recs[order])

    eng = engine()
    # point log: on, on again with another capacity, off
    eng.point_log_enable(H * W)
    ingest(0)
    keep_log()
    eng.point_log_enable(2 * H * W + 7)
    ingest(1)
    keep_log()
    eng.point_log_enable(0)
    if exact:
        eng.flush()
        assert eng.store_usage()["capacity"] > 8     # the pool grew
        keep(*eng.export_store())
        ingest(2)
        eng.flush_surprise(1, 0.5, 0.95)
        ingest(3)
        eng.flush_surprise(2, 0.5, 0.95)             # 125 neighbours after 27: the neighbour lists are allocated again
        u = eng.store_usage()
        keep(u["pool_rows"], u["live_rows"], *eng.compact_store())
        keep(*eng.export_store())
    else:
        ingest(2)
        ingest(3)
        keep(*eng.export_dense())
    keep(*eng.export_rgb())
    pos = eng.export_rgb()[0]
    q = torch.from_numpy(synth.make_query_tokens(13, 8, 1, D).reshape(8, D)).cuda()
    keep_top(eng.localize(q[:1], K=10))                 # one query, then eight: the scratch grows
    keep_top(eng.localize(q, K=10))
    mid = pos[len(pos) // 2]
    keep_top(eng.localize_regions(q, K=10, radius=[12.0, 25.0, None, 40.0, 12.0, 25.0, None, 40.0], curr=mid, floor=(0, 63)))
    for centers, labels, sizes in eng.cluster_centers_batch(eps=6.0, min_samples=2):          # the resident results
        keep(centers, labels, sizes)
    rs = np.random.RandomState(3)
    hp = [rs.randint(0, 40, size=(n, 3)).astype(np.int32) for n in (30, 0, 17)]
    hs = [rs.uniform(0.1, 1.0, size=len(p)).astype(np.float32) for p in hp]
    for centers, labels, sizes in eng.cluster_centers_batch(hp, hs, eps=6.0, min_samples=2):  # host arrays
        keep(centers, labels, sizes)
    keep(eng.frontier_mask())
    fc = eng.frontier_clusters(min_cluster_size=1)
    keep(fc["n"], fc["first"], fc["sizes"], fc["centers"], fc["gains"], fc["best"], fc["labels"])
    g = eng.geometry(d[0], Ts[0])
    keep(*(g[k] for k in sorted(g)))
    # export -> import into a second, fresh context
    eng2 = engine()
    eng2.import_rgb(*eng.export_rgb())
    if exact:
        eng2.import_store(*eng.export_store())
        assert eng2.store_usage()["capacity"] > 8
        keep(*eng2.export_store())
    else:
        eng2.import_dense(*eng.export_dense())
        keep(*eng2.export_dense())
    keep_top(eng2.localize(q, K=10))
    eng2.close()
    keys = torch.from_numpy(rs.randint(0, 1 << 31, size=12000).astype(np.int32)).cuda()     # two tiles of the sort
    vals = torch.arange(12000, dtype=torch.int32, device="cuda")
    keep(*eng.sort_pairs_u32(keys, vals))
    eng.close()
    return out


@pytest.mark.parametrize("mode", ["exact", "mean"])
def test_three_lifetimes_give_the_same_answers(mode):
    first = _cycle(mode)
    assert len(first) > 40 and sum(a.size for a in first) > 10000
    for n in (2, 3):
        again = _cycle(mode)
        assert len(again) == len(first)
        differ = [i for i, (a, b) in enumerate(zip(first, again))
                  if not (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())]
        assert not differ, f"cycle {n}: outputs {differ} differ from cycle 1"
