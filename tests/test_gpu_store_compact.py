"""bsc_store_usage / bsc_compact_store and the two automatic compaction sites (BSC_STORE_COMPACT): the pool rows a merge of the
surprise policy leaves behind are reclaimed, and nothing a caller can observe changes."""
import random

import numpy as np
import pytest

import surprise_cases as SC
import surprise_replay as R
from test_gpu_surprise import _dist_replay, assert_store_matches

pytestmark = pytest.mark.gpu

GS, NH = 64, 8


def _engine(vox, D, cs, iter_size, mode="exact", token_capacity=None):
    import bsc_nav_amd as B
    eng = B.VoxelEngine(48, 64, GS, 1.0, 0.0, float(NH), 16, D, mode=mode, iter_size=iter_size, cache_size=cs,
                        voxel_capacity=max(len(vox), 1), token_capacity=token_capacity)
    if len(vox):
        eng.import_rgb(vox, np.zeros((len(vox), 3), np.uint8), np.zeros(len(vox), np.float32))
    return eng


def _voxels(rs, n):
    cells = 1 + rs.choice(GS * GS * NH - 1, n, replace=False)            # not cell 0
    return np.stack([cells // (GS * NH), (cells // NH) % GS, cells % NH], 1).astype(np.int32)


def _cache(tok, rs, vox, who, ks, n):
    """n cache rows: tokens of the directions ks at the voxels vox[who], then the zero tail at [0,0,0]."""
    m = len(who)
    assert m <= n
    pos, feat, dis = np.zeros((n, 3), np.int32), np.zeros((n, tok.D), np.float32), np.zeros(n, np.float32)
    pos[:m], feat[:m], dis[:m] = vox[who], tok.many(ks), rs.uniform(0.5, 5.0, m).astype(np.float32)
    return pos, feat, dis


def _surprise(eng, st, cache, radius, cs):
    eng.import_cache(*cache)
    eng.flush_surprise(radius, SC.STHR, SC.BTHR)
    counts, margins = R.replay(st, cache[0], cache[1], cache[2], radius, SC.STHR, SC.BTHR, cs)
    assert min(margins.values()) >= 1e-4, margins
    return counts


def _import_store(eng, st, D):
    pos, cnt, feat, dis, _ = R.store_to_arrays(st, D)
    eng.import_store(pos, cnt, feat, dis.astype(np.float32))


def _twice(rs, S, n):
    """S voxels twice each in random order, cut to n rows: (voxel of a row, the row is the voxel's second one)."""
    who = rs.permutation(np.repeat(np.arange(S), 2))[:n]
    second = np.zeros(len(who), bool)
    seen = set()
    for i, v in enumerate(who):
        second[i] = v in seen
        seen.add(v)
    return who, second


def _queries(tok, rs, nq):
    import torch
    k = np.arange(nq) % tok.nd
    q = tok.dirs[k] + 0.05 * rs.standard_normal((nq, tok.D))
    return torch.from_numpy(q.astype(np.float32)).cuda()


def _observe(eng, qs, monkeypatch):
    out = list(eng.export_store())
    for q in qs:
        out += list(eng.localize(q, K=20))
    for prune in ("always", "never"):
        monkeypatch.setenv("BSC_REGION_PRUNE", prune)
        out += list(eng.localize_regions(qs[1], K=20, radius=14.0, curr=(32, 32, 4), floor=(1, 6)))
    monkeypatch.delenv("BSC_REGION_PRUNE")
    return out


def test_leak_is_reclaimed(monkeypatch):
    """20 001 voxels, 4-D tokens, radius 0 (every row is accepted: the direction decides between append and merge).  Cycle 1
    gives 3 000 voxels two directions each; cycle 2 gives each a row of its first direction (appended to a fresh pool row,
    merged, the fresh row dead) and a row of a third direction (appended, live), in random order: ~3 000 dead rows lie between
    ~3 000 live ones, about half of the live ones above L — more movers than one 1024-thread block.  The zero tail of cycle 2
    creates grid_0_0_0 last: the rows of entry vcap are the highest and must move."""
    monkeypatch.setenv("BSC_STORE_COMPACT", "never")
    D, cs, nd, S, N = 4, 4, 3, 3000, 6000
    rs = np.random.RandomState(7)
    tok = SC.Tokens(rs, nd, D)
    vox = _voxels(rs, 20001)
    k0 = rs.randint(nd, size=S)
    eng = _engine(vox, D, cs, N)
    st = {}
    who, second = _twice(rs, S, N)
    c1 = _cache(tok, rs, vox, who, np.where(second, (k0[who] + 1) % nd, k0[who]), N)
    _surprise(eng, st, c1, 0, cs)
    who, second = _twice(rs, S, N - 40)
    counts = _surprise(eng, st, _cache(tok, rs, vox, who, np.where(second, (k0[who] + 2) % nd, k0[who]), N), 0, cs)
    assert counts["merge"] > 2000 and counts["append"] > 2000 and counts["replace_nan"] > 0
    u = eng.store_usage()
    pos, cnt, feat, dis = eng.export_store()
    assert u["pool_rows"] > u["live_rows"] + 2000 and u["live_rows"] == int(cnt.sum()) == len(feat)
    zero = np.flatnonzero((pos == 0).all(1))
    assert len(zero) == 1 and cnt[zero[0]] == cs                 # grid_0_0_0, created by the last rows of cycle 2
    qs = [_queries(tok, rs, nq) for nq in (1, 8, 80)]
    before = _observe(eng, qs, monkeypatch)
    assert eng.compact_store() == (u["pool_rows"], u["live_rows"])
    u2 = eng.store_usage()
    assert u2["pool_rows"] == u2["live_rows"] == u["live_rows"] and u2["capacity"] == u["capacity"]
    after = _observe(eng, qs, monkeypatch)
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert eng.compact_store() == (u["live_rows"], u["live_rows"])
    # the store goes on as if nothing had happened: one more surprise cycle (radius 1) and one distance flush
    who = np.concatenate([rs.permutation(S)[:2000], S + np.arange(1000)])
    ks = np.concatenate([(k0[who[:2000]] + 1) % nd, rs.randint(nd, size=1000)])
    _surprise(eng, st, _cache(tok, rs, vox, who, ks, N), 1, cs)
    eng.import_cache(*c1)
    random.seed(5)
    eng.flush()
    random.seed(5)
    _dist_replay(st, c1[0], c1[1], c1[2], cs)
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), "after compaction")
    eng.close()


def _pairs_case(V, same):
    """V voxels with two stored tokens each — of one direction (same: the next accepted row merges them, the second one's
    row dies) or of two."""
    D, cs, nd = 8, 4, 4
    rs = np.random.RandomState(11)
    tok = SC.Tokens(rs, nd, D)
    vox = _voxels(rs, V)
    k0 = rs.randint(nd, size=V)
    st = {}
    for i in range(V):
        f = tok.many([k0[i], k0[i] if same else (k0[i] + 1) % nd])
        st[tuple(int(v) for v in vox[i])] = [[f[0], f[1]], [1.0, 2.0], [False, False]]
    return D, cs, nd, rs, tok, vox, k0, st


def test_dead_rows_below_the_live_count():
    """Every voxel holds rows 2i, 2i + 1 of one direction; a row of another direction is appended (a fresh row above 2 V) and
    forgetting merges the two old ones: the V dead rows are all below L = 2 V, the V fresh rows all move."""
    V = 300
    D, cs, nd, rs, tok, vox, k0, st = _pairs_case(V, True)
    eng = _engine(vox, D, cs, V)
    _import_store(eng, st, D)
    counts = _surprise(eng, st, _cache(tok, rs, vox, np.arange(V), (k0 + 1) % nd, V), 0, cs)
    assert counts["merge"] == V
    assert eng.store_usage() == dict(pool_rows=3 * V, live_rows=2 * V, capacity=eng.store_usage()["capacity"])
    before = eng.export_store()
    assert eng.compact_store() == (3 * V, 2 * V)
    cst = eng.compact_stats()
    assert (cst["compactions"], cst["rows_moved"]) == (1, V) and cst["ms"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, eng.export_store()))
    who = rs.permutation(V)
    _surprise(eng, st, _cache(tok, rs, vox, who, (k0[who] + 2) % nd, V), 1, cs)
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), "remapped rows")
    eng.close()


def test_dead_rows_above_the_live_count(monkeypatch):
    """A row of a stored direction is appended to a fresh row and merged into the old one: every dead row lies above L, nothing
    moves, the rows in use shrink."""
    monkeypatch.setenv("BSC_STORE_COMPACT", "never")
    V = 300
    D, cs, nd, rs, tok, vox, k0, st = _pairs_case(V, False)
    eng = _engine(vox, D, cs, V)
    _import_store(eng, st, D)
    counts = _surprise(eng, st, _cache(tok, rs, vox, np.arange(V), k0, V), 0, cs)
    assert counts["merge"] == V
    before = eng.export_store()
    assert eng.compact_store() == (3 * V, 2 * V)
    assert eng.compact_stats() == dict(compactions=0, rows_moved=0, ms=0.0)             # nothing had to move
    assert eng.store_usage()["pool_rows"] == 2 * V
    assert all(np.array_equal(a, b) for a, b in zip(before, eng.export_store()))
    _surprise(eng, st, _cache(tok, rs, vox, np.arange(V), (k0 + 2) % nd, V), 0, cs)
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), "after the shrink")
    eng.close()


def test_one_live_row_empty_store_and_dense_mode(monkeypatch):
    import bsc_nav_amd as B
    monkeypatch.setenv("BSC_STORE_COMPACT", "never")
    D, cs, nd, rs, tok, vox, k0, st = _pairs_case(1, True)
    eng = _engine(vox, D, cs, 1)
    assert eng.compact_store() == (0, 0) and eng.store_usage()["pool_rows"] == 0          # an empty store
    _import_store(eng, st, D)
    _surprise(eng, st, _cache(tok, rs, vox, [0], [k0[0]], 1), 0, cs)                        # all three tokens merge
    assert eng.store_usage()["live_rows"] == 1 and eng.store_usage()["pool_rows"] == 3
    assert eng.compact_store() == (3, 1)
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), "one live row")
    eng.close()
    dense = _engine(vox, D, cs, 1, mode="mean")
    with pytest.raises(B._lib.BscError, match="status -4"):
        dense.compact_store()
    with pytest.raises(B._lib.BscError, match="status -4"):
        dense.store_usage()
    dense.close()


@pytest.mark.parametrize("switch", ["auto", "never"])
def test_compaction_before_growing(monkeypatch, switch):
    """400 stored rows, capacity 700, 200 cache rows: the first cycle fits (600) and leaves 200 dead rows; the second would
    need 800 — reclaiming the dead rows makes room (auto), otherwise the pool doubles (never)."""
    monkeypatch.setenv("BSC_STORE_COMPACT", switch)
    V = 200
    D, cs, nd, rs, tok, vox, k0, st = _pairs_case(V, True)
    eng = _engine(vox, D, cs, V, token_capacity=700)
    _import_store(eng, st, D)
    _surprise(eng, st, _cache(tok, rs, vox, np.arange(V), (k0 + 1) % nd, V), 0, cs)
    assert eng.store_usage() == dict(pool_rows=600, live_rows=400, capacity=700)
    who = rs.permutation(V)
    _surprise(eng, st, _cache(tok, rs, vox, who, (k0[who] + 2) % nd, V), 0, cs)
    u = eng.store_usage()
    assert u["live_rows"] == 600
    assert (u["capacity"], u["pool_rows"]) == ((700, 600) if switch == "auto" else (1400, 800))
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), switch)
    # the distance flush reserves its rows the same way
    c = _cache(tok, rs, vox, np.arange(V), (k0 + 3) % nd, V)
    eng.import_cache(*c)
    random.seed(9)
    eng.flush()
    random.seed(9)
    _dist_replay(st, c[0], c[1], c[2], cs)
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), switch + ", distance flush")
    assert eng.store_usage()["capacity"] == 1400         # 800 rows would not fit into 700: nothing dead is left to reclaim
    eng.close()


@pytest.mark.parametrize("switch", ["auto", "never"])
def test_compaction_after_a_surprise_flush(monkeypatch, switch):
    """V one-token groups; every cycle appends a row of the stored direction to each and merges it away: V more dead rows per
    cycle.  After two cycles 3 V > 2 V rows are in use under never; auto has compacted."""
    monkeypatch.setenv("BSC_STORE_COMPACT", switch)
    V = 300
    D, cs, nd, rs, tok, vox, k0, st = _pairs_case(V, False)
    for g in st.values():
        g[0], g[1], g[2] = g[0][:1], g[1][:1], g[2][:1]
    eng = _engine(vox, D, cs, V)
    _import_store(eng, st, D)
    for _ in range(2):
        who = rs.permutation(V)
        _surprise(eng, st, _cache(tok, rs, vox, who, k0[who], V), 0, cs)
    u = eng.store_usage()
    assert u["live_rows"] == V and u["pool_rows"] == (V if switch == "auto" else 3 * V)
    assert_store_matches(eng.export_store(), *R.store_to_arrays(st, D), switch)
    eng.close()
