"""Generated inputs that drive bsc_flush_surprise (csrc/surprise.hip) through every schedule path, radius 0-3 and the edge
tokens, shared by tests/test_surprise_cases.py (CPU: the replay's margins and paths) and tests/test_gpu_surprise_cases.py.

NumPy only.  A case is a dict in the layout of the g9_surprise_direct fixtures (what test_gpu_surprise._direct_engine
reads): gs, cell, floor_height, map_height (cell 1.0 and floor 0, so nh == map_height), D, iter_size, cache_size,
voxel_capacity, vox_pos for import_rgb, prior_* for import_store in HDF5 name order (surprise_replay.name_key), cache_* for
import_cache (all iter_size rows, the zero tail at [0,0,0] included), radius, sthr, bthr.

Tokens follow tests/golden/gen_golden_surprise.py: a fixed direction scaled by U(0.5, 2) plus small noise.  The directions
are built so that no decision of the policy sits near a threshold (the replay's three margins stay >= 1e-4):

    d_k = normalize(q_k + a_k z),   q_0 .. q_{n-1}, z orthonormal,   a_k = 0.2 + 0.4 k / (n - 1)
    cos(d_j, d_k) = f(a_j) f(a_k),  f(a) = a / sqrt(1 + a^2)         (0.038 .. 0.265 for j != k)

Two tokens of one direction have a cosine of 1 - O(noise^2) (boring: > 0.95, not surprising: 1 - cos < 0.5), two tokens of
different directions at most 0.27.  The 1 - cos values of a replacement in a group whose slots hold DISTINCT directions are
f(a_new) f(a_slot): strictly ordered by a_slot, the two smallest at least f(0.2) (f(0.6) - f(0.6 - 0.4 / (n - 1))) apart
(6e-4 at n = 80), which the noise (relative size `rel`) stays well below.  Every group of a case therefore holds distinct
directions, before and after: forgetting merges two tokens of one direction.
"""
import numpy as np

import surprise_replay as R

STHR, BTHR = 0.5, 0.95
MARGIN = 1e-4
# the three constants of surprise_flush's choice of level table (csrc/surprise.hip)
TAB16_TASKS = 65535      # fewer tasks: levels fit u16
SURP_TAB16 = 81920       # task voxels the u16 table in LDS holds
SURP_TAB32 = 40960       # ... the u32 table in LDS; beyond: a table in global memory
SURP_TASK_LDS = 49152


def lds_bytes(radius, cache_size, D):
    return 4 * (2 * ((2 * radius + 1) ** 3 - 1) * cache_size + D)


class Tokens:
    def __init__(self, rs, nd, D, rel=1e-3):
        assert nd + 1 <= D and D % 4 == 0, (nd, D)
        q, _ = np.linalg.qr(rs.standard_normal((D, nd + 1)))
        a = 0.2 + 0.4 * np.arange(nd) / max(nd - 1, 1)
        d = q[:, :nd].T + a[:, None] * q[:, nd][None, :]
        self.dirs = d / np.linalg.norm(d, axis=1, keepdims=True)
        self.rs, self.nd, self.D, self.rel = rs, nd, D, rel

    def many(self, ks):
        """(n, D) f32 tokens of the directions ks; k < 0: a zero token."""
        ks = np.asarray(ks, np.int64).reshape(-1)
        n = len(ks)
        scale = self.rs.uniform(0.5, 2.0, (n, 1))
        noise = self.rel * self.rs.standard_normal((n, self.D)) / np.sqrt(self.D)
        t = (self.dirs[np.maximum(ks, 0)] + noise) * scale
        t[ks < 0] = 0.0
        return t.astype(np.float32)


class Builder:
    """Collects voxels, prior groups (lists of directions; -1 a zero token) and cache rows."""

    def __init__(self, seed, gs, nh, D, cs, nd, radius, sthr=STHR, bthr=BTHR, rel=1e-3):
        self.rs = np.random.RandomState(seed)
        self.tok = Tokens(self.rs, nd, D, rel)
        self.gs, self.nh, self.D, self.cs, self.nd, self.radius, self.sthr, self.bthr = gs, nh, D, cs, nd, radius, sthr, bthr
        self.vox, self.prior, self.rows_p, self.rows_k = [], {}, [], []

    def voxel(self, p, prior=None):
        p = tuple(int(v) for v in p)
        assert 0 <= p[0] < self.gs and 0 <= p[1] < self.gs and 0 <= p[2] < self.nh, p
        if p not in self.vox:
            self.vox.append(p)
        if prior is not None:
            assert len(prior) <= self.cs
            self.prior[p] = list(prior)
        return p

    def row(self, p, k, times=1):
        for _ in range(times):
            self.rows_p.append(tuple(p)); self.rows_k.append(int(k))

    def finish(self, name, tail, **extra):
        """tail zero rows at [0,0,0] follow the real rows (memory_2.py: the unused part of the cache is flushed too)."""
        rs, D = self.rs, self.D
        keys = sorted((p for p in self.prior if self.prior[p]), key=R.name_key)
        ks = [k for p in keys for k in self.prior[p]]
        n = len(self.rows_p)
        cf = np.zeros((n + tail, D), np.float32)
        cp = np.zeros((n + tail, 3), np.int32)
        cd = np.zeros(n + tail, np.float32)
        if n:
            cf[:n], cp[:n] = self.tok.many(self.rows_k), np.array(self.rows_p, np.int32)
            cd[:n] = rs.uniform(0.5, 5.0, n).astype(np.float32)
        vox = [p for p in self.vox]
        assert len(set(vox)) == len(vox)
        used = set(self.rows_p) | set(keys)
        assert used <= set(vox) | {(0, 0, 0)}, "a row or a prior group without a voxel"
        z = dict(name=name, gs=self.gs, cell=1.0, floor_height=0.0, map_height=float(self.nh), nh=self.nh, D=D,
                 iter_size=n + tail, cache_size=self.cs, voxel_capacity=max(len(vox), self.gs * self.gs), n_real=n,
                 vox_pos=np.array(vox, np.int32).reshape(-1, 3),
                 prior_pos=np.array(keys, np.int32).reshape(-1, 3),
                 prior_cnt=np.array([len(self.prior[p]) for p in keys], np.int32),
                 prior_feat=self.tok.many(ks) if ks else np.zeros((0, D), np.float32),
                 prior_dis=rs.uniform(0.5, 5.0, len(ks)).astype(np.float32),
                 cache_pos=cp, cache_feat=cf, cache_dis=cd, radius=self.radius, sthr=self.sthr, bthr=self.bthr)
        z.update(extra)
        return z


def cheb(p, q):
    return max(abs(int(a) - int(b)) for a, b in zip(p, q))


# ---- a small mixed scene: a dense block, isolated voxels, runs of rows ----------------------------------------------------------
def _mixed(name, seed, D, cs, nd, radius=1, sthr=STHR, bthr=BTHR, rows=260, tail=30, rel=1e-3, max_per_voxel=None, **extra):
    """A 3 x 3 x 2 block of mutually close voxels (each with a few directions of its own, most with a prior group) and four
    voxels with no other voxel within `radius` (their rows have no neighbour token: surprise = +inf); [0,0,0] has no
    neighbour either.  max_per_voxel: at most that many rows per voxel (so that no group fills up)."""
    far = 2 * radius + 2
    gs, nh = 4 + 4 * far, 3 + 2 * far
    b = Builder(seed, gs, nh, D, cs, nd, radius, sthr, bthr, rel)
    rs = b.rs
    o = far
    block = [b.voxel((o + r, o + c, o + h)) for r in range(3) for c in range(3) for h in range(2)]
    lone = [b.voxel(p) for p in ((o + 2 + far, o, o), (o, o + 2 + far, o + 1), (o + 2 + far, o + 2 + far, nh - 1),
                                 (gs - 1, o, nh - 1))]
    for p in lone:
        assert all(cheb(p, q) > radius for q in block + [(0, 0, 0)] + [x for x in lone if x != p]), p
    own = {}
    for p in block + lone:
        own[p] = rs.choice(min(nd, 6), min(nd, 3), replace=False)
        if rs.rand() < 0.7:
            b.prior[p] = [int(k) for k in own[p][:rs.randint(1, min(cs, len(own[p])) + 1)]]
    every = block + lone
    left = {p: (max_per_voxel if max_per_voxel else 1 << 30) for p in every}
    n = 0
    while n < rows and any(left.values()):
        p = every[rs.randint(len(every))] if rs.rand() < 0.75 else lone[rs.randint(len(lone))]
        for _ in range(min(int(rs.choice([1, 1, 2, 3])), left[p])):
            b.row(p, rs.choice(own[p]) if rs.rand() < 0.35 else rs.randint(nd))
            left[p] -= 1
            n += 1
    return b.finish(name, tail, **extra)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def radius0():
    """K = 1: no row ever has a neighbour token, every row after the creating one is +inf-accepted."""
    b = Builder(101, 8, 4, 32, 6, 10, 0)
    rs = b.rs
    vox = [b.voxel(p) for p in [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1), (5, 5, 0), (7, 7, 3), (0, 7, 0), (7, 0, 3), (3, 4, 2),
                                (3, 4, 3), (4, 4, 2), (6, 2, 1)]]
    for p in vox[:8]:
        b.prior[p] = [int(k) for k in rs.choice(10, rs.randint(1, 7), replace=False)]
    for _ in range(330):
        b.row(vox[rs.randint(len(vox))], rs.randint(10), times=int(rs.choice([1, 1, 2])))
    return b.finish("radius0", 25)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def radius3():
    """K = 343 on a sparse 16 x 16 x 10 grid: clusters on every kind of border, voxels with nothing within 3, the real voxel
    [0,0,0] with a zero tail, and 'wrap traps': a border voxel whose rows use a direction that no true neighbour holds but
    the cell a missing clip would reach (row gs -> row 0 of the next index, column / height likewise) does."""
    gs, nh, r = 16, 10, 3
    b = Builder(102, gs, nh, 32, 4, 14, r)
    rs = b.rs
    clusters = [[(15, 15, 9), (13, 14, 8), (15, 12, 9)],            # a corner other than [0,0,0]
                [(0, 0, 0), (2, 1, 0), (0, 3, 2)],                   # the real voxel [0,0,0]
                [(15, 0, 4), (13, 0, 5), (15, 2, 2)],                # an edge
                [(8, 8, 0), (8, 10, 2), (6, 9, 0)],                  # the face h = 0
                [(4, 4, 9), (5, 2, 9), (4, 6, 7)]]                   # the face h = nh - 1
    # (border voxel, the cell reached when the clip of one coordinate is missing, the direction only these two hold)
    traps = [((15, 6, 5), (0, 6, 5), 9), ((6, 15, 5), (7, 0, 5), 10), ((10, 7, 9), (10, 8, 0), 11),
             ((9, 0, 6), (8, 15, 6), 12), ((12, 11, 0), (12, 10, 9), 13)]
    for cl in clusters:
        for p in cl:
            b.voxel(p)
            if rs.rand() < 0.7 and p != (0, 0, 0):
                b.prior[p] = [int(k) for k in rs.choice(9, rs.randint(1, 4), replace=False)]
    for x, t, k in traps:
        b.voxel(x, [int(rs.randint(9))])
        b.voxel(t, [k])
    lone = []                                                        # three voxels with nothing within 3
    for p in ((a, c, h) for a in range(gs) for c in range(gs) for h in range(nh)):
        if len(lone) < 3 and all(cheb(p, q) > r for q in b.vox):
            lone.append(b.voxel(p, [int(k) for k in rs.choice(9, 2, replace=False)]))
    assert len(lone) == 3
    allv = list(b.vox)
    for x, t, k in traps:
        assert cheb(x, t) > r
        assert all(k not in b.prior.get(q, []) for q in allv if q != x and cheb(x, q) <= r)
    pool = [p for cl in clusters for p in cl if p != (0, 0, 0)] + lone
    seq = []
    for _ in range(260):
        seq.append((pool[rs.randint(len(pool))], int(rs.randint(9)), int(rs.choice([1, 1, 2]))))
    for x, t, k in traps:                    # the trap direction at the border voxel: appended (twice: the second merges)
        seq.insert(rs.randint(len(seq)), (x, k, 2))
    for p, k, times in seq:
        b.row(p, k, times)
    return b.finish("radius3", 40, lone=lone)


# ---- 3 / 4 ---------------------------------------------------------------------------------------------------------------------
def _lds_full(name, seed, radius, D, cs):
    """The centre of a (2r+1)^3 block whose other voxels all hold full groups: nrow is filled to K1 * cache_size entries, the
    LDS request is the largest the argument check lets through.  One direction ('rare') sits in a single token of a corner
    group; 'novel' directions sit in no prior group."""
    w = 2 * radius + 1
    nd = cs + 6
    b = Builder(seed, w + 13, w + 2, D, cs, nd, radius, rel=2e-4)
    rs = b.rs
    common, rare, novel = cs + 2, cs + 2, [cs + 3, cs + 4, cs + 5]
    block = [(1 + r, 1 + c, 1 + h) for r in range(w) for c in range(w) for h in range(w)]
    centre = (1 + radius,) * 3
    for p in block:
        b.voxel(p)
        if p != centre:
            b.prior[p] = [int(k) for k in rs.choice(common, cs, replace=False)]
    b.prior[block[-1]][cs // 2] = rare
    b.prior[centre] = [int(k) for k in rs.choice(common, cs - 2, replace=False)]
    far = b.voxel((w + 12, w + 12, w + 1), [0, 1])
    b.row(far, 2)
    for k in [novel[0], 3, rare, novel[1], novel[0], 5, novel[2], rare, novel[1], 7, novel[2]]:
        b.row(centre, k)
    b.row(far, 0)
    for p in (block[0], block[-1], block[len(block) // 3], (1 + radius, 1 + radius, 1)):
        b.row(p, novel[0], 2)
        b.row(p, 1)
    b.row(centre, novel[0])
    z = b.finish(name, 12)
    assert lds_bytes(radius, cs, D) <= SURP_TASK_LDS < lds_bytes(radius, cs + 1, D)
    return z


def lds_r3():
    return _lds_full("lds_r3_d1024_c16", 103, 3, 1024, 16)


def lds_r2():
    return _lds_full("lds_r2_d768_c46", 104, 2, 768, 46)


def refused_r3():
    z = _mixed("refused_r3_d1024_c17", 105, 1024, 17, 24, rows=120, refused_radius=3)
    assert lds_bytes(3, 17, 1024) > SURP_TASK_LDS >= lds_bytes(1, 17, 1024)
    return z


def refused_r2():
    z = _mixed("refused_r2_d768_c47", 106, 768, 47, 24, rows=120, refused_radius=2)
    assert lds_bytes(2, 47, 768) > SURP_TASK_LDS >= lds_bytes(1, 47, 768)
    return z


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def cache64():
    """cache_size 64, 80 directions: a group that grows to 64 tokens (a merge at 64: full masks), then replaces — a direction
    absent from the group lands on the slot with the largest a_k, which the ascending order puts in slot 63."""
    b = Builder(107, 10, 6, 96, 64, 80, 1, rel=1e-4)
    rs = b.rs
    P = b.voxel((4, 4, 3), list(range(60)))
    Q = b.voxel((4, 5, 3), [70, 71])
    S = b.voxel((8, 8, 1), list(range(10, 40)))
    for k in (60, 61, 62):
        b.row(P, k)                  # 63 tokens
    b.row(P, 5)                      # 64, merged with slot 5 -> 63
    b.row(P, 63)                     # 64 again (the token of direction 5 moved: slots are compacted)
    b.row(P, 70)                     # Q holds it: rejected
    for k in range(64, 70):
        b.row(P, k)                  # each replaces the slot of the largest a_k
    b.row(Q, 3)
    for k in rs.permutation(80)[:50]:
        b.row(P, int(k), times=int(rs.choice([1, 2])))
    for k in rs.permutation(80):
        b.row(S, int(k))
        if rs.rand() < 0.3:
            b.row(P, int(rs.randint(80)))
    return b.finish("cache64", 20)


def cache1():
    return _mixed("cache1", 108, 16, 1, 6)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def dim4():
    return _mixed("dim4", 109, 4, 2, 3)


def dim520():
    return _mixed("dim520", 110, 520, 5, 12)


def dim2048():
    return _mixed("dim2048", 111, 2048, 5, 12, rows=200)


def radius2_small():
    return _mixed("radius2_small", 112, 32, 4, 10, radius=2)


def radius1_small():
    return _mixed("radius1_small", 113, 32, 4, 10, radius=1)


# ---- 7 / 8 ---------------------------------------------------------------------------------------------------------------------
def _big(name, seed, gs, nh, n_vox, n_rows, tail):
    """Rows over n_vox voxels of a dense grid, consecutive rows never at one voxel (every row its own task): a permutation
    of all voxels, repeated.  The direction follows the 4 x 4 x 4 cell of the voxel most of the time."""
    D, cs, nd = 16, 4, 12
    rs = np.random.RandomState(seed)
    tok = Tokens(rs, nd, D)
    cells = 1 + rs.choice(gs * gs * nh - 1, n_vox, replace=False)       # not cell 0
    vox = np.stack([cells // (gs * nh), (cells // nh) % gs, cells % nh], 1).astype(np.int32)
    base = (vox[:, 0] // 4 + 3 * (vox[:, 1] // 4) + 5 * (vox[:, 2] // 4)) % nd
    order = []
    while sum(len(o) for o in order) < n_rows:
        p = rs.permutation(n_vox)
        if order and order[-1][-1] == p[0]:
            p = p[::-1]
        order.append(p)
    idx = np.concatenate(order)[:n_rows]
    k = np.where(rs.rand(n_rows) < 0.7, base[idx], rs.randint(nd, size=n_rows))
    has = rs.rand(n_vox) < 0.3
    pk = np.where(rs.rand(n_vox) < 0.6, base, rs.randint(nd, size=n_vox))[has]
    ppos = vox[has]
    o = np.array(sorted(range(len(ppos)), key=lambda i: R.name_key(ppos[i])), np.int64)
    cf = np.zeros((n_rows + tail, D), np.float32)
    cp = np.zeros((n_rows + tail, 3), np.int32)
    cd = np.zeros(n_rows + tail, np.float32)
    cf[:n_rows], cp[:n_rows], cd[:n_rows] = tok.many(k), vox[idx], rs.uniform(0.5, 5.0, n_rows).astype(np.float32)
    return dict(name=name, gs=gs, cell=1.0, floor_height=0.0, map_height=float(nh), nh=nh, D=D, iter_size=n_rows + tail,
                cache_size=cs, voxel_capacity=n_vox, n_real=n_rows, vox_pos=vox, prior_pos=ppos[o],
                prior_cnt=np.ones(len(o), np.int32), prior_feat=tok.many(pk[o]),
                prior_dis=rs.uniform(0.5, 5.0, len(o)).astype(np.float32), cache_pos=cp, cache_feat=cf, cache_dis=cd,
                radius=1, sthr=STHR, bthr=BTHR)


def table_u32():
    """n_tasks >= 65535 with n_u <= SURP_TAB32: the u32 level table in LDS."""
    return _big("table_u32", 114, 64, 8, 20000, 69000, 1000)


def table_global():
    """n_u > SURP_TAB16: the level table in global memory."""
    return _big("table_global", 115, 64, 32, 90000, 99000, 1000)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def deep():
    """A, B adjacent and visited alternately, C, D far away doing the same: every row is a task, every task depends on the
    one two rows earlier, every level holds two tasks (one workgroup each)."""
    b = Builder(116, 24, 6, 32, 4, 8, 1)
    rs = b.rs
    A, B_, C, D_ = b.voxel((3, 3, 2), [0]), b.voxel((3, 4, 2), [1]), b.voxel((20, 20, 4)), b.voxel((20, 19, 3), [2, 3])
    for _ in range(1500):
        for p in (A, C, B_, D_):
            b.row(p, rs.randint(8))
    return b.finish("deep", 0, pairs=[(A, B_), (C, D_)])


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def long_task():
    """One voxel V receives 700 consecutive rows (phase B: two full chunks of 256 and one of 188; phase C: eleven ballots of
    64).  Its only neighbour W holds eight directions (rows of those are rejected).  The first 330 rows use six other
    directions with cache_size 8: append + merge again and again; the rest twelve: the group fills up, then replaces."""
    b = Builder(117, 12, 6, 48, 8, 20, 1)
    rs = b.rs
    V, W = b.voxel((5, 5, 2), [8]), b.voxel((5, 6, 2), list(range(8)))
    X = b.voxel((10, 10, 5))
    for k in (0, 9, 0, 3, 10):
        b.row(X, k)
    b.row(W, 4, 2)
    for i in range(700):
        acc = rs.randint(8, 14) if i < 330 else rs.randint(8, 20)
        b.row(V, rs.randint(8) if rs.rand() < 0.45 else acc)
    b.row(X, 11)
    b.row(W, 9, 2)
    b.row(X, 0)
    return b.finish("long_task", 17, long_voxel=V, rows_elsewhere=11)


# ---- 11 -----------------------------------------------------------------------------------------------------------------------
def zeros():
    """Zero tokens (direction -1) as cache rows, in neighbour groups and in slots of a full group; every voxel below has no
    other voxel within 1 unless it says so."""
    b = Builder(118, 14, 6, 16, 4, 10, 1)
    # (a) zero rows at a voxel without neighbours, group not full: +inf -> appended (NaN slots), then filled and replaced
    Za = b.voxel((2, 2, 2), [0, 1])
    b.row(Za, -1, 2)
    for k in (2, 3, 4, 2):
        b.row(Za, k)
    # (b) runs of zero rows into a full group without edges, a non-zero accepted row between them, one 64-row ballot
    Zb = b.voxel((2, 6, 2), [0, 1, 2, 3])
    b.row(Zb, -1, 3)
    b.row(Zb, 5)
    b.row(Zb, -1, 4)
    #     the same with an edge in the group (slots 1 and 2 hold one direction): the shortcut must not fire
    Zc = b.voxel((2, 10, 2), [0, 1, 1, 3])
    b.row(Zc, -1, 3)
    b.row(Zc, 5)
    b.row(Zc, -1, 4)
    #     and a run that crosses a ballot boundary (70 zero rows) into a full group without edges, then a non-zero row
    Ze = b.voxel((10, 2, 4), [4, 5, 6, 7])
    b.row(Ze, 1)
    b.row(Ze, -1, 70)
    b.row(Ze, 2)
    b.row(Ze, -1, 2)
    # (c) a zero token inside a neighbour group: every row next to it is NaN-rejected
    N1, M = b.voxel((6, 2, 1), [0, -1]), b.voxel((6, 3, 1), [1])
    for k in (2, -1, 1, 3):
        b.row(M, k)
    b.row(N1, 4)                 # M's tokens are fine: accepted
    # (d) zero tokens in slots 1 and 3 of a full group: a non-zero row replaces the first NaN slot first
    Zd = b.voxel((6, 7, 3), [0, -1, 1, -1])
    b.row(Zd, 5)
    b.row(Za, 6)
    b.row(Zd, 6)
    b.row(Zd, 0)
    return b.finish("zeros", 9)


# ---- 12 -----------------------------------------------------------------------------------------------------------------------
def sthr_pinf():
    return _mixed("sthr_pinf", 119, 32, 4, 10, sthr=np.inf)


def sthr_ninf():
    return _mixed("sthr_ninf", 119, 32, 4, 10, sthr=-np.inf)


def bthr_pinf():
    """No merge ever, so a group may collect several tokens of one direction: cache_size 10 and at most 6 rows per voxel
    keep every group short of full (a replacement among equal directions would have no argmin margin)."""
    return _mixed("bthr_pinf", 119, 32, 10, 10, bthr=np.inf, max_per_voxel=6)


CASES = {f.__name__: f for f in (radius0, radius3, lds_r3, lds_r2, refused_r3, refused_r2, cache64, cache1, dim4, dim520,
                                 dim2048, radius1_small, radius2_small, table_u32, table_global, deep, long_task, zeros,
                                 sthr_pinf, sthr_ninf, bthr_pinf)}
LOCALIZE = {"radius0": 0, "radius1_small": 1, "radius2_small": 2, "radius3": 3}      # one small case per radius

_made, _replayed = {}, {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def schedule(z):
    """(n_tasks, n_u, n_levels) as surprise_flush plans them: a task is a run of consecutive rows at one voxel, n_u the
    distinct voxels, a task's level 1 + the largest level of the last task at any voxel within the radius."""
    pos, r = z["cache_pos"], int(z["radius"])
    head = np.ones(len(pos), bool)
    head[1:] = np.any(pos[1:] != pos[:-1], axis=1)
    tasks = [tuple(int(v) for v in p) for p in pos[head]]
    offs = [(a, b, c) for a in range(-r, r + 1) for b in range(-r, r + 1) for c in range(-r, r + 1)]
    last, depth = {}, 0
    for p in tasks:
        lv = 1 + max(last.get((p[0] + a, p[1] + b, p[2] + c), 0) for a, b, c in offs)
        last[p] = lv
        depth = max(depth, lv)
    return len(tasks), len(last), depth


def replayed(name):
    """The replay of the case and of a second flush over iter_size zero rows, once per process:
    dict(counts, margins, store, counts2, store2); store* = (pos, cnt, feat, dis, merged) in name order."""
    if name not in _replayed:
        z = case(name)
        D, n = int(z["D"]), int(z["iter_size"])
        st = R.store_from_arrays(z["prior_pos"], z["prior_cnt"], z["prior_feat"], z["prior_dis"])
        args = (int(z["radius"]), float(z["sthr"]), float(z["bthr"]), int(z["cache_size"]))
        counts, margins = R.replay(st, z["cache_pos"], z["cache_feat"], z["cache_dis"], *args)
        store = R.store_to_arrays(st, D)
        counts2, margins2 = R.replay(st, np.zeros((n, 3), np.int32), np.zeros((n, D), np.float32), np.zeros(n, np.float32), *args)
        store2 = R.store_to_arrays(st, D)
        margins = {k: min(margins[k], margins2[k]) for k in margins}
        _replayed[name] = dict(counts=counts, margins=margins, store=store, counts2=counts2, store2=store2)
    return _replayed[name]
