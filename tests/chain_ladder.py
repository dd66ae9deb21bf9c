"""A scene in which every voxel's segment of an ingest call has a length chosen in advance: the "ladder" of lengths at which the rgb
chain of csrc/ingest.hip changes its path, shared by tests/test_chain_ladder.py (CPU: the scene is what it claims) and
tests/test_gpu_chain_ladder.py (the default dense path, bit for bit against the sequential oracle).

NumPy and the CPU oracle only.  With L = 2^LONG_MIN_LOG2, E = LONG_EARLY and T = 2^HOT_MIN_LOG2 read from ingest.hip, the rungs are

    1 2 3 4 5 15 16 17                         the quad chain
    L-1 L L+1  2L-1 2L 2L+1  3L-1 3L 3L+1      first one-wavefront segments, whole and ragged 64-point chunks
    E-1 E E+1  E+L-1 E+L E+L+1                 a new voxel's early part: nothing, one point, a short and a long rest
    1023 1024 1025                             a run holds at most 1024 points
    2047 2048 2049  4095 4096 4097             a k_points workgroup holds 1024 / 2048 / 4096 points (RPW 4 / 8 / 16)
    T-1 T T+1  T+511 T+512 T+513               the hot class; its last round of 8 wavefronts ends 511 / 512 / 513 points in
    T + T/2 + 1,  2T+1                         an odd hot length, and one past two whole hot units

240x320 frames (a whole number of RPW x 64 slices for RPW 4, 8 and 16), 0.5 m cells, a 32-cell grid, heights -4 to 4 m, 16x16 patches
of 8-D tokens, depths 0.1 to 10.  A call holds twelve frames:

    two "room" frames of synth.make_frames       a few hundred voxels of up to ~4000 candidate points: the short rungs
    "near" cameras 5 cm behind a cell's x = const face, at its centre, looking along +x at constant depth 0.2:
                                                 all 76,800 pixels in one voxel, one camera per hot rung; one of them twice
    an "edge" camera on a cell plane (2 voxels of ~38,400) and a "corner" camera on a cell edge (4 of ~19,200): 4095 .. T-1

in mixed order.  The voxel seen twice is seen in two frames that are not adjacent, so its points interleave with other voxels'
across frames and workgroups.  Every pixel's cell comes from the oracle's geometry; a voxel's surplus pixels (a seeded permutation,
so the survivors are spread over its frames) get depth 0.0, which the depth mask drops.  Rungs go, largest first, to voxels with
enough candidates; every other voxel gets a seeded random length of at most 300.

Four calls:  A the ladder on new voxels;  B the same cameras, the rungs dealt out again (every segment belongs to an old voxel: no
early part, the lengths from L to E included);  C three near cameras moved to new cells and the room seen from two other poses (new
and old mixed);  D B's frames again."""
import functools
import os
import re

import numpy as np

import synth
from oracle import oracle as orc
from render_scenes import _look, _pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, GS, CS, FLOOR, TOP, G, D = 240, 320, 32, 0.5, -4.0, 4.0, 16, 8
VCAP = 4000                      # 12 bits of voxel id in a run key: the length field beside it has its full 10 bits (runs of 1024)
NEAR_DEPTH = 0.2
MAX_OTHER = 300
CALLS = "ABCD"


def thresholds():
    """(L, E, T) from the #define lines of csrc/ingest.hip"""
    text = open(os.path.join(ROOT, "bsc-nav_amd", "csrc", "ingest.hip")).read()
    v = {n: int(re.search(r"^#define\s+%s\s+(\d+)\b" % n, text, flags=re.M).group(1))
         for n in ("LONG_MIN_LOG2", "LONG_EARLY", "HOT_MIN_LOG2")}
    return 1 << v["LONG_MIN_LOG2"], v["LONG_EARLY"], 1 << v["HOT_MIN_LOG2"]


def rungs(L, E, T):
    r = [1, 2, 3, 4, 5, 15, 16, 17]
    r += [m * L + d for m in (1, 2, 3) for d in (-1, 0, 1)]
    r += [E - 1, E, E + 1, E + L - 1, E + L, E + L + 1]
    r += [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
    r += [T - 1, T, T + 1, T + 511, T + 512, T + 513, T + T // 2 + 1, 2 * T + 1]
    assert len(set(r)) == len(r), "two rungs coincide: the thresholds moved, choose the ladder again"
    assert max(r) <= H * W and (T + T // 2 + 1) % 2 == 1
    return sorted(r)


def config():
    return orc.make_config(H, W, GS, CS, FLOOR, TOP, G, D, mode=1)


# ---- cameras ---------------------------------------------------------------------------------------------------------------
# (k, j, m): the camera sits in truncation cell (k, j, m) of the map axes x, y, z.  The room's walls are at x = -3 and 3, y = -4 and 4,
# its floor and ceiling at z = 0 and 3: cells with k, j, m from 1 to 4, 6, 4 hold no room point, whatever the pose.  That matters:
# a room point seen from metres away has an alpha below half an ulp of a hot voxel's weight and would leave no trace in it, whereas
# every point of a near camera (alpha ~ 0.93) moves the weight by hundreds of ulps.
NEAR_CELLS = [(1, 1, 1), (3, 2, 2), (2, 4, 1), (4, 1, 3), (1, 5, 2), (4, 3, 1), (3, 6, 3)]
NEAR_MOVED = {0: (2, 2, 4), 3: (4, 5, 2), 5: (1, 3, 4)}        # call C: cameras 0, 3 and 5 in cells no call has touched
TWICE = 4                                                      # the near camera that two frames of a call share
EDGE_CELL, CORNER_CELL = (2, 2, 1), (3, 5, 3)
# frame order of a call: n<i> near camera i, r<i> room frame i, e / c the edge / corner camera
ORDER = ["n0", "r0", "n4", "n1", "e", "n2", "r1", "n4", "n3", "c", "n5", "n6"]
ROOM_SEED = {"A": (61, 0), "B": (61, 0), "C": (62, 3), "D": (61, 0)}     # (seed, first yaw in 30 degree steps)
# the voxel seen in two frames holds a hot rung in every call
PINNED = {"A": lambda L, E, T: T + T // 2 + 1, "B": lambda L, E, T: 2 * T + 1, "C": lambda L, E, T: T + 512}
PINNED["D"] = PINNED["B"]


def _near_T(cell, on_plane=0):
    """on_plane 0: the cell's centre in y and z; 1: y on the cell's lower plane (edge); 2: y and z (corner)"""
    k, j, m = cell
    centre = (k * CS + 0.05, j * CS + (0.25 if on_plane < 1 else 0.0), m * CS + (0.25 if on_plane < 2 else 0.0))
    return _pose(centre, _look((1.0, 0.0, 0.0)))


def _raw_call(name, chain):
    """depth (F,H,W) f32 before the trimming and Ts (F,4,4) of call `name`"""
    seed, yaw = ROOM_SEED[name]
    _, room_depth, poses = synth.make_frames(seed, 2, H, W, "room", start_yaw_steps=yaw)
    F = len(ORDER)
    depth, Ts = np.empty((F, H, W), np.float32), np.empty((F, 4, 4))
    for f, tag in enumerate(ORDER):
        i = int(tag[1:]) if len(tag) > 1 else 0
        if tag[0] == "r":
            depth[f], Ts[f] = room_depth[i], chain.pc_transform(poses[i])
            continue
        depth[f] = np.float32(NEAR_DEPTH)
        if tag[0] == "n":
            Ts[f] = _near_T(NEAR_MOVED[i] if name == "C" and i in NEAR_MOVED else NEAR_CELLS[i])
        else:
            Ts[f] = _near_T(EDGE_CELL, 1) if tag == "e" else _near_T(CORNER_CELL, 2)
    return depth, Ts


def pixel_cells(cfg, depth, Ts):
    """(F*H*W,) int64 cell code (row * GS + col) * nh + stored h of every pixel that the ingest keeps, -1 of the others"""
    nh = cfg.max_h - cfg.min_h
    out = []
    for f in range(len(depth)):
        gm = orc.geometry(cfg, depth[f], None, Ts[f])
        vox, pat = gm["vox"].astype(np.int64), gm["pat"]
        keep = (gm["valid"] != 0) & (gm["in_range"] != 0) & (pat >= 0).all(1) & (pat < G).all(1)
        out.append(np.where(keep, (vox[:, 0] * GS + vox[:, 1]) * nh + (vox[:, 2] - cfg.min_h), -1))
    return np.concatenate(out)


def cell_code(cfg, row, col, h):
    """the cell code of a voxel position as export_rgb reports it: row, column, stored h"""
    return (int(row) * GS + int(col)) * (cfg.max_h - cfg.min_h) + int(h)


def _assign(name, cells, counts, ladder, pinned_cell, pinned_rung, rs):
    """cell -> length.  The rungs, largest first, go to free voxels with enough candidates: call A takes the one with the fewest
    (ties: the lowest cell), the later calls a seeded random one.  Whatever the choice, a rung finds a voxel if the best fit does:
    the voxels taken before it all had enough candidates for it."""
    cap = dict(zip(cells.tolist(), counts.tolist()))
    assert cap[pinned_cell] >= pinned_rung
    want, free = {pinned_cell: pinned_rung}, set(cap) - {pinned_cell}
    for r in sorted(ladder, reverse=True):
        if r == pinned_rung:
            continue
        ok = sorted((cap[c], c) for c in free if cap[c] >= r)
        assert ok, "call %s: no voxel with %d candidate points is left" % (name, r)
        c = ok[0][1] if name == "A" else ok[rs.randint(len(ok))][1]
        want[c] = r
        free.discard(c)
    for c in sorted(free):
        want[c] = int(rs.randint(1, min(MAX_OTHER, cap[c]) + 1))
    return want


class Call:
    """One ingest call: depth (F,H,W) f32, rgb (F,H,W,4) u8, tokens (F,G,G,D) f32, Ts (F,4,4) f64; want: cell code -> points."""

    def __init__(self, name, depth, rgb, tokens, Ts, want):
        self.name, self.depth, self.rgb, self.tokens, self.Ts, self.want = name, depth, rgb, tokens, Ts, want

    def rgb3(self):
        return np.ascontiguousarray(self.rgb[..., :3])


@functools.lru_cache(maxsize=None)
def build_scene():
    """dict(cfg, L, E, T, rungs, calls: [Call A, B, C, D]).  Built once per process; nobody writes to its arrays."""
    cfg = config()
    L, E, T = thresholds()
    ladder = rungs(L, E, T)
    chain = orc.PoseChain()
    calls = []
    for n, name in enumerate(CALLS):
        if name == "D":
            b = calls[1]
            calls.append(Call("D", b.depth, b.rgb, b.tokens, b.Ts, b.want))
            continue
        rs = np.random.RandomState(900 + n)
        depth, Ts = _raw_call(name, chain)
        code = pixel_cells(cfg, depth, Ts)
        cells, counts = np.unique(code[code >= 0], return_counts=True)
        is_room = np.repeat([tag[0] == "r" for tag in ORDER], H * W)
        assert not set(code[is_room].tolist()) & set(code[~is_room].tolist()), "a near camera's voxel holds room points"
        assert (code[~is_room] >= 0).all()
        f_twice = ORDER.index("n%d" % TWICE)
        pinned_cell = int(code[f_twice * H * W])
        assert (code[f_twice * H * W:(f_twice + 1) * H * W] == pinned_cell).all(), "a near camera sees more than one voxel"
        want = _assign(name, cells, counts, ladder, pinned_cell, PINNED[name](L, E, T), rs)
        # trim: the surplus of every voxel, chosen by a seeded permutation of its pixels, gets depth 0
        order = np.argsort(code, kind="stable")
        start = np.searchsorted(code[order], cells)
        flat = depth.reshape(-1)
        for c, s, k in zip(cells.tolist(), start.tolist(), counts.tolist()):
            px = order[s:s + k]
            flat[rs.permutation(px)[:k - want[c]]] = 0.0
        rgb = rs.randint(0, 256, size=(len(ORDER), H, W, 4)).astype(np.uint8)
        calls.append(Call(name, depth, rgb, synth.make_tokens(70 + n, len(ORDER), G, D), Ts, want))
    return dict(cfg=cfg, L=L, E=E, T=T, rungs=ladder, calls=calls)


def length_class(n, L, T):
    return 0 if n < L else (1 if n < T else 2)


# ---- what the tests compare ------------------------------------------------------------------------------------------------
EXACT = ("max_id", "pos", "rgb", "weight", "max_height", "cv_map", "cnt")


def state(m):
    """Everything the comparison looks at, of an engine or of an oracle memory (same method names)."""
    pos, rgb, w = m.export_rgb()
    mh, cv = m.export_heightmap()
    acc, cnt = m.export_dense()
    return dict(max_id=np.int64(m.counters()["max_id"]), pos=pos, rgb=rgb, weight=w, max_height=mh, cv_map=cv, cnt=cnt, acc=acc)


def compare(got, ref, label, wants=()):
    """wants: the cell -> length tables of the calls ingested so far: a mismatch names the voxel's lengths, hence its classes"""
    assert int(got["max_id"]) == int(ref["max_id"]), label
    for k in EXACT:
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k)
        if np.array_equal(a, b):
            continue
        detail = ""
        if k in ("rgb", "weight", "cnt"):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
            for v in bad[:8].tolist():
                r, c, h = (int(t) for t in ref["pos"][v])
                code = cell_code(config(), r, c, h)
                detail += "\n  voxel %d at %s, lengths per call %s: got %s, expected %s" % (
                    v, (r, c, h), [w.get(code, 0) for w in wants], a[v].tolist(), b[v].tolist())
            detail = " %d voxels differ:%s" % (len(bad), detail)
        raise AssertionError("%s: %s differs from the oracle.%s" % (label, k, detail))
    c = np.maximum(ref["cnt"], 1)[:, None].astype(np.float64)
    np.testing.assert_allclose(got["acc"] / c, ref["acc"] / c, rtol=1e-3, atol=1e-3, err_msg=label)
