#!/usr/bin/env python3
"""Golden vectors for the top-down map at a height cut: TrajectoryDrawer._get_rgb_2d_map (BSCAgent.py:203-234), produced by
calling the reference's own method on a small random memory (build container only).

    python tests/golden/gen_golden_topdown.py <directory of the reference>"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_clusters import import_agent  # noqa: E402

GS, NH, V, MINH, CS = 32, 24, 700, -7, 0.1
HEIGHTS = [-0.75, -0.7, 0.0, 0.31, 0.95, 1.6, 5.0]


def main():
    B = import_agent(sys.argv[1])
    B.cv2.cvtColor = lambda a, code: a[..., ::-1]           # COLOR_RGB2BGR of the stubbed cv2
    rs = np.random.RandomState(10)
    cells = rs.choice(GS * GS * NH, size=V, replace=False)  # distinct voxels, in a random id order
    pos = np.stack([cells // (GS * NH), cells // NH % GS, cells % NH], 1).astype(np.int32)
    rgb = rs.randint(1, 256, size=(V, 3)).astype(np.uint8)  # no voxel is black: a known cell is one with a colour
    drawer = object.__new__(B.TrajectoryDrawer)
    drawer.pc, drawer.rgb = pos, rgb
    drawer.memory = types.SimpleNamespace(gs=GS, cs=CS, minh=MINH)
    cuts, maps = [], []
    for h in HEIGHTS:
        cuts.append(int(np.floor((h / CS) - MINH)))
        m = np.ascontiguousarray(drawer._get_rgb_2d_map(h))
        assert m.dtype == np.uint8 and m.shape == (GS, GS, 3)
        maps.append(m)
        print("height", h, "cut", cuts[-1], "known cells", int((m.sum(-1) != 0).sum()))
    np.savez_compressed(os.path.join(HERE, "g10_topdown_slice.npz"), pos=pos, rgb=rgb, cs=np.float64(CS), minh=np.int64(MINH),
                        gs=np.int64(GS), nh=np.int64(NH), heights=np.array(HEIGHTS, np.float64), cuts=np.array(cuts, np.int64),
                        maps_bgr=np.stack(maps))


if __name__ == "__main__":
    main()
