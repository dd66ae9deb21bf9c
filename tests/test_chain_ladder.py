"""The ladder scene of tests/chain_ladder.py is what it claims, decided on the CPU: the sequential oracle ingests the four calls and
every voxel's point count of a call is the one the scene assigned.  This is what keeps tests/test_gpu_chain_ladder.py from passing
on a scene that missed its rungs: no rung may be left out, in call A on new voxels and in call B on old ones."""
import numpy as np
import pytest

import chain_ladder as cl
from oracle import oracle as orc


@pytest.fixture(scope="module")
def ingested():
    """The scene and, per call: cell -> points added by the call, and the set of cells that existed before the call."""
    sc = cl.build_scene()
    cfg = sc["cfg"]
    nh = cfg.max_h - cfg.min_h
    om = orc.OracleMemory(cfg, voxel_capacity=cl.VCAP)
    before, per_call = np.zeros(0, np.int64), []
    for call in sc["calls"]:
        for f in range(len(call.depth)):
            gm = orc.geometry(cfg, call.depth[f], None, call.Ts[f])
            om.ingest_frame(call.depth[f], call.rgb[f], None, call.Ts[f], call.tokens[f], np.exp(-gm["r2"] / 1.2))
        cnt = om.export_dense()[1].astype(np.int64)
        pos = om.export_rgb()[0].astype(np.int64)
        code = (pos[:, 0] * cl.GS + pos[:, 1]) * nh + pos[:, 2]
        added = cnt - np.concatenate([before, np.zeros(len(cnt) - len(before), np.int64)])
        got = {int(c): int(a) for c, a in zip(code, added) if a}
        old = set(code[:len(before)].tolist())
        per_call.append((got, old))
        before = cnt
    assert len(before) <= cl.VCAP
    return sc, per_call


def test_every_voxel_gets_the_assigned_number_of_points(ingested):
    sc, per_call = ingested
    for call, (got, _) in zip(sc["calls"], per_call):
        assert got == call.want, call.name                   # per cell, hence also as a multiset
        assert set(got.values()) >= set(sc["rungs"])


def test_call_a_has_every_rung_on_a_new_voxel_and_call_b_on_an_old_one(ingested, capsys):
    sc, per_call = ingested
    (got_a, old_a), (got_b, old_b) = per_call[0], per_call[1]
    assert not old_a
    new_a = sorted(n for c, n in got_a.items() if c not in old_a)
    on_old_b = sorted(n for c, n in got_b.items() if c in old_b)
    with capsys.disabled():                                  # the list belongs to the run's output, passed or not
        print("\ncall A, rungs on new voxels:", [r for r in sc["rungs"] if r in new_a])
        print("call B, rungs on old voxels:", [r for r in sc["rungs"] if r in on_old_b])
    for r in sc["rungs"]:
        assert r in new_a, "rung %d is missing from call A" % r
        assert r in on_old_b, "rung %d is on no old voxel in call B" % r
    assert set(got_b) <= old_b                               # B creates no voxel: no segment of it has an early part
    # the rungs moved: B is not A again
    by_rung_a, by_rung_b = {n: c for c, n in got_a.items()}, {n: c for c, n in got_b.items()}
    assert sum(by_rung_a[r] != by_rung_b[r] for r in sc["rungs"]) > len(sc["rungs"]) // 2


def test_call_c_mixes_new_and_old_voxels_in_every_class(ingested):
    sc, per_call = ingested
    got, old = per_call[2]
    seen = {(cl.length_class(n, sc["L"], sc["T"]), c in old) for c, n in got.items()}
    print("call C (class, old):", sorted(seen))
    assert seen == {(k, o) for k in (0, 1, 2) for o in (False, True)}
    got_d, old_d = per_call[3]
    assert got_d == per_call[1][0] and set(got_d) <= old_d   # D: B's frames again


def test_a_hot_voxel_is_seen_in_two_frames_that_are_not_adjacent():
    sc = cl.build_scene()
    f = [i for i, tag in enumerate(cl.ORDER) if tag == "n%d" % cl.TWICE]
    assert len(f) == 2 and f[1] - f[0] > 1
    for call in sc["calls"]:
        kept = [(call.depth[i] > 0).sum() for i in f]
        assert min(kept) > 1000 and sum(kept) >= sc["T"]      # both frames carry a good part of one hot segment


def _oracle_after_call_a(call, cfg):
    om = orc.OracleMemory(cfg, voxel_capacity=cl.VCAP)
    for f in range(len(call.depth)):
        gm = orc.geometry(cfg, call.depth[f], None, call.Ts[f])
        om.ingest_frame(call.depth[f], call.rgb[f], None, call.Ts[f], call.tokens[f], np.exp(-gm["r2"] / 1.2))
    return cl.state(om)


@pytest.mark.parametrize("which", ["last point of a hot segment", "point LONG_EARLY of a new voxel"])
def test_the_comparison_sees_a_single_dropped_point(which):
    """What a chain that loses one point at a class boundary would leave behind, made on the CPU: the oracle ingests call A once
    more without the last point of the T+512 segment, or without point E (counted from 0) of the E+L segment.  The comparison that
    tests/test_gpu_chain_ladder.py uses (chain_ladder.compare) must refuse that state: a weight of a few 10^4 still resolves one
    point (alpha ~ 0.9 against an ulp of 2^-9), which the tolerances of the large-scene tests do not."""
    sc = cl.build_scene()
    cfg, call = sc["cfg"], sc["calls"][0]
    rung, nth = (sc["T"] + 512, sc["T"] + 511) if which.startswith("last") else (sc["E"] + sc["L"], sc["E"])
    cell = {n: c for c, n in call.want.items()}[rung]
    px = np.nonzero(cl.pixel_cells(cfg, call.depth, call.Ts) == cell)[0]
    assert len(px) == rung
    ref = _oracle_after_call_a(call, cfg)
    depth = call.depth.copy()
    depth.reshape(-1)[px[nth]] = 0.0
    bad = _oracle_after_call_a(cl.Call("A", depth, call.rgb, call.tokens, call.Ts, call.want), cfg)
    bad["cnt"] = ref["cnt"]                                # the counts come from the dense reduce, not from the chain
    cl.compare(ref, ref, "the reference against itself", [call.want])
    with pytest.raises(AssertionError, match=r"(rgb|weight) differs from the oracle. 1 voxels differ:\s+voxel \d+ at .* lengths per call \[%d\]" % rung):
        cl.compare(bad, ref, which, [call.want])


def test_the_three_channel_form_is_the_same_scene():
    call = cl.build_scene()["calls"][0]
    assert call.rgb.shape[-1] == 4 and np.array_equal(call.rgb3(), call.rgb[..., :3]) and call.rgb3().flags.c_contiguous
