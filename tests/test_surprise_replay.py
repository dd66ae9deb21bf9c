"""CPU checks of the surprise-policy fixtures (g9_*) and of the test-side replay (tests/surprise_replay.py)."""
import numpy as np
import pytest

import golden_util as gu
import surprise_replay as R

DIRECT = ["g9_surprise_direct_c10", "g9_surprise_direct_c4"]


def _cases():
    for name in DIRECT:
        for r in (1, 2):
            yield name, r
    yield "g9_surprise_e2e", 1


def _prior(z):
    if "prior_feat" in z:
        return R.store_from_arrays(z["prior_pos"], z["prior_cnt"], z["prior_feat"], z["prior_dis"])
    return None


@pytest.mark.parametrize("name,radius", [c for c in _cases() if c[0] in DIRECT])
def test_replay_reproduces_direct_fixture(name, radius):
    z = gu.load(name)
    st = _prior(z)
    counts, margins = R.replay(st, z["cache_pos"], z["cache_feat"], z["cache_dis"], radius, float(z["sthr"]), float(z["bthr"]),
                               int(z["cache_size"]))
    pos, cnt, feat, dis, merged = R.store_to_arrays(st, int(z["D"]))
    p = f"r{radius}_"
    assert np.array_equal(pos, z[p + "pos"]) and np.array_equal(cnt, z[p + "cnt"])
    assert np.array_equal(feat, z[p + "feat"]) and np.array_equal(dis, z[p + "dis"]) and np.array_equal(merged, z[p + "merged"])
    assert [counts[k] for k in R.PATHS] == list(z[p + "counts"])
    assert np.allclose([margins["surprise"], margins["boring"], margins["argmin"]], z[p + "margins"])


@pytest.mark.parametrize("name,radius", list(_cases()))
def test_fixture_margins_and_paths(name, radius):
    z = gu.load(name)
    assert list(z["paths"]) == list(R.PATHS)
    assert z[f"r{radius}_margins"].min() > 1e-4
    counts = dict(zip(R.PATHS, z[f"r{radius}_counts"]))
    assert counts["create"] > 0 and counts["append"] > 0 and counts["reject"] > 0
    assert int(z[f"r{radius}_cnt"].sum()) == len(z[f"r{radius}_feat"]) == len(z[f"r{radius}_dis"])


@pytest.mark.parametrize("name", DIRECT)
def test_direct_fixture_fires_every_path(name):
    z = gu.load(name)
    total = z["r1_counts"] + z["r2_counts"]
    assert (total > 0).all(), dict(zip(R.PATHS, total))


def test_replay_nan_and_zero_group():
    """A zero token next to grid_0_0_0's zero group: NaN surprise, dropped; without neighbours: +inf, appended, then slot 0."""
    D = 4
    st = {(0, 0, 0): [[np.zeros(D, np.float32)], [0.0], [False]]}
    x = np.array([1, 0, 0, 0], np.float32)
    counts, _ = R.replay(st, np.array([[1, 0, 0]] * 2), np.stack([x, x]), np.array([1.0, 2.0]), 1, 0.5, 0.95, 2)
    assert counts["create"] == 1 and counts["nan_reject"] == 1 and len(st[(1, 0, 0)][0]) == 1
    counts, _ = R.replay(st, np.zeros((3, 3), np.int32), np.zeros((3, D), np.float32), np.zeros(3), 1, 0.5, 0.95, 2)
    # (1,0,0) holds a real token and is a neighbour of (0,0,0): the zero row's cosine is NaN -> dropped
    assert counts["nan_reject"] == 3 and len(st[(0, 0, 0)][0]) == 1
