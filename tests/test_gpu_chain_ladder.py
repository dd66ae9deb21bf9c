"""The default dense ingest path — every pixel, no alpha passed: k_points<fast, RPW, PLAIN, REC8> and the REC8 forms of k_chain,
k_chain_long (hot and mid) and k_hwin, which bench.py times — bit for bit against the sequential oracle on the ladder scene of
tests/chain_ladder.py, where every voxel's segment of a call has a length chosen in advance (tests/test_chain_ladder.py proves on the
CPU that no rung is missing).

Reference: the oracle ingests the same frames; per pixel it takes the alpha the library's own export reports (bsc_geometry:
k_geometry_debug runs geom_point with the device bsc_exp).  Every k_points form and the chain's re-evaluation from an 8-byte record
produce that same double by design, so max_id, positions, rgb bytes, weights, max_height, cv_map and counts are compared with no
tolerance; feature means within rtol = atol = 1e-3 (the oracle adds the points one by one in f32)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import chain_ladder as cl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = cl.EXACT
KNOBS = ["BSC_REC12=1", "BSC_GENERIC_GEOMETRY=1", "BSC_QUAD_CHAIN_ONLY=1", "BSC_NO_HOT_SPLIT=1", "BSC_CHAIN_SPLIT=0", "BSC_LONG_NWV=16",
         "BSC_HOT_LOG2=10", "BSC_LONG_LOG2=8", "BSC_GROUP_RPW=4", "BSC_GROUP_RPW=16", "BSC_CHAIN_EAGER=1", "BSC_ORDER_MAIN=1",
         "BSC_TOTALS_UNFUSED=1", "BSC_NO_MAILBOX=1"]
REC12_KNOBS = ("BSC_REC12", "BSC_GENERIC_GEOMETRY")          # the two under which the 8-byte records are off


def _engine():
    import bsc_nav_amd as B
    return B.VoxelEngine(cl.H, cl.W, cl.GS, cl.CS, cl.FLOOR, cl.TOP, cl.G, cl.D, mode="mean", voxel_capacity=cl.VCAP,
                         max_points=len(cl.ORDER) * cl.H * cl.W)


def _oracle_states(eng, calls):
    """The oracle's state after every call of `calls`, each pixel's alpha taken from eng.geometry."""
    import torch
    from oracle import oracle as orc
    om = orc.OracleMemory(cl.config(), voxel_capacity=cl.VCAP)
    alphas, out = {}, []
    for call in calls:
        if id(call.depth) not in alphas:                    # D is B's frames again
            alphas[id(call.depth)] = [eng.geometry(torch.from_numpy(call.depth[f]).cuda(), call.Ts[f])["alpha"]
                                      for f in range(len(call.depth))]
        for f in range(len(call.depth)):
            om.ingest_frame(call.depth[f], call.rgb[f], None, call.Ts[f], call.tokens[f], alphas[id(call.depth)][f])
        out.append(cl.state(om))
    return out


@pytest.fixture(scope="module")
def scene():
    return cl.build_scene()


@pytest.fixture(scope="module")
def reference(scene):
    """Computed once, shared, never written to."""
    eng = _engine()
    ref = _oracle_states(eng, scene["calls"])
    eng.close()
    return ref


@functools.lru_cache(maxsize=None)
def _device_calls(channels):
    """[(depth, rgb, tokens, Ts)] of the four calls on the GPU: uploaded before the first ingest, so that nothing between two calls
    synchronises"""
    import torch
    out = []
    for call in cl.build_scene()["calls"]:
        rgb = call.rgb if channels == 4 else call.rgb3()
        out.append((torch.from_numpy(call.depth).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(call.tokens).cuda(), call.Ts))
    torch.cuda.synchronize()
    return out


def _back_to_back(channels):
    eng = _engine()
    for d, c, t, Ts in _device_calls(channels):
        eng.ingest(d, c, t, Ts)
    got = cl.state(eng)
    eng.close()
    return got


@pytest.mark.parametrize("channels", [3, 4])
def test_ladder_four_calls_back_to_back(scene, reference, channels):
    """Calls A to D with nothing between them: each call's chain stays deferred and overlaps the next call's front end, both
    scratch sets are used twice.  3-channel and RGBA frames (the bench's) are the same scene."""
    wants = [c.want for c in scene["calls"]]
    cl.compare(_back_to_back(channels), reference[3], "after A B C D, %d channels" % channels, wants)


def test_ladder_call_by_call(scene, reference):
    """The same with an export after every call, so that a failure names the call; the final state is the back-to-back one."""
    eng = _engine()
    wants = [c.want for c in scene["calls"]]
    for i, (d, c, t, Ts) in enumerate(_device_calls(4)):
        eng.ingest(d, c, t, Ts)
        got = cl.state(eng)
        cl.compare(got, reference[i], "after call " + cl.CALLS[i], wants[:i + 1])
    eng.close()
    b2b = _back_to_back(4)
    assert set(got) == set(b2b)
    for k in got:                                           # the feature sums too: the same calls in the same order
        assert got[k].dtype == b2b[k].dtype and got[k].shape == b2b[k].shape and got[k].tobytes() == b2b[k].tobytes(), k


def test_ladder_as_one_call_per_frame(scene, reference):
    """Call A's frames, one frame per call: segments are cut at frame ends and the launch sizes of the long chain sit at their lower
    clamps; the final map is the one of the single call."""
    eng = _engine()
    d, c, t, Ts = _device_calls(4)[0]
    for f in range(len(cl.ORDER)):
        eng.ingest(d[f:f + 1], c[f:f + 1], t[f:f + 1], Ts[f:f + 1])
    got = cl.state(eng)
    eng.close()
    cl.compare(got, reference[0], "call A frame by frame", [scene["calls"][0].want])


# ---- the chain knobs: one interpreter per case ---------------------------------------------------------------------------------
def _run_ladder(out_path):
    """Calls A to D on one engine, compared with the oracle, the final state written to out_path (runs in a child interpreter)."""
    sc = cl.build_scene()
    eng = _engine()
    ref = _oracle_states(eng, sc["calls"])
    for d, c, t, Ts in _device_calls(4):
        eng.ingest(d, c, t, Ts)
    got = cl.state(eng)
    eng.close()
    np.savez(out_path, **got)
    cl.compare(got, ref[3], "after A B C D", [c.want for c in sc["calls"]])


def _child(out_path, knob=None):
    """-> the arrays the child wrote and the rec8 values its BSC_DEBUG lines name"""
    code = ("import sys; sys.path[:0] = ['.', 'tests', 'tests/golden']; import test_gpu_chain_ladder as t; "
            "t._run_ladder(%r); print('ok')" % out_path)
    env = {k: v for k, v in os.environ.items() if k not in {kn.split("=")[0] for kn in KNOBS}}
    env["BSC_DEBUG"] = "1"
    if knob:
        name, val = knob.split("=")
        env[name] = val
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    lines = re.findall(r"^bsc_ingest: k_points fast=(\d) plain=(\d) rec8=(\d) group_rpw=(\d+)$", r.stderr, flags=re.M)
    with np.load(out_path) as z:
        return {n: z[n] for n in z.files}, lines


@pytest.fixture(scope="module")
def default_run(tmp_path_factory):
    got, lines = _child(str(tmp_path_factory.mktemp("ladder") / "default.npz"))
    assert lines == [("1", "1", "1", "8")], lines          # the kernels the bench runs; one line per context and choice
    return got


@pytest.mark.parametrize("knob", KNOBS)
def test_ladder_under_the_chain_knobs(default_run, tmp_path, knob):
    """The library's A/B switches on the kernels the bench runs (no alpha passed: PLAIN / REC8 unless the knob itself turns the
    8-byte records off, which the BSC_DEBUG line of ingest_front_end shows): calls A to D against the oracle, and the final state
    byte for byte that of the default run.  Under BSC_HOT_LOG2=10 and BSC_LONG_LOG2=8 the ladder's thresholds move; the result
    must not.  That holds for the feature sums too: with every pixel ingested a voxel's pairs are reduced in (frame, patch) order
    whatever kernels listed them (dense.hip), so no switch here may move a bit of them."""
    got, lines = _child(str(tmp_path / "knob.npz"), knob)
    name, val = knob.split("=")
    fast = "0" if name == "BSC_GENERIC_GEOMETRY" else "1"
    plain = fast                                            # PLAIN is a form of the fast k_points only
    rec8 = "0" if name in REC12_KNOBS else "1"
    rpw = val if name == "BSC_GROUP_RPW" else "8"
    assert lines == [(fast, plain, rec8, rpw)], lines
    assert set(got) == set(default_run)
    for k in sorted(got):
        assert got[k].dtype == default_run[k].dtype and got[k].shape == default_run[k].shape, k
        assert got[k].tobytes() == default_run[k].tobytes(), "%s under %s differs from the default run" % (k, knob)
