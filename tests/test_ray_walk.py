"""The traversal of bsc_render_views (csrc/ray_walk.h: the very code k_rv_cast runs) on the CPU: a stand-alone program
(tests/host/ray_walk_main.cpp) built with g++, with the address / undefined-behaviour sanitizers where they link, run as a child
process on the scenes of tests/test_gpu_render.py.  The program checks the walk over a host-built brick mask against its own slab
test of every ray with every voxel; here its per-pixel results are also held against the NumPy reference the GPU tests use
(render_scenes.slab_reference), so that reference is itself checked without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import render_scenes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bsc-nav_amd", "csrc")


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    out = tmp_path_factory.mktemp("ray_walk")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++", *san, str(probe), "-o", str(out / "probe")], capture_output=True).returncode == 0
    ok = ok and subprocess.run([str(out / "probe")], capture_output=True).returncode == 0
    exe = out / "ray_walk_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(san if ok else []),
           os.path.join(ROOT, "tests", "host", "ray_walk_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _one_brick():
    grid = dict(gs=4, nh=4, min_h=-2, cs=0.25, t_min=0.05, t_max=10.0)
    pos = np.array([(0, 0, 0), (3, 3, 3), (1, 2, 1), (2, 1, 3), (3, 0, 2), (0, 3, 1)], np.int32)
    cams = [("inside", rs._pose((0.11, -0.07, 0.06), rs._euler(10.0, 20.0, 30.0)), 24, 32),
            ("outside", rs._pose((2.3, 1.9, 0.8), rs._look((-1.0, -0.8, -0.3))), 24, 32)]
    return grid, pos, cams


def _groups():
    """name -> (grid, pos, [(case name, T, kinv, H, W, t_min, t_max, band as given)])"""
    g1, pos1 = rs.CASE1, rs.case1_voxels()[0]
    out = {"case1": (g1, pos1, [(n, T, rs.kinv_fov(H, W), H, W, g1["t_min"], g1["t_max"], None) for n, T, H, W in rs.case1_cameras()])}
    n, T, H, W = rs.case1_cameras()[0]
    out["case1_band_range"] = (g1, pos1, [("band_3_7", T, rs.kinv_fov(H, W), H, W, 0.1, 10.0, (3, 7)),
                                          ("band_above", T, rs.kinv_fov(H, W), H, W, 0.1, 10.0, (20, 30)),
                                          ("short_range", T, rs.kinv_fov(H, W), H, W, 0.5, 1.5, None),
                                          ("from_zero", T, rs.kinv_fov(H, W), H, W, 0.0, 3.0, (-5, 8))])
    g2 = rs.CASE2
    for name, pos in rs.case2_scenes().items():
        out["case2_" + name] = (g2, pos, [(n, T, rs.kinv_fov(H, W), H, W, g2["t_min"], g2["t_max"], None)
                                          for n, T, H, W in rs.case2_cameras()])
    g3, pos3, cams3 = _one_brick()
    out["one_brick"] = (g3, pos3, [(n, T, rs.kinv_fov(H, W), H, W, g3["t_min"], g3["t_max"], None) for n, T, H, W in cams3])
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_walk_against_the_slab_tests(walk_program, tmp_path, group):
    grid, pos, cases = GROUPS[group]
    scene, result = tmp_path / "scene.txt", tmp_path / "result.txt"
    rs.write_scene_file(scene, grid, pos, [c[:7] + (rs.clip_band(c[7], grid["nh"]),) for c in cases])
    r = subprocess.run([walk_program, str(scene), str(result)], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and len(lines) == len(cases), r.stdout + r.stderr
    for line, c in zip(lines, cases):
        assert line.startswith("ok %s " % c[0]), r.stdout + r.stderr
    # the same results against the NumPy reference of the GPU tests
    got = [ln.split() for ln in open(result).read().splitlines()]
    cell = np.array([[int(v) for v in g[:3]] for g in got], np.int64)
    t = np.array([float.fromhex(g[3]) for g in got])
    at = 0
    for name, T, kinv, H, W, t_min, t_max, band in cases:
        ref = rs.slab_reference(grid["gs"], grid["nh"], grid["min_h"], grid["cs"], pos, T, kinv, H, W, t_min, t_max, band)
        P = H * W
        c, tt = cell[at:at + P], t[at:at + P]
        at += P
        sure = ~ref["ambiguous"]
        assert ref["ambiguous"].sum() <= rs.AMBIGUOUS_CAP * P, (name, int(ref["ambiguous"].sum()))
        want = np.where(ref["idx"][:, None] >= 0, np.asarray(pos, np.int64)[np.maximum(ref["idx"], 0)], -1)
        assert np.array_equal(c[sure], want[sure]), name
        assert np.array_equal(tt[sure], ref["t"][sure]), name          # the same planes, the same division: the same bits
        if group == "case1":                                               # every camera sees something, the inner ones a lot
            assert (ref["idx"] >= 0).sum() > (P // 2 if name[0] in "abcd" else 30), (name, "the camera sees next to nothing")
            assert (ref["idx"] < 0).sum() > 30, (name, "no ray leaves the scene")
    assert at == len(cell)


def test_walk_header_is_host_and_device_code():
    """ray_walk.h includes no HIP header (the program above includes nothing else of the library), has no unbounded loop, and is
    what render.hip walks with."""
    src = re.sub(r"//.*", "", open(os.path.join(CSRC, "ray_walk.h")).read())
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == ["stdint.h"]
    assert not re.search(r"while\s*\(\s*(true|1)\s*\)|for\s*\(\s*;\s*;\s*\)", src)
    main = open(os.path.join(ROOT, "tests", "host", "ray_walk_main.cpp")).read()
    assert re.findall(r"#include\s*\"([^\"]+)", main) == ["../../bsc-nav_amd/csrc/ray_walk.h"]
    render = open(os.path.join(CSRC, "render.hip")).read()
    assert '#include "ray_walk.h"' in render and "rw_first_hit(" in render
    assert "ray_walk.h" in open(os.path.join(CSRC, "build.sh")).read()
