"""The LDS weight image and the fragment maps of the split GEMM's 16x16x32 main loop (csrc/gemm_split_plan.h: gs_dma_*, gs_frag_off,
gs_acc_* — the functions k_gemm_split calls) on the CPU: a stand-alone program (tests/host/gemm_frag_main.cpp) built with g++, with
the address / undefined-behaviour sanitizers where they link, run as a child process.
  image     the DMA plan of a 512- and of a 256-thread workgroup composed with the fragment reads: lane (i, g) of tile t' gets weight
            row 16 t' + i, halfs 8 g .. 8 g + 7; every byte of a chunk lands exactly once
  banks     every 16-lane group of a ds_read_b128 touches 16 different 16-byte slots; the swizzle of the 32-row fragment does not
  epilogue  (lane, row half, tile, register) -> (row, column) is a bijection onto the wavefront's strip; bias index = column"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["image", "banks", "epilogue"]


@pytest.fixture(scope="module")
def frag_program(tmp_path_factory):
    out = tmp_path_factory.mktemp("gemm_frag")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++", *san, str(probe), "-o", str(out / "probe")], capture_output=True).returncode == 0
    ok = ok and subprocess.run([str(out / "probe")], capture_output=True).returncode == 0
    exe = out / "gemm_frag_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(san if ok else []),
           os.path.join(ROOT, "tests", "host", "gemm_frag_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_frag_map(frag_program, case):
    r = subprocess.run([frag_program, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
