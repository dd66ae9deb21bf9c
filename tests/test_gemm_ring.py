"""The weight-buffer ring of the split GEMM's DMA-scheduled tiles (csrc/gemm_split_plan.h: gs_w_ring, gs_ring_next / gs_ring_prev, the
buffer index of gs_dma_lds_off / gs_frag_off — the functions k_gemm_split calls) on the CPU: a stand-alone program
(tests/host/gemm_ring_main.cpp) built with g++, with the address / undefined-behaviour sanitizers where they link, run as a child process.
  image     for every buffer of the ring (three for the 256-row tiles, two for the 128 x 128 tile) the DMA plan writes, and the fragment
            reads of all lanes read, every byte of [buf, buf + 1) x gs_w_buf_bytes exactly once and nothing outside it
  layout    every plan of a grid of shapes: ring buffers, epilogue blocks and bias row do not overlap and end below 160 KB, the
            half-width form included; the 128 x 128 tile stays at two workgroups per CU; N = 20 000 is refused as before
  schedule  the ring walked as the kernel walks it (1 .. 8 chunks, tiles chained or not): a request never goes to the buffer being
            read or the one that lands next, and every chunk is read from the buffer its request went to"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["image", "layout", "schedule"]


@pytest.fixture(scope="module")
def ring_program(tmp_path_factory):
    out = tmp_path_factory.mktemp("gemm_ring")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++", *san, str(probe), "-o", str(out / "probe")], capture_output=True).returncode == 0
    ok = ok and subprocess.run([str(out / "probe")], capture_output=True).returncode == 0
    exe = out / "gemm_ring_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(san if ok else []),
           os.path.join(ROOT, "tests", "host", "gemm_ring_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_ring(ring_program, case):
    r = subprocess.run([ring_program, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
