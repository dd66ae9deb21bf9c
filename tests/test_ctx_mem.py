"""The context's memory ledger (csrc/ctx_mem.cpp) on the CPU: a stand-alone program of the ledger, a malloc-backed stub of
the four HIP allocation calls (tests/host/hip_stub.cpp) and a main with the cases (tests/host/ctx_mem_main.cpp), run as a
child process.  The stub keeps every live pointer with its kind and aborts on a free of an unknown pointer or through the
wrong call; with the address / undefined-behaviour sanitizers where they link, without them otherwise."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["alloc_free_grow", "pinned_flags", "free_null_and_released", "mark_release_to", "fail_each", "all_or_nothing",
         "failed_grow_retries"]


def _rocm():
    if os.environ.get("ROCM_PATH"):
        return os.environ["ROCM_PATH"]
    hipcc = shutil.which("hipcc")
    return os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else "/opt/rocm"


@pytest.fixture(scope="module")
def ledger_program(tmp_path_factory):
    out = tmp_path_factory.mktemp("ctx_mem")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++", *san, str(probe), "-o", str(out / "probe")], capture_output=True).returncode == 0
    ok = ok and subprocess.run([str(out / "probe")], capture_output=True).returncode == 0
    exe = out / "ctx_mem_test"
    srcs = [os.path.join(ROOT, "bsc-nav_amd", "csrc", "ctx_mem.cpp"), os.path.join(ROOT, "tests", "host", "hip_stub.cpp"),
            os.path.join(ROOT, "tests", "host", "ctx_mem_main.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(san if ok else []), "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(_rocm(), "include"), *srcs, "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_ledger(ledger_program, case):
    r = subprocess.run([ledger_program, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr


def test_ledger_source_is_host_only():
    """ctx_mem.cpp knows the public header, the HIP runtime API and its own header: nothing of bsc_ctx."""
    src = open(os.path.join(ROOT, "bsc-nav_amd", "csrc", "ctx_mem.cpp")).read()
    assert "bsc_internal.h" not in src and "bsc_ctx" not in src
    assert "bsc_internal.h" not in open(os.path.join(ROOT, "bsc-nav_amd", "csrc", "ctx_mem.h")).read()


def test_only_the_ledger_allocates():
    """No .hip file calls the allocation functions, the per-device tap table of encoder_ops.hip (no context owns it) excepted."""
    csrc = os.path.join(ROOT, "bsc-nav_amd", "csrc")
    hits = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        for n, line in enumerate(open(os.path.join(csrc, f)), 1):
            if any(w in line for w in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(")):
                hits.append((f, n))
    assert hits and all(f == "encoder_ops.hip" for f, _ in hits) and len(hits) == 2, hits
