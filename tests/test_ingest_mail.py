"""The scalar mailbox of bsc_ingest (csrc/ingest_mail.h: word format + the host's take) on the CPU: a stand-alone program
(tests/host/ingest_mail_main.cpp) built with g++, with the address / undefined-behaviour sanitizers where they link, run as a
child process — and the static rule that goes with the explicit primitive lanes: nobody redirects the context's stream."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bsc-nav_amd", "csrc")
CASES = ["all_tagged", "one_stale_word", "sign_and_range", "tag_wraps", "rewrite_between_takes"]


@pytest.fixture(scope="module")
def mail_program(tmp_path_factory):
    out = tmp_path_factory.mktemp("ingest_mail")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ok = subprocess.run(["g++", *san, str(probe), "-o", str(out / "probe")], capture_output=True).returncode == 0
    ok = ok and subprocess.run([str(out / "probe")], capture_output=True).returncode == 0
    exe = out / "ingest_mail_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(san if ok else []),
           os.path.join(ROOT, "tests", "host", "ingest_mail_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_mailbox(mail_program, case):
    r = subprocess.run([mail_program, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr


def test_mail_header_is_host_only():
    """ingest_mail.h compiles without HIP (the program above includes nothing else) and names no HIP header."""
    src = open(os.path.join(CSRC, "ingest_mail.h")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()


def test_only_capi_sets_the_context_stream_and_workspace():
    """The primitives take their stream and workspace as a PrimLane argument: outside bsc_create / ctx_build (capi.hip) no file
    under csrc/ assigns x->stream or x->prim_tmp."""
    hits = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h", ".cpp")) or f == "capi.hip":
            continue
        for n, line in enumerate(open(os.path.join(CSRC, f)), 1):
            if re.search(r"x->(stream|prim_tmp)\s*=(?!=)", line):
                hits.append((f, n))
    assert not hits, hits
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert len(re.findall(r"x->stream\s*=(?!=)", capi)) == 1 and "&x->prim_tmp," in capi
