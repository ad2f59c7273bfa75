"""When the planner gives the merged fused sweep 16-byte row records, at the edges of the
record's fields (65,535 sinks; n_sinks x merged entries per replica = 2^32), without a GPU:
tests/host/rows16_check.cpp with the HIP-free host core (csrc/rq_host.h, rq_topo.cpp,
rq_plan.cpp), built with the system C++ compiler and run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redqueen_amd", "csrc")


def test_rows16_condition_at_its_edges(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "rows16_check")
    src = [os.path.join(CSRC, "rq_topo.cpp"), os.path.join(CSRC, "rq_plan.cpp"),
           os.path.join(ROOT, "tests", "host", "rows16_check.cpp")]
    obj = [str(tmp_path / ("%d.o" % k)) for k in range(len(src))]
    ccs = [subprocess.Popen([cxx, "-std=c++17", "-O1", "-Wall", "-c", "-o", o, s], stderr=subprocess.PIPE, text=True)
           for o, s in zip(obj, src)]
    for cc in ccs:
        err = cc.communicate()[1]
        assert cc.returncode == 0, err
    ld = subprocess.run([cxx, "-o", exe] + obj, capture_output=True, text=True)
    assert ld.returncode == 0, ld.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
