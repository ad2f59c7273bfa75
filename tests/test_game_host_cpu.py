"""The players' rate tables of rq_log_game (rqh::game_tables in csrc/rq_topo.cpp) and their
refusals without a GPU: tests/host/game_table_check.cpp, built like tests/host/plan_check.cpp
-- the system C++ compiler under AddressSanitizer and UBSan, no ROCm include path, nothing
loaded into Python -- and run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redqueen_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_game_tables_without_a_gpu(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "game_table_check")
    src = [os.path.join(CSRC, "rq_topo.cpp"), os.path.join(ROOT, "tests", "host", "game_table_check.cpp")]
    obj = [str(tmp_path / ("%d.o" % k)) for k in range(len(src))]
    ccs = [subprocess.Popen([cxx] + FLAGS + ["-Wall", "-c", "-o", o, s], stderr=subprocess.PIPE, text=True)
           for o, s in zip(obj, src)]
    for cc in ccs:
        err = cc.communicate()[1]
        assert cc.returncode == 0, err
    ld = subprocess.run([cxx] + FLAGS + ["-o", exe] + obj, capture_output=True, text=True)
    assert ld.returncode == 0, ld.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
