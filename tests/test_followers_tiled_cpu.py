"""CPU side of rq_log_followers_tiled (no GPU): the three symbols and their export, the
tile size's bound, validation before any HIP call, and the sink-tiled CSR of the host core
(GraphTopo.tile_ptr / tile_col) through tests/host/tile_check.cpp -- built with the system
C++ compiler under AddressSanitizer and UBSan from rq_topo.cpp + rq_plan.cpp, no ROCm
include path, nothing loaded into Python, run as a child process.

The workspace size, 4 * n_rep * ceil(n_sinks / TS) rounded up to 256 bytes, is checked
twice: its arithmetic (rqh::followers_tiled_ws_bytes, which the ABI query returns) in
tile_check.cpp here, and the ABI query on real graphs in tests/test_gpu_followers_tiled.py
-- a graph handle needs a device, so without one the query can only be shown to refuse.
For the same reason the workspace that is one byte short (its size depends on the graph) is
refused there, in test_validation_on_device, beside the null workspace refused here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from redqueen_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redqueen_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_symbols_are_exported():
    lib = L.lib()
    for fn in ("rq_log_followers_tiled", "rq_log_followers_tiled_workspace"):
        assert fn in L.EXPORTED and hasattr(lib, fn), fn
    assert hasattr(lib, "rq_log_followers_tile_sinks")
    src = open(os.path.join(ROOT, "include", "rq.h")).read()
    assert "#define RQ_FOLLOWERS_TILED_MAX_SINKS %d" % L.FOLLOWERS_TILED_MAX_SINKS in src
    assert L.FOLLOWERS_TILED_MAX_SINKS == 40960 and lib.rq_abi_version() == 6


def test_tile_size_fits_every_variant():
    lib = L.lib()
    TS = int(lib.rq_log_followers_tile_sinks())
    # TS * (12 + 8 * (4 + 2) + 8) <= 160 KiB: every nK and rows variant of a tile fits
    assert 0 < TS <= 2409
    assert TS <= int(lib.rq_log_followers_max_sinks(L.MAX_K, 1))


def test_validation_comes_before_hip():
    """No GPU here: anything but RQ_EINVAL would mean a HIP call was reached.  g is a
    non-null dummy handle where the argument under test is another one: validation must
    refuse before it looks into the graph."""
    lib = L.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    k1 = np.asarray([1, 2, 3, 4, 5], dtype=np.int32)
    k0 = np.asarray([1, 0], dtype=np.int32)

    def call(h=p, ev_t=p, ev_src=p, counts=p, n_rep=2, cap=4, ks=k1, nK=2, vals=p, first=p, rows=None,
             r2=p, sta=p, ws=p, ws_bytes=4096):
        return lib.rq_log_followers_tiled(h, ev_t, ev_src, counts, n_rep, cap,
                                          None if ks is None else ks.ctypes.data_as(L._pi32), nK, vals,
                                          first, rows, r2, sta, ws, ws_bytes, None)
    # rq_log_followers' list (tests/test_gpu_followers.py, test_validation) ...
    bad = [dict(nK=0), dict(nK=5), dict(nK=-1), dict(ks=k0), dict(ks=None), dict(n_rep=0), dict(n_rep=-2),
           dict(n_rep=1 << 31), dict(cap=0), dict(cap=-1), dict(cap=(1 << 24) + 1), dict(vals=None),
           dict(first=None), dict(r2=None), dict(sta=None), dict(h=None), dict(ev_t=None), dict(ev_src=None),
           dict(counts=None)]
    # ... and a null workspace
    bad += [dict(ws=None), dict(ws=None, ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == L.RQ_EINVAL, kw
    assert bytes(buf) == b"\0" * 4096
    n = C.c_size_t(77)
    assert lib.rq_log_followers_tiled_workspace(None, 4, C.byref(n)) == L.RQ_EINVAL
    assert lib.rq_log_followers_tiled_workspace(p, 4, None) == L.RQ_EINVAL
    assert lib.rq_log_followers_tiled_workspace(p, 0, C.byref(n)) == L.RQ_EINVAL
    assert lib.rq_log_followers_tiled_workspace(p, 1 << 31, C.byref(n)) == L.RQ_EINVAL
    assert n.value == 77


def test_tiled_csr_of_the_host_core(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "tile_check")
    src = [os.path.join(CSRC, "rq_topo.cpp"), os.path.join(CSRC, "rq_plan.cpp"),
           os.path.join(ROOT, "tests", "host", "tile_check.cpp")]
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
