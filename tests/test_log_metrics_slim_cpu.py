"""CPU side of rq_log_metrics_slim / rq_log_metrics_of_slim (no GPU): the symbols, the
limit the header and the binding state, and the argument checks that come before any HIP
call.  The kernels are tested in tests/test_gpu_log_metrics_slim.py."""
import ctypes as C
import os
import re

import numpy as np

SLIM = ("rq_log_metrics_slim_workspace", "rq_log_metrics_slim",
        "rq_log_metrics_of_slim_workspace", "rq_log_metrics_of_slim")


def test_symbols():
    from redqueen_amd import _lib as L
    lib = L.lib()
    for fn in SLIM:
        assert fn in L.EXPORTED and fn in L.OPTIONAL_SLIM and L.has(fn) and hasattr(lib, fn), fn
    assert set(L.OPTIONAL_SLIM) == set(SLIM)
    assert lib.rq_abi_version() == 6 and L.ABI_VERSION == 6


def test_the_limit_is_the_headers():
    from redqueen_amd import _lib as L
    assert L.LOG_METRICS_SLIM_MAX_SINKS == 19400
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "rq.h")).read()
    assert re.search(r"#define RQ_LOG_METRICS_SLIM_MAX_SINKS\s+%d\b" % L.LOG_METRICS_SLIM_MAX_SINKS, src)
    assert re.search(r"#define RQ_LOG_METRICS_MAX_SINKS\s+9800\b", src)   # the 16-byte entries keep theirs
    # the LDS formula of the slim cells: scratch + 8 n + 4 W + round4(2 W), W = ceil(n / 32)

    def lds(n):
        w = (n + 31) // 32
        return 4784 + 8 * n + 4 * w + (2 * w + 3) // 4 * 4
    assert lds(L.LOG_METRICS_SLIM_MAX_SINKS) == 163628 and lds(19426) == 160 * 1024 < lds(19427)


def test_null_arguments_are_refused_before_any_hip_call():
    from redqueen_amd import _lib as L
    lib = L.lib()
    E = L.RQ_EINVAL
    k = np.asarray([1], dtype=np.int32)
    ids = np.asarray([1], dtype=np.int64)
    n = C.c_size_t(12345)
    fake = C.create_string_buffer(64)   # stands for a graph: a NULL ``bytes`` is refused before g is read
    h = C.cast(fake, C.c_void_p)
    assert lib.rq_log_metrics_slim_workspace(None, 1, 1, 1, C.byref(n)) == E
    assert lib.rq_log_metrics_slim_workspace(h, 1, 1, 1, None) == E
    assert lib.rq_log_metrics_of_slim_workspace(None, 1, 1, 1, 1, C.byref(n)) == E
    assert lib.rq_log_metrics_of_slim_workspace(h, 1, 1, 1, 1, None) == E
    assert n.value == 12345   # a refused query writes nothing
    assert lib.rq_log_metrics_slim(None, None, None, None, 1, 1, k.ctypes.data_as(L._pi32), 1, None, None, None,
                                   None, 0, None) == E
    assert lib.rq_log_metrics_of_slim(None, ids.ctypes.data_as(L._pi64), 1, L.LOG_OF_DF, None, None, None, 1, 1,
                                      k.ctypes.data_as(L._pi32), 1, None, None, None, None, 0, None) == E
