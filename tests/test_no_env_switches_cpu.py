"""The inference library reads no environment variable and keeps no retired A/B kernel form: no getenv
under csrc/, the dev entries refuse the removed forms' flags with KV_EINVAL before any device call (so these
run without a GPU), and the A/B GEMM bench entry is neither declared nor exported."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV_EINVAL = -1


def test_csrc_reads_no_environment():
    files = sorted(glob.glob(os.path.join(REPO, "knightvision_amd", "csrc", "*")))
    assert files
    hits = [os.path.basename(f) for f in files if "getenv" in open(f, errors="replace").read()]
    assert not hits, hits


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def test_dev_wino88i_refuses_segment_exponents():
    """seg 1 (V's exponents per 256-channel segment) went with its GEMM; the dummy pointers are never read."""
    from knightvision_amd import _lib
    L = _lib.lib()
    d, b, e = np.zeros(1), np.zeros(1, dtype=np.int8), np.zeros(1, dtype=np.int32)
    rc = L.kv_dev_wino88i(0, _ptr(d, C.c_double), 128, _ptr(d, C.c_double), 512, 4, 1, _ptr(d, C.c_double),
                          _ptr(b, C.c_int8), _ptr(e, C.c_int32))
    assert rc == KV_EINVAL
    assert "seg 1" in L.kv_last_error().decode()


@pytest.mark.parametrize("fused", [1 | 2, 1 | 8, 1 | 32])
def test_dev_wino88i32_out_refuses_removed_forms(fused):
    """Bits 1 (segment exponents), 3 (the 64-register kernel) and 5 (the persistent kernel) are refused."""
    from knightvision_amd import _lib
    L = _lib.lib()
    f, b, e = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.int8), np.zeros(1, dtype=np.int32)
    fp = _ptr(f, C.c_float)
    rc = L.kv_dev_wino88i32_out(0, fp, 128, fp, fp, None, fused, fp, _ptr(b, C.c_int8), _ptr(e, C.c_int32))
    assert rc == KV_EINVAL
    assert f"fused {fused}" in L.kv_last_error().decode()


def test_gemm_bench_entry_is_gone():
    from knightvision_amd import _lib
    assert "kv_dev_i8gemm_bench" not in open(os.path.join(REPO, "include", "kv.h")).read()
    assert "kv_dev_i8gemm_bench" not in _lib.EXPORTED
    assert not hasattr(C.CDLL(_lib.LIB_PATH), "kv_dev_i8gemm_bench")
