"""wino88i32_gemm_r3k64_kernel's tile epilogue (the three-level combine, the rounding to fp32 and M's
addressing: one 64-bit base per tile plus a 32-bit offset inside it) through kv_dev_wino88i_r3, which runs R3's
slice kernel and GEMM with an explicit tiles-per-workgroup, workgroup count, row stride and first row -- so 128
rows reach the group loop, the exponents staged by group parity, the copy ring across group boundaries, a tile
that is not at row 0 and element offsets past 2^31 bytes. Every case is bit for bit against
tests/_i8_digits.gemm_r3 on test_i8r3_gemm_bit_exact's edge rows (a zero row, the 127/128 exponent bump,
subnormals, +-2^-40), and every element of M outside the written rows must stay as the entry initialised it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _i8_digits as D

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(K):
    """V [100][256][K], U [100][512][K] and gemm_r3's M for them, computed once per K (read-only). A row of M
    depends on that row of V alone, so the 128-row cases take the first 128 rows."""
    rng = np.random.default_rng(K + 11)
    V = rng.standard_normal((100, 256, K)) * np.exp2(rng.integers(-20, 20, size=(100, 256, 1)))
    V[0, 0] = 0.0
    V[1, 1] = np.nextafter(8.0 * 127 / 128, 0.0) * np.where(rng.random(K) < 0.5, -1.0, 1.0)
    V[1, 2] = 8.0 * 127 / 128
    V[1, 3] = -8.0 * 255 / 256
    V[2, 2, ::3] = 1e-310
    V[3, 3] = np.where(rng.random(K) < 0.5, -1.0, 1.0) * np.exp2(-40.0)
    U = rng.standard_normal((100, 512, K)) * 0.05
    U[5, 7] = 0.0
    Mr, _, _ = D.gemm_r3(V, U)
    for a in (V, U, Mr):
        a.setflags(write=False)
    return V, U, Mr


def _check(K, rows, tpw, nwg, stride=None, row0=0):
    from knightvision_amd import _lib
    L = _lib.lib()
    V, U, Mr = _case(K)
    V = np.ascontiguousarray(V[:, :rows])
    M = np.zeros((100, rows, 512))
    outside = C.c_longlong(-1)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    _lib.check(L.kv_dev_wino88i_r3(0, P(V, C.c_double), rows, P(U, C.c_double), K, tpw, nwg, stride or rows, row0,
                                   P(M, C.c_double), C.byref(outside)), "kv_dev_wino88i_r3")
    want = Mr[:, :rows]
    same = M.view(np.uint64) == want.view(np.uint64)
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), float(np.abs(M - want).max()))
    assert outside.value == 0, f"{outside.value} elements of M outside the written rows changed"


@pytest.mark.parametrize("K", [512, 256])
def test_r3_epilogue_single_tiles(K):
    """One tile per workgroup on the default grid: no previous tile, the epilogue right after the only one."""
    _check(K, 128, 1, 0)


def test_r3_epilogue_tpw4_default_grid():
    _check(512, 256, 4, 0)


@pytest.mark.parametrize("nwg", [8, 40, 80])
def test_r3_epilogue_groups_tpw5(nwg):
    """400 tiles in 5-tile groups: 10, 2 and 1 groups per workgroup -- the group boundaries, the exponents by
    group parity, the ring across groups."""
    _check(512, 128, 5, nwg)


def test_r3_epilogue_groups_k256():
    """5 groups per workgroup at 4 stages per tile (K 256)."""
    _check(256, 128, 5, 16)


def test_r3_epilogue_groups_tpw4():
    """25 groups of 4 tiles per workgroup."""
    _check(512, 256, 4, 8)


def test_r3_epilogue_strided_slice():
    """The product's kernel and grid on rows 128-255 of 256-row buffers: the tile is not at row 0."""
    _check(512, 128, 0, 0, stride=256, row0=128)


def test_r3_epilogue_offsets_past_2g():
    """The last 128 rows of 16,384-row buffers: M is 3.36 GB, so most tiles' element offsets exceed 2^31 bytes
    (only those rows are copied back; the rest is checked on the device)."""
    _check(512, 128, 0, 0, stride=16384, row0=16384 - 128)
