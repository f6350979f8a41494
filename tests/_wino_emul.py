"""numpy restatement of the F(8x8) transforms for the GPU tests (test infrastructure): B10^T and A8^T of the
points 0, +-2/5, +-4/5, +-5/4, +-2 and infinity (csrc/kv_wino88d.h w88d_bt / w88d_at, derived exactly by
tools/wino_emulate.toom_cook_exact), applied in fp64 to the zero-padded 10x10 plane of each (board, channel) /
to the 10x10 points of M; and the |.| form of both (|matrix| on |data|), the factor of a rounding-error bound."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np

P88 = [Fr(0), Fr(2, 5), Fr(-2, 5), Fr(4, 5), Fr(-4, 5), Fr(5, 4), Fr(-5, 4), Fr(2), Fr(-2)]


def _toom_cook():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from wino_emulate import toom_cook
    return toom_cook(P88, 8)


def bt88():
    return _toom_cook()[2]


def at88():
    """A^T [8][10] (max |entry| 128)."""
    return _toom_cook()[0]


def input_transform_f64(Y, optimize=False):
    """Y [boards][64][C] (pixel = row * 8 + col) -> V [100][boards][C], V = B^T d B of the padded plane d.
    optimize: one axis at a time (einsum's pairwise contraction: a third of the time, another summation order)."""
    B, _, C = Y.shape
    d = np.zeros((B, 10, 10, C))
    d[:, 1:9, 1:9] = Y.reshape(B, 8, 8, C)
    BT = bt88()
    V = np.einsum("ai,bijc,dj->adbc", BT, d, BT, optimize=optimize)  # [10][10][boards][C]
    return V.reshape(100, B, C)


def input_transform_abs(Y):
    """|B^T| |d| |B|: input_transform_f64's einsum on the absolute values of the matrix and of the data."""
    B, _, C = Y.shape
    d = np.zeros((B, 10, 10, C))
    d[:, 1:9, 1:9] = np.abs(Y.reshape(B, 8, 8, C))
    BT = np.abs(bt88())
    return np.einsum("ai,bijc,dj->adbc", BT, d, BT, optimize=True).reshape(100, B, C)


def output_transform_f64(M):
    """M [100][boards][C] (point = a * 10 + b) -> T [boards][64][C] (pixel = row * 8 + col), T = A^T m A of
    the 10x10 points m of each (board, channel)."""
    _, B, C = M.shape
    AT = at88()
    T = np.einsum("ia,abnc,jb->nijc", AT, M.reshape(10, 10, B, C), AT, optimize=True)  # [boards][8][8][C]
    return T.reshape(B, 64, C)


def output_transform_abs(M):
    """|A^T| |m| |A|: output_transform_f64's einsum on the absolute values of the matrix and of the data."""
    _, B, C = M.shape
    AT = np.abs(at88())
    return np.einsum("ia,abnc,jb->nijc", AT, np.abs(M).reshape(10, 10, B, C), AT,
                     optimize=True).reshape(B, 64, C)
