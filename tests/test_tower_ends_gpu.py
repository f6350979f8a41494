"""The two ends of the fp32 tower on int8 digits, each as one kernel against the two-kernel form it replaces,
bit for bit.
Front (kv_dev_tower_front, the R3 tower): stem_r3_kernel -- conv1 + BN + ReLU from the board codes, conv2's input
transform, row exponents and 3 radix-256 digits in 96-byte row lines, no fp32 V256 -- against stem_kernel<4>'s
V256 followed by the slice kernel.
Back (kv_dev_tower_back): wino88_out_heads_kernel -- the last residual block's output transform with the heads on
top, the board's activation going from one to the other through LDS, X never written -- against
wino88_out_kernel<true, true, false>'s X followed by heads_kernel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _front(codes, rows, wT, scale, shift, fused):
    from knightvision_amd import _lib
    L = _lib.lib()
    nb = codes.shape[0]
    buf = np.zeros(100 * 8 * rows * 128, dtype=np.int8)
    ex = np.full((100, rows), -999, dtype=np.int32)
    F = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    _lib.check(L.kv_dev_tower_front(0, np.ascontiguousarray(codes).ctypes.data_as(C.POINTER(C.c_int8)), nb, rows,
                                    F(wT), F(scale), F(shift), int(fused),
                                    buf.ctypes.data_as(C.POINTER(C.c_int8)), ex.ctypes.data_as(C.POINTER(C.c_int32))),
               "kv_dev_tower_front")
    n = 100 * 8 * rows * 96
    return buf[:n].reshape(100, 8, rows, 3, 32), buf[n:], ex


@pytest.mark.parametrize("rows,nb", [(32, 32), (128, 128), (64, 41), (544, 530)])
def test_stem_writes_conv2s_r3_digits(rows, nb):
    """Random legal-looking piece codes (half the squares empty), board 3 empty (all-zero rows under a
    non-positive BN shift: exponent 0, digits 0), board 4 a single piece; (64, 41): 23 padding rows, which are
    empty boards; (544, 530): more rows than CUs, so the persistent workgroups loop (2 or 3 boards each, the LDS
    codes / maxima / exponents reused from board to board). Digits, exponents and the bytes behind the lines
    (untouched) equal in both forms."""
    rng = np.random.default_rng(700 + rows + nb)
    codes = rng.integers(1, 13, size=(nb, 64)).astype(np.int8)
    codes[rng.random((nb, 64)) < 0.5] = 0
    codes[3] = 0
    codes[4] = 0
    codes[4, 27] = 5
    wT = (rng.standard_normal((9, 12, 256)) * 0.2).astype(np.float32)
    scale = (0.5 + rng.random(256)).astype(np.float32)
    scale[::7] *= np.float32(2.0 ** -12)  # channels far below the row max
    shift = -np.abs(rng.standard_normal(256) * 0.05).astype(np.float32)  # an empty board: ReLU(shift) = 0
    df, tf, ef = _front(codes, rows, wT, scale, shift, 1)
    ds, ts, es = _front(codes, rows, wT, scale, shift, 0)
    assert np.array_equal(ef, es)
    assert np.array_equal(df, ds)
    assert (tf == 0x55).all() and (ts == 0x55).all()  # nothing written behind the 96-byte lines
    assert (ef[:, 3] == 0).all() and not df[:, :, 3].any()  # the empty board
    assert (ef[:, nb:] == 0).all() and not df[:, :, nb:].any()  # padding rows
    assert df[:, :, 4].any() and len(np.unique(ef[:, 4])) > 3  # the single piece: few nonzero pixels, rows that vary
    assert len(np.unique(ef)) > 3 and df.any(axis=(0, 1, 3, 4))[np.r_[0:3, 4:nb]].all()  # exponents vary across rows


def _back_inputs(rows, seed):
    """M, scale, shift, residual as the fused output kernel's tests take them (tests/test_wino_i8_gpu.py
    _out_inputs): board 5 all zero after the ReLU (M = 0, residual 0, shift <= 0), every 7th channel 2^-12 below the
    others, the two 256-channel halves 2^-5 apart. The heads' parameters are random, the head convs' BN shifts of
    both signs (so the ReLU cuts some features and keeps others)."""
    rng = np.random.default_rng(seed)
    M = (rng.standard_normal((100, rows, 512)) * 0.3).astype(np.float32)
    M[:, 5, :] = 0.0
    scale = (0.5 + rng.random(512)).astype(np.float32)
    scale[::7] *= np.float32(2.0 ** -12)
    scale[256:] *= np.float32(2.0 ** -5)
    shift = -np.abs(rng.standard_normal(512) * 0.1).astype(np.float32)
    R = (np.abs(rng.standard_normal((rows, 64, 512))) * 0.5).astype(np.float32)
    R[5] = 0.0
    heads = np.concatenate([
        (rng.standard_normal(3 * 512) * 0.05).astype(np.float32),   # policy_conv (2) and value_conv weights
        # their folded BN scale: 2^-12, as the output transform of a random M gives activations of 1e3 - 1e4
        # (at scale 1 every value but board 5's saturates to +-1)
        ((0.5 + rng.random(3)) * 2.0 ** -12).astype(np.float32),
        np.array([0.05, -0.05, 0.02], dtype=np.float32),            # and shift
        (rng.standard_normal(512 * 64) * 0.1).astype(np.float32),   # value_fc1 weight [512][64]
        (rng.standard_normal(512) * 0.1).astype(np.float32),        # bias
        (rng.standard_normal(512) * 0.05).astype(np.float32),       # value_fc2 weight
        np.array([0.01], dtype=np.float32)])                        # bias
    return M, scale, shift, R, heads


def _back(M, scale, shift, R, heads, fused):
    from knightvision_amd import _lib
    L = _lib.lib()
    rows = M.shape[1]
    pfeat = np.full((rows, 128), np.nan, dtype=np.float32)
    value = np.full(rows, np.nan, dtype=np.float32)
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    _lib.check(L.kv_dev_tower_back(0, P(M), rows, P(scale), P(shift), P(R), P(heads), int(fused), P(pfeat), P(value)),
               "kv_dev_tower_back")
    return pfeat, value


@pytest.mark.parametrize("rows,form", [(32, 1), (128, 1), (128, 3)])
def test_last_output_kernel_with_heads_equals_out_kernel_then_heads(rows, form):
    """form 3: the residual read non-temporally, as the tower runs the kernel at 1,024+ boards."""
    M, scale, shift, R, heads = _back_inputs(rows, 900 + rows)
    pf, vf = _back(M, scale, shift, R, heads, form)
    ps, vs = _back(M, scale, shift, R, heads, 0)
    assert np.array_equal(pf.view(np.uint32), ps.view(np.uint32))
    assert np.array_equal(vf.view(np.uint32), vs.view(np.uint32))
    assert np.isfinite(pf).all() and np.isfinite(vf).all()  # every board's row was written
    # board 5's activation is all zero: its features are the ReLU of the head convs' BN shifts alone
    hb = heads[3 * 512 + 3:3 * 512 + 6]
    assert (pf[5, :64] == max(hb[0], 0)).all() and (pf[5, 64:] == max(hb[1], 0)).all()
    # the others' are not: features both cut and kept by the ReLU, values that differ from board to board
    rest = np.delete(pf, 5, axis=0)
    assert (rest > 0).mean() > 0.2 and (rest == 0).mean() > 0.05
    assert len(np.unique(vf)) > rows // 2 and (np.abs(vf) < 1).all()
