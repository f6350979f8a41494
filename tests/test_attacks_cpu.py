"""The whole attack set on the host: targets() (knightvision_amd/csrc/kv_movegen.h) is __host__ __device__, and
kv_host_attacks runs its host build over state vectors, so all 64 bits of squareUnderAttack are pinned without a
GPU against tests/golden/attacks.npz -- the reference's own answers for every state of movegen.npz and
movegen_wide.npz, before and after getValidMoves. The device build: tests/test_engine_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from knightvision_amd import _lib

from tests import _attack_classes as AC
from tests._attack_classes import SETS, differing, recorded


def test_the_fixture_holds_every_class_the_attack_set_special_cases(golden_dir):
    total = {c: 0 for c in AC.CLASSES}
    for _, states, att in recorded(golden_dir):
        for c, n in AC.count_classes(states, att).items():
            total[c] += n
    assert all(n > 0 for n in total.values()), total
    # the king-square bit the older tests compare is one of the 64: inCheck as the fixtures recorded it
    g = np.load(os.path.join(golden_dir, "movegen_wide.npz"))
    post, att = g["post_states"], np.load(os.path.join(golden_dir, "attacks.npz"))["movegen_wide_post"]
    ksq = np.where(post[:, 64] == 1, post[:, 65] * 8 + post[:, 66], post[:, 67] * 8 + post[:, 68]).astype(np.uint64)
    assert ((att >> ksq) & np.uint64(1)).astype(np.uint8).tolist() == g["in_check"].tolist()


def test_the_classes_are_told_apart():
    from tests._mcts_search import make_state, sq
    v = make_state({sq("e1"): 1, sq("e8"): 7, sq("a2"): 6, sq("h2"): 6, sq("c2"): 6, sq("c4"): 12}, False)
    # white attacks: a2 and h2 push once and twice, c2 once (c4 blocks the second), no diagonal onto empty squares
    att = sum(1 << sq(s) for s in ("a3", "a4", "h3", "h4", "c3", "d1", "d2", "e2", "f2", "f1"))
    got = AC.classes_of(v, att)
    assert got == {"pawn_file_a", "pawn_file_h", "push_attacks", "double_free", "double_blocked",
                   "diag_empty_not_attacked"}
    assert "diag_empty_not_attacked" not in AC.classes_of(v, att | sum(1 << sq(s) for s in ("b3", "d3", "g3")))


@pytest.mark.parametrize("which", range(len(SETS)))
def test_host_attacks_equal_the_reference_on_every_bit(golden_dir, which):
    name, states, want = recorded(golden_dir)[which]
    got = np.zeros(len(states), dtype=np.uint64)
    _lib.check(_lib.lib().kv_host_attacks(states.ctypes.data_as(C.POINTER(C.c_int8)), len(states),
                                          got.ctypes.data_as(C.POINTER(C.c_uint64))), "kv_host_attacks")
    assert np.array_equal(got, want), f"{name}: {differing(got, want)}"


def test_host_attacks_refuses_bad_arguments():
    L = _lib.lib()
    assert "kv_host_attacks" in _lib.EXPORTED
    assert L.kv_host_attacks(None, 1, None) == -1 and b"kv_host_attacks: bad arguments" in L.kv_last_error()
