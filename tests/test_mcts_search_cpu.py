"""The position search's CPU restatement (tests/_mcts_search.py) against the
unchanged oracle, the virtual-loss invariants that hold for every L, and the
parts of kv_search that need no GPU (argument checks, the struct mirror)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

from tests import _mcts_search as S


def test_restatement_l1_equals_oracle_visits():
    """L = 1 is the self-play search: the visit vectors of 3 oracle games x 6 plies at 48 sims."""
    pos = S.hash_positions()
    assert len(pos) == 18
    for k, (state, visits) in enumerate(pos):
        r = S.search(state, 48, 1)
        n = len(r["visits"])
        assert np.array_equal(visits[:n], r["visits"]) and (visits[n:] == -1).all(), k
        assert r["steps"] == 48 and r["best"] == int(np.argmax(visits[:n]))


@pytest.mark.parametrize("leaves", [2, 8])
def test_restatement_multi_leaf_invariants(leaves):
    sims = 48
    for state, _ in S.hash_positions():
        r = S.search(state, sims, leaves)
        assert sum(r["visits"]) == sims
        assert r["steps"] >= -(-sims // leaves)
        assert 1 <= r["nn_rows"] <= 1 + sims


def test_one_legal_move_root_accepts_one_descent_per_step():
    moves, _ = O.valid_moves(S.ONE_MOVE)
    assert len(moves) == 1 and O.in_check(S.ONE_MOVE)
    for leaves in (2, 8):
        r = S.search(S.ONE_MOVE, 8, leaves)
        assert r["visits"] == [8] and sum(r["accepted"]) == 8
        # the first step's leaf is the one root edge itself: descent 1 finds it held and the step ends. From
        # the second step on the forced line is one ply long only -- the reply node has several edges, the
        # in-flight count turns descent 1 to another one, and the step accepts more than one descent
        assert r["accepted"][0] == 1
        assert all(1 <= a <= leaves for a in r["accepted"])
    r = S.search(S.ONE_MOVE, 1, 8)
    assert r["steps"] == 1 and r["visits"] == [1] and r["accepted"] == [1]


def test_special_positions_are_what_their_names_say():
    assert len(O.valid_moves(S.CHECKMATED_ROOT)[0]) == 0 and O.in_check(S.CHECKMATED_ROOT)
    assert len(O.valid_moves(S.STALEMATE_ROOT)[0]) == 0 and not O.in_check(S.STALEMATE_ROOT)
    assert O.is_draw(S.KINGS_ONLY_ROOT)
    assert [S.search(s, 4)["status"] for s in (S.CHECKMATED_ROOT, S.STALEMATE_ROOT, S.KINGS_ONLY_ROOT)] == [1, 2, 3]
    # a mate in one: some root move leaves black without a move, in check
    m, st = O.valid_moves(S.MATE_IN_ONE)
    after = [O.make_valid_move(st, j) for j in range(len(m))]
    assert any(len(O.valid_moves(a)[0]) == 0 and O.in_check(O.valid_moves(a)[1]) for a in after)
    # K+P vs K: some root move (the capture) leaves kings only
    m, st = O.valid_moves(S.KPK_CAPTURE)
    assert any(O.is_draw(O.make_valid_move(st, j)) for j in range(len(m)))


def test_kv_search_null_is_einval_without_a_gpu():
    from knightvision_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.kv_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.kv_last_error.restype = C.c_char_p
    p = _lib.SearchParams(sims=8, leaves=1, eps=0.0, alpha=0.3, seed=0)
    out = _lib.SearchResult()
    st = np.zeros(80, dtype=np.int8)
    assert L.kv_search(None, st.ctypes.data, 1, C.byref(p), C.byref(out)) == -1  # KV_EINVAL
    assert b"kv_search" in L.kv_last_error()


def test_search_result_mirror_has_the_library_size():
    from knightvision_amd import _lib
    from knightvision_amd.engine import SEARCH_DTYPE
    L = C.CDLL(_lib.LIB_PATH)
    L.kv_sizeof_search_result.restype = C.c_size_t
    assert L.kv_sizeof_search_result() == C.sizeof(_lib.SearchResult) == SEARCH_DTYPE.itemsize
    for name, _ in _lib.SearchResult._fields_:
        assert SEARCH_DTYPE.fields[name][1] == getattr(_lib.SearchResult, name).offset, name
