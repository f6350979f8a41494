"""The position search's CPU restatement (tests/_mcts_search.py) against the
unchanged oracle under the hash evaluator and under a non-uniform synthetic
one (visit vectors at L = 1, the Dirichlet root), the virtual-loss invariants
that hold for every L, the condition that the multi-leaf inputs tell a search
with mispaired logits rows from the right one, and the parts of kv_search that
need no GPU (argument checks, the struct mirror)."""
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


def _bits(a):
    return np.array(a, dtype=np.float32).view(np.uint32).tolist()


def test_synthetic_evaluator_is_what_it_says():
    st = O.valid_moves(O.initial_state())[1]
    lg, v = S.synthetic_eval(st)
    assert lg.dtype == np.float32 and lg.shape == (4096,) and v == S.hash_value(st[:64])
    assert (lg * 8 == np.round(lg * 8)).all() and lg.min() >= -4 and lg.max() < 4
    assert len(np.unique(lg)) == 64  # every level occurs: far from uniform
    other = S.synthetic_eval(O.valid_moves(S.MATE_IN_ONE)[1])[0]
    assert (other != lg).mean() > 0.9  # the board enters every logit
    pl, pv = S.synthetic_eval_planes(np.stack([O.encode_board(st), O.encode_board(S.MATE_IN_ONE)]))
    assert np.array_equal(pl[0], lg) and np.array_equal(pl[1], other) and pv[0] == v


def test_synthetic_l1_equals_oracle_visits():
    """Non-uniform priors at L = 1: the oracle's own games with the synthetic evaluator, 3 x 6 plies at 48
    sims, eps = 0; and the priors matter, the hash run of the same position visits other edges."""
    pos = S.synthetic_positions()
    assert len(pos) == 18
    for k, (state, visits) in enumerate(pos):
        r = S.search(state, 48, 1, evaluate=S.synthetic_eval_many)
        n = len(r["visits"])
        assert np.array_equal(visits[:n], r["visits"]) and (visits[n:] == -1).all(), k
        assert r["steps"] == 48 and r["best"] == int(np.argmax(visits[:n]))
        assert r["root_value"] == S.hash_value(O.valid_moves(state)[1][:64])
        assert len(set(_bits(r["prior"]))) > 1, k
        assert S.search(state, 48, 1)["visits"] != r["visits"], k


def test_synthetic_l1_dirichlet_root_equals_oracle():
    """The noisy root (eps = 0.25, the oracle's default) over non-uniform logits, from the stream seeded 42."""
    for ev_planes, ev in ((S.synthetic_eval_planes, S.synthetic_eval_many), (None, None)):
        r = O.mcts_play_game(48, O.MT(42, "numpy"), O.MT(42, "python"), ev_planes, max_moves=1)
        s = S.search(O.initial_state(), 48, 1, evaluate=ev, eps=0.25, seed=42)
        n = len(s["visits"])
        assert np.array_equal(r["visits"][0][:n], s["visits"]) and (r["visits"][0][n:] == -1).all()
    assert S.search(O.initial_state(), 48, 1, evaluate=ev, eps=0.25, seed=43)["prior"] != s["prior"]


def test_hash_evaluator_given_explicitly_is_the_closed_form():
    """evaluate=None takes the closed forms of the all-zero row (1/n); the general path on hash_eval's rows
    (root_priors, leaf_priors) gives the same bits."""
    for state in [s for s, _ in S.hash_positions()[::7]] + [S.MATE_IN_ONE]:
        a, b = S.search(state, 48, 8), S.search(state, 48, 8, evaluate=S.hash_eval)
        assert set(a) == set(b)
        for key in a:
            assert (_bits(a[key]) == _bits(b[key])) if key in ("q", "prior") else a[key] == b[key], key


def test_rotated_logits_rows_change_the_search():
    """The teeth of the multi-leaf inputs, a condition on them: a search that gives each pending leaf of a
    step its neighbour's logits row (values kept) must not pass for the right one. 64 sims on the 18
    positions; at L = 64 collisions end most steps after a few descents, so few steps have two leaves."""
    syn, rot = S.synthetic_eval_many, S.rotated(S.synthetic_eval_many)
    for leaves in (2, 8, 64):
        differs = 0
        for state, _ in S.synthetic_positions():
            a, b = S.search(state, 64, leaves, evaluate=syn), S.search(state, 64, leaves, evaluate=rot)
            differs += a["visits"] != b["visits"] or _bits(a["q"]) != _bits(b["q"])
        print(f"L = {leaves}: rotated rows change {differs} of 18 searches")
        assert differs == 18 if leaves < 64 else differs >= 1, leaves
    state = S.synthetic_positions()[0][0]
    a, b = S.search(state, 64, 1, evaluate=syn), S.search(state, 64, 1, evaluate=rot)
    assert a["visits"] == b["visits"] and _bits(a["q"]) == _bits(b["q"])  # one row per step: nothing to rotate


@pytest.mark.parametrize("leaves", [2, 8, 64])
def test_synthetic_multi_leaf_invariants(leaves):
    """The 18 game positions and the three special ones. Under virtual loss a descent turns away from the
    edges in flight, so on the game positions (some 20 to 30 root moves) no step of L = 2 or 8 collides; the
    one-legal-move root collides at every L > 1 (its first step has one leaf to find), and at L = 64 every
    root with fewer than 64 moves does: the first step's descents all end on root edges."""
    sims = 64
    collided = []
    states = [s for s, _ in S.synthetic_positions()] + [S.ONE_MOVE, S.MATE_IN_ONE, S.KPK_CAPTURE]
    for state in states:
        r = S.search(state, sims, leaves, evaluate=S.synthetic_eval_many)
        assert sum(r["visits"]) == sims == sum(r["accepted"])
        assert r["steps"] >= -(-sims // leaves) and r["steps"] == len(r["accepted"])
        assert 1 <= r["nn_rows"] <= 1 + sims
        # a step accepts fewer descents than it may only when a collision ended it
        done = np.cumsum([0] + r["accepted"][:-1])
        collided.append(any(a < min(leaves, sims - d) for a, d in zip(r["accepted"], done)))
        assert len(r["visits"]) < 64
    print(f"L = {leaves}: a step collided in {sum(collided)} of {len(states)} searches")
    assert collided[18]  # the one-legal-move root
    assert leaves < 64 or all(collided)


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
