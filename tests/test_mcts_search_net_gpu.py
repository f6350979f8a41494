"""kv_search with several leaves in flight and search sessions with the real
ChessNet, against the plain-Python restatements (tests/_mcts_search.py,
tests/_mcts_session.py) given the HIP network's own rows: every field of every
tree, q and priors bit for bit, zero divergences.

Under the hash test evaluator every prior is 1/n, so a leaf paired with its
neighbour's logits row, a re-root that permuted priors inside a node, or a
dropped tree given leaf priors in place of fresh root priors passes every hash
test. Here the logits differ from row to row and from move to move.

The evaluator is KVNet.forward_boards in the batch class of the call restated
(the network is batch-invariant bit for bit inside a class, tests/test_nn_gpu.py):
a call of n trees at L leaves runs the > 16-board class when n * L > 16, its
root batch padded to 17 rows, and the <= 16-board class otherwise."""
import numpy as np
import pytest
import torch

from knightvision_amd.engine import PositionSearch, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_search as S
from tests import _mcts_session as SS
from tests._mcts_compare import line, same, same_call

pytestmark = pytest.mark.gpu

CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class
SPECIAL = [S.ONE_MOVE, S.MATE_IN_ONE, S.KPK_CAPTURE]
TERMINAL = [S.CHECKMATED_ROOT, S.STALEMATE_ROOT, S.KINGS_ONLY_ROOT]
_NETS, _SEARCHES = {}, {}


def _net(variant):
    from knightvision_amd.model import KVNet
    if variant not in _NETS:
        _NETS[variant] = KVNet(0, packed_from(synthetic_state_dict(42, variant)))
    return _NETS[variant]


def _ps(variant):
    if variant not in _SEARCHES:
        _SEARCHES[variant] = PositionSearch(synthetic_state_dict(42, variant), max_positions=CLASS_ROWS, max_sims=64)
    return _SEARCHES[variant]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for made in (_NETS, _SEARCHES):
        while made:
            made.popitem()[1].close()


def _hip_eval(variant, n, leaves):
    """The restatements' evaluator of a call of n trees at `leaves` leaves: the HIP network's rows of a list of
    positions (the board codes of the state vectors after getValidMoves), one forward in the call's class."""
    net = _net(variant)
    large = n * leaves > 16

    def ev(states):
        codes = np.stack([np.asarray(st[:64], dtype=np.int8) for st in states])
        k = len(codes)
        if large and k < CLASS_ROWS:
            codes = np.concatenate([codes, np.repeat(codes[:1], CLASS_ROWS - k, axis=0)])
        assert large or k <= 16
        pol, val = net.forward_boards(torch.from_numpy(np.ascontiguousarray(codes)).cuda())
        torch.cuda.synchronize()
        pol, val = pol.cpu().numpy(), val.cpu().numpy().reshape(-1)
        return [(pol[j], val[j]) for j in range(k)]

    return ev


def _game(*ks):
    pos = S.hash_positions()
    return [pos[k][0] for k in ks]


def _search_equals_restatement(variant, states, sims, leaves, eps=0.0, alpha=0.3, seed=0):
    ps = _ps(variant)
    ev = _hip_eval(variant, len(states), leaves)
    rows = ps.search(np.stack(states), sims, leaves=leaves, eps=eps, alpha=alpha, seed=seed)
    refs = []
    for i, (row, st) in enumerate(zip(rows, states)):
        r = S.search(st, sims, leaves, ncap=66, evaluate=ev, eps=eps, alpha=alpha, seed=seed + i)
        same(row, r, f"{variant} n {len(states)} L {leaves} sims {sims} position {i}")
        refs.append(r)
    return rows, refs


@pytest.mark.parametrize("variant", ["peaked", "init"])
def test_one_position_8_leaves(variant):
    """Case A: 8 rows, the <= 16-board class for the root and every leaf batch; 50 visits: the last step is
    short."""
    _, (r,) = _search_equals_restatement(variant, _game(7), 50, 8)
    assert sum(r["accepted"]) == 50 and len(set(r["prior"])) > 1


def test_two_positions_8_leaves():
    """Case B: 16 rows, the top of the <= 16-board class."""
    _search_equals_restatement("peaked", _game(3, 12), 64, 8)


@pytest.mark.parametrize("variant", ["peaked", "init"])
def test_three_positions_8_leaves(variant):
    """Case C: 24 rows, the > 16-board class; the root batch of 3 is padded to 17."""
    _search_equals_restatement(variant, _game(1, 8, 15), 64, 8)


def test_17_positions_2_leaves_specials_and_terminal_roots():
    """Case D: 34 rows; the one-legal-move root, mate in one, K+P vs K, and the three terminal roots in the
    middle of the call: their rows stay in every leaf batch with count 0."""
    states = _game(0, 2, 4, 6, 9) + SPECIAL[:2] + TERMINAL + SPECIAL[2:] + _game(10, 11, 13, 14, 16, 17)
    assert len(states) == 17
    rows, _ = _search_equals_restatement("peaked", states, 50, 2)
    assert rows["status"].tolist() == [0] * 7 + [1, 2, 3] + [0] * 7


def test_one_position_64_leaves():
    """Case E: one tree filling a 64-row batch; collisions end most steps early."""
    _, (r,) = _search_equals_restatement("peaked", _game(5), 64, 64)
    assert r["steps"] > 1 and max(r["accepted"]) > 1  # fewer than 64 root moves: the first step must collide


def test_dirichlet_roots_8_leaves():
    """Case F: noisy root priors (eps 0.25, alpha 0.3), position i from the stream seeded 42 + i."""
    states = _game(1, 8, 15)
    rows, refs = _search_equals_restatement("peaked", states, 64, 8, eps=0.25, alpha=0.3, seed=42)
    plain = _ps("peaked").search(np.stack(states), 64, leaves=8)
    assert all(a["prior"].tobytes() != b["prior"].tobytes() for a, b in zip(rows, plain))


def test_stress_weights_8_leaves():
    """Case G: logits of std 4 through AUTO's fp64-domain tower."""
    ps = _ps("stress")
    assert ps.calibration()["path_large"] in ("winograd88_i8r", "winograd88_i8")
    _search_equals_restatement("stress", _game(1, 8, 15), 64, 8)


@pytest.mark.parametrize("leaves", [1, 8])
@pytest.mark.parametrize("variant", ["peaked", "init"])
def test_session_line_17_trees(variant, leaves):
    """Case H: four calls at 48 visits: carried roots keep the leaf priors their nodes were expanded with, the
    re-root moves e_P with the edges."""
    states = _game(*range(14)) + SPECIAL
    line(_ps(variant), states, [(48, leaves)] * 4, lambda n, L: _hip_eval(variant, n, L))


def test_session_line_class_changes_from_call_to_call():
    """Case I: 3 trees at 1 leaf are 3 rows (<= 16-board class), at 8 leaves 24 (> 16): the evaluator follows
    the call, and nodes expanded in one class are searched on in the other."""
    line(_ps("peaked"), _game(2, 9, 16), [(48, 1), (48, 8), (48, 1), (64, 8)],
         lambda n, L: _hip_eval("peaked", n, L))


def test_session_fresh_and_carried_roots_in_one_call():
    """Case J: after 8 visits two trees play an edge without a visit (dropped: fresh root priors from
    k_mcts_root) and three their best edge (carried: leaf priors), and all resume in one call."""
    variant, states = "peaked", _game(0, 4, 8, 12, 16)
    ps, ses = _ps(variant), SS.Session(states)
    rows = ps.search(np.stack(states), 8, leaves=1)  # 5 rows: the <= 16-board class
    ref = ses.search(8, 1, evaluate=_hip_eval(variant, 5, 1))
    same_call(ps, ses, rows, ref, "search")
    edges = [r["visits"].index(0) if i in (1, 3) else r["best"] for i, r in enumerate(ref)]
    after = ps.advance(edges)
    assert np.array_equal(after, np.stack(ses.advance(edges)))
    sizes = [ses.tree_size(i) for i in range(5)]
    assert [ps.tree_size(i) for i in range(5)] == sizes
    assert [nodes > 0 for nodes, _ in sizes] == [True, False, True, False, True]  # carried / dropped
    ev = _hip_eval(variant, 5, 8)  # 40 rows: the > 16-board class
    rows, kept = ps.resume(48, 8)
    ref, ref_kept = ses.resume(48, 8, evaluate=ev)
    assert kept.tolist() == ref_kept and [ref_kept[i] for i in (1, 3)] == [0, 0]
    same_call(ps, ses, rows, ref, "resume")
    for i in (1, 3):  # a dropped tree is kv_search of the state after the move
        same(rows[i], S.search(after[i], 48, 8, ncap=66, evaluate=ev), f"fresh {i}")
