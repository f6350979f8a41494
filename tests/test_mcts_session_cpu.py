"""The plain-Python restatement of search sessions (tests/_mcts_session.py)
against its own invariants and against the restated position search
(tests/_mcts_search.py), under the hash evaluator and under the non-uniform
synthetic one, where a carried root's leaf priors and a fresh root's differ in
bits; no GPU."""
import numpy as np
import pytest

from tests import _mcts_search as S
from tests import _mcts_session as SS


def _first_unvisited(r):
    return r["visits"].index(0) if 0 in r["visits"] else -1


@pytest.mark.parametrize("leaves", [1, 8])
def test_session_invariants_on_hash_positions(leaves):
    """Three plies of search -> advance(best) -> resume on the 18 positions: the root visits sum to sims after
    every continue, kept is the played edge's visits - 1, and a carried root keeps that edge's subtree."""
    sims = 48
    ses = SS.Session([s for s, _ in S.hash_positions()])
    rows = ses.search(sims, leaves)
    for _ in range(3):
        assert all(sum(r["visits"]) == sims == r["sims"] for r in rows)
        best = [r["best"] for r in rows]
        played = [r["visits"][b] for r, b in zip(rows, best)]
        sizes = [ses.tree_size(i) for i in range(len(rows))]
        ses.advance(best)
        for i in range(len(rows)):  # the root's node goes, and every sibling subtree with it
            nodes, edges = ses.tree_size(i)
            assert 1 <= nodes < sizes[i][0] and edges < sizes[i][1] and edges % 16 == 0
            assert nodes <= played[i]  # an expansion per visit at the most
        rows, kept = ses.resume(sims, leaves)
        assert kept == [n - 1 for n in played]
        for r, k in zip(rows, kept):
            assert r["nn_rows"] <= sims - k and sum(r["accepted"]) == sims - k
            assert len(r["visits"]) == len(r["moves"]) and r["pv"][0] == r["moves"][r["best"]]


def test_session_node_count_stays_within_sims_on_a_long_line():
    """30 plies of one game at 64 visits, L = 8: a tree never holds more than sims + 1 nodes, which is what
    keeps a session inside the engine's pools at any game length."""
    sims = 64
    ses = SS.Session([S.hash_positions()[0][0]])
    row = ses.search(sims, 8)[0]
    for ply in range(30):
        if row["status"] != SS.SEARCHED:
            break
        assert sum(row["visits"]) == sims
        assert ses.tree_size(0)[0] <= sims + 1, ply
        ses.advance([row["best"]])
        (row,), _ = ses.resume(sims, 8)
    assert ply >= 10


@pytest.mark.parametrize("leaves", [1, 8])
def test_unvisited_edge_then_continue_equals_search_of_the_state_after(leaves):
    """A dropped tree is searched exactly as a given position: every field of the restated kv_search. The
    first search is 8 visits, so that every root still has an edge without one."""
    sims = 48
    pos = [s for s, _ in S.hash_positions()[::3]] + [S.MATE_IN_ONE, S.KPK_CAPTURE]
    ses = SS.Session(pos)
    rows = ses.search(8, leaves)
    edges = [_first_unvisited(r) for r in rows]
    assert all(e >= 0 for e in edges[:-2])
    after = ses.advance(edges)
    got, kept = ses.resume(sims, leaves)
    assert kept == [0 if e >= 0 else 8 for e in edges]  # a tree left alone (-1) keeps its 8 visits
    for st, g, e in zip(after, got, edges):
        if e < 0:
            continue
        ref = S.search(st, sims, leaves, ncap=ses.ncap)
        assert set(ref) <= set(g)
        for key in ref:
            a, b = g[key], ref[key]
            if key in ("q", "prior"):
                a, b = np.array(a, dtype=np.float32).view(np.uint32).tolist(), \
                    np.array(b, dtype=np.float32).view(np.uint32).tolist()
            assert a == b, key


def _bits(a):
    return np.array(a, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("leaves", [1, 8])
def test_synthetic_dropped_tree_resumes_as_a_search_of_the_state_after(leaves):
    """Non-uniform priors: a dropped tree's root takes fresh root priors (k_mcts_root's), every field of the
    restated kv_search of the state after the move, prior bits included."""
    sims, ev = 48, S.synthetic_eval_many
    pos = [s for s, _ in S.synthetic_positions()[::3]] + [S.MATE_IN_ONE, S.KPK_CAPTURE]
    ses = SS.Session(pos, evaluate=ev)
    rows = ses.search(8, leaves)
    edges = [_first_unvisited(r) for r in rows]
    assert all(e >= 0 for e in edges[:-2])
    after = ses.advance(edges)
    got, kept = ses.resume(sims, leaves)
    assert kept == [0 if e >= 0 else 8 for e in edges]
    for st, g, e in zip(after, got, edges):
        if e < 0:
            continue
        ref = S.search(st, sims, leaves, ncap=ses.ncap, evaluate=ev)
        assert set(ref) <= set(g) and len(set(_bits(ref["prior"]))) > 1
        for key in ref:
            a, b = g[key], ref[key]
            if key in ("q", "prior"):
                a, b = _bits(a), _bits(b)
            assert a == b, key


@pytest.mark.parametrize("leaves", [1, 8])
def test_synthetic_carried_root_keeps_its_leaf_priors(leaves):
    """A zero-step resume(1) of a carried tree returns the played child's edge counts and the leaf priors it
    was expanded with; those are not the priors a fresh root of the same position gets (softmax over the
    legal logits in float against the 4,096-way softmax renormalised in double), so a session that rebuilt
    them, or a search that gave a dropped tree leaf priors, would show."""
    ev = S.synthetic_eval_many
    states = [s for s, _ in S.synthetic_positions()]
    ses = SS.Session(states, evaluate=ev)
    prev = ses.search(48, leaves)
    best = [r["best"] for r in prev]
    children = [t.root.child[b] for t, b in zip(ses.trees, best)]
    after = ses.advance(best)
    zero, kept = ses.resume(1, leaves, evaluate=None)  # no step runs: the evaluator is never asked
    differ = 0
    for i, (z, p, ch) in enumerate(zip(zero, prev, children)):
        assert ch is not None and p["visits"][best[i]] > 1, i
        assert z["steps"] == 0 and z["nn_rows"] == 0 and z["accepted"] == []
        assert z["visits"] == list(ch.N) and sum(z["visits"]) == kept[i] == p["visits"][best[i]] - 1 == z["sims"]
        assert z["moves"] == ch.words and z["root_value"] == ch.value == S.hash_value(ch.state[:64])
        want = S.leaf_priors(S.synthetic_logits(ch.state[:64]), ch.words)
        assert _bits(z["prior"]) == _bits(want), i
        fresh = S.search(after[i], 1, 1, evaluate=ev)
        assert fresh["moves"] == z["moves"] and fresh["root_value"] == z["root_value"]
        assert np.allclose(fresh["prior"], z["prior"], rtol=1e-5, atol=0)  # the same distribution...
        differ += _bits(fresh["prior"]) != _bits(z["prior"])  # ...in other bits
    print(f"L = {leaves}: {differ} of {len(states)} carried roots differ in bits from the fresh root's priors")
    assert differ >= 1
    rows, kept2 = ses.resume(48, leaves)
    assert kept2 == kept
    for r, z in zip(rows, zero):
        assert sum(r["visits"]) == 48 and _bits(r["prior"]) == _bits(z["prior"])


def test_session_evaluator_may_change_from_call_to_call():
    """search and resume take the evaluator of their call: the session's own when none is given."""
    state = S.synthetic_positions()[4][0]
    ses = SS.Session([state], evaluate=S.synthetic_eval_many)
    a = ses.search(16, 4)[0]
    b = ses.search(16, 4, evaluate=None)[0]
    assert a["visits"] == S.search(state, 16, 4, evaluate=S.synthetic_eval_many, ncap=ses.ncap)["visits"]
    assert b["visits"] == S.search(state, 16, 4, ncap=ses.ncap)["visits"] and _bits(b["prior"]) != _bits(a["prior"])
    asked = []

    def counting(states):
        asked.append(len(states))
        return S.synthetic_eval_many(states)

    ses.advance([b["best"]])
    (r,), (kept,) = ses.resume(16, 4, evaluate=counting)
    assert sum(r["visits"]) == 16 and sum(asked) == r["nn_rows"] == 16 - kept and max(asked) <= 4


def test_moves_into_terminal_positions_drop_the_tree():
    mate = SS.Session([S.MATE_IN_ONE])
    row = mate.search(48, 1)[0]
    words = row["moves"]
    k = words.index(S.sq("a1") | (S.sq("a8") << 6))  # Ra8#
    mate.advance([k])
    (r,), kept = mate.resume(48, 1)
    assert (r["status"], kept, r["root_value"], mate.tree_size(0)) == (SS.CHECKMATED, [0], 1.0, (0, 0))
    with pytest.raises(IndexError):
        mate.advance([0])  # a root that is not searched has no edge
    kk = SS.Session([S.KPK_CAPTURE])
    row = kk.search(48, 1)[0]
    k = row["moves"].index(S.sq("e5") | (S.sq("e4") << 6) | (8 << 12))  # ...Kxe4
    kk.advance([k])
    assert kk.resume(48, 1)[0][0]["status"] == SS.DRAW
