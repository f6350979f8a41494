"""The wide roots WIDE_A / WIDE_B / WIDE_C of tests/_mcts_search.py (found by tools/find_wide_positions.py):
the properties the GPU tests of tests/test_mcts_wide_gpu.py rely on, asserted on the plain-Python restatements
alone, so that a changed position cannot quietly leave the kernels' second and later 64-edge chunks unrun."""
import numpy as np
import pytest

from oracle import oracle as O

from tests import _mcts_search as S
from tests import _mcts_session as SS
from tests import _mcts_wide as W


def test_root_move_counts_and_no_root_move_ends_the_game():
    a, b, c = W.N_MOVES
    assert 65 <= a <= 128 and 129 <= b <= 192 and c > 192
    for st in W.WIDE:
        m3, after = O.valid_moves(st)
        assert not O.in_check(after)
        for k in range(len(m3)):
            nxt = O.make_valid_move(st, k)
            assert not O.is_draw(nxt) and len(O.valid_moves(nxt)[0]) > 0, k  # a mate in one soaks up every visit


@pytest.fixture(scope="module")
def trees():
    """{(i, L): (result, tree)} of the hash searches at 3 x n_moves visits."""
    out = {}
    for i, st in enumerate(W.WIDE):
        for leaves in (1, 8):
            ses = SS.Session([st], ncap=W.MAX_SIMS + 2)
            out[i, leaves] = (ses.search(3 * W.N_MOVES[i], leaves)[0], ses.trees[0])
    return out


def test_hash_searches_reach_the_later_chunks(trees):
    for (i, leaves), (r, tree) in trees.items():
        assert any(v > 0 for v in r["visits"][64:]), (i, leaves)
        if i > 0:
            assert any(v > 0 for v in r["visits"][128:]), (i, leaves)
    assert any(r["best"] >= 64 for r, _ in trees.values())
    below = [len(nd.words) for _, tree in trees.values() for nd in tree.nodes() if nd is not tree.root]
    assert max(below) > 64


def test_session_restatement_equals_search_restatement(trees):
    """The two restatements share the scoring loop: the same call gives the same result."""
    r, _ = trees[1, 8]
    ref = S.search(W.WIDE[1], 3 * W.N_MOVES[1], 8)
    for f in ("visits", "moves", "best", "pv", "steps", "nn_rows", "accepted", "sims"):
        assert r[f] == ref[f], f
    assert np.array(r["q"]).tobytes() == np.array(ref["q"]).tobytes()


def test_session_has_the_four_kinds_of_edge():
    """An edge whose child has more than 64 edges (the pack's j0 loop on a kept block), a visited edge at 64 or
    above, the best edge and an unvisited one, in the trees the GPU session test advances."""
    ses = SS.Session(W.SESSION_STATES, ncap=W.SESSION_SIMS + 2)
    ses.search(W.SESSION_SIMS, 8)
    e = W.session_edges(ses)
    roots = [t.root for t in ses.trees]
    assert W.child_edges(roots[0], e[0]) > 64 and roots[0].N[e[0]] > 0
    assert e[1] >= 64 and roots[1].N[e[1]] > 0 and roots[1].child[e[1]] is not None
    assert roots[2].child[e[2]] is not None and roots[3].N[e[3]] == 0 and roots[3].child[e[3]] is None
    ses.advance(e)
    assert [ses.tree_size(i)[0] > 0 for i in range(4)] == [True, True, True, False]
