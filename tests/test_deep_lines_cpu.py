"""CPU side of the deep-line tests (tests/_mcts_deep.py): from the references alone, the conditions without which
tests/test_deep_lines_gpu.py would pass vacuously -- the forced lines are forced, the restated searches descend
more than two full passes of a 64-lane loop, several such descents are in flight in one sim-step -- and the chain
from the Python restatements to the C oracle on these starts."""
import numpy as np
import pytest

from oracle import oracle as O

from tests import _mcts_deep as D
from tests import _mcts_search as S


@pytest.mark.parametrize("start", [D.CHAIN, D.CHAIN_BLACK], ids=["white", "black"])
def test_the_chain_has_one_legal_move_for_300_plies(start):
    vec, seen = np.array(start, dtype=np.int8), set()
    for ply in range(300):
        assert not O.is_draw(vec), ply
        moves3, st = O.valid_moves(vec)
        assert len(moves3) == 1 and not O.in_check(st), ply
        assert S.move_words(st, moves3)[0] >> 12 == 8, ply  # a plain king move
        seen.add(bytes(st[:65]))
        vec = O.make_valid_move(vec, 0)
    assert len(seen) == 4  # Ka1-b1-a1 against Kh8-g8-h8: the positions repeat with period 4


def test_chain_b_has_two_root_moves_and_the_pieces_named():
    assert len(O.valid_moves(D.CHAIN_B)[0]) == 2
    diff = {s: int(D.CHAIN_B[s]) for s in range(64) if D.CHAIN_B[s] != D.CHAIN[s]}
    assert diff == {S.sq("b5"): 6, S.sq("b7"): 12}
    codes = D.CHAIN[:64]
    assert sorted(int(c) for c in codes if c) == [1, 4] + [6] * 7 + [7, 10] + [12] * 7
    assert D.CHAIN[64] == 1 and D.CHAIN_BLACK[64] == 0 and np.array_equal(D.CHAIN[:64], D.CHAIN_BLACK[:64])


@pytest.mark.parametrize("leaves", [1, 4, 8])
def test_the_chain_search_descends_more_than_two_lane_passes(leaves):
    r = D.search_ref("CHAIN", leaves)
    assert D.deepest(r) >= 130  # > 2 x 64: every lane of a 64-strided path loop runs a second and a third pass
    assert D.deepest(r) == 160 and r["visits"] == [160] and len(r["pv"]) == 16
    # the second descent of a step always meets the leaf the first one holds: one accepted descent per step
    assert set(r["accepted"]) == {1} and r["steps"] == 160
    assert [d for step in r["depths"] for d in step] == list(range(1, 161))


def test_chain_b_holds_several_deep_descents_in_flight():
    r = D.search_ref("CHAIN_B", 4)
    assert D.deepest(r) >= 130
    assert D.steps_with_two_deep(r) >= 10
    assert {1, 2, 3, 4} <= set(r["accepted"])
    assert len(r["visits"]) == 2 and min(r["visits"]) > 64
    for leaves in (1, 8):
        assert D.deepest(D.search_ref("CHAIN_B", leaves)) >= 130
    assert D.steps_with_two_deep(D.search_ref("CHAIN_B", 8)) >= 10


def test_the_synthetic_evaluator_never_has_two_deep_descents_in_flight():
    """Why the hash evaluator carries the in-flight condition: with non-uniform priors the search of CHAIN_B goes
    deeper still, but its steps never hold two descents deeper than 64."""
    r = S.search(D.CHAIN_B, 400, 4, evaluate=S.synthetic_eval_many, depths=True)
    assert D.deepest(r) >= 130 and D.steps_with_two_deep(r) == 0


def test_the_depths_field_changes_nothing():
    st = S.hash_positions()[3][0]
    a, b = S.search(st, 48, 8), S.search(st, 48, 8, depths=True)
    assert "depths" not in a and [len(x) for x in b.pop("depths")] == a["accepted"]
    assert {k: (np.array(v).tobytes() if k in ("q", "prior") else v) for k, v in a.items() if k != "root_value"} == \
        {k: (np.array(v).tobytes() if k in ("q", "prior") else v) for k, v in b.items() if k != "root_value"}
    assert a["root_value"] == b["root_value"]


@pytest.mark.parametrize("name", ["CHAIN", "CHAIN_B"])
def test_the_one_leaf_restatement_is_the_oracle_on_the_deep_starts(name):
    want = D.oracle_games(name)
    mine = D.leaves_games(name, 1)
    assert len(mine) >= 1
    for g, p in enumerate(mine):
        r = want[g]
        assert [x["move"] for x in p] == r["moves"].tolist(), g
        for x, v in zip(p, r["visits"]):
            n = int((v >= 0).sum())
            assert x["visits"] == v[:n].tolist(), g
        assert p.result[:3] == (r["plies"], r["outcome"], r["reason"]) == (D.MAX_MOVES, 0, 0), g
        assert len(p) + sum(sum(map(sum, x["leaf_pending"])) for x in p) == r["n_evals"], g
    if name != "CHAIN":
        return
    # ... and so are the one-leaf restatements the carried-tree and arena comparisons rest on, with those off
    from tests import _mcts_arena as AR
    from tests import _mcts_selfplay_reuse as RU
    r = want[0]
    p = RU.play(D.SEED, D.SIMS[name], None, False, **D._kw(name, 0))
    assert [x["move"] for x in p] == r["moves"].tolist() and \
        [x["visits"] for x in p] == [v[:int((v >= 0).sum())].tolist() for v in r["visits"]]
    p = AR.play(D.SEED, 0, D.SIMS[name], None, AR.hash_eval, AR.hash_eval, **D._kw(name, 0))
    assert [x["move"] for x in p] == r["moves"].tolist() and \
        [x["visits"] for x in p] == [v[:int((v >= 0).sum())].tolist() for v in r["visits"]]


@pytest.mark.parametrize("name", ["CHAIN", "CHAIN_B"])
def test_the_carried_trees_sit_at_the_edge(name):
    """reuse_tree: from ply 1 on a root carried down the chain holds sims - 1 visits (rem 1); with fast plies a
    carried root holds far more than the fast target (rem 0)."""
    games = D.reuse_games(name)
    if name == "CHAIN":
        for p in games:
            assert [(x["kept"], x["rem"]) for x in p] == [(0, 160)] + [(159, 1)] * 5
            assert all(x["played_n"] - 1 == y["kept"] for x, y in zip(p, p[1:]))
    assert any(x["rem"] == 1 and x["kept"] == D.SIMS[name] - 1 for p in games for x in p)
    fast = [x for p in D.pcr_reuse_games(name) for x in p if not x["full"]]
    full = [x for p in D.pcr_reuse_games(name) for x in p if x["full"]]
    assert fast and full and sum(x["rem"] == 0 and x["kept"] > 64 for x in fast) >= 2


def test_the_sizes_of_the_position_search_call():
    """kv_search takes one visit count per call: CHAIN beside CHAIN_B is searched at CHAIN_B's 400."""
    r = D.search_ref("CHAIN", 4, 400)
    assert D.deepest(r) == 400 and set(r["accepted"]) == {1} and len(r["pv"]) == 16


def test_the_cache_run_repeats_its_positions():
    """CHAIN's positions repeat with period 4, so behind a cache most leaves of a search are hits on entries an
    earlier ply -- or the other game, which plays the same line -- stored. Every move is forced, and one descent
    is accepted per step, so the games are the one-leaf oracle's."""
    games, info, table = D.cached_games()
    for p, r in zip(games, D.oracle_games("CHAIN")):
        assert [x["move"] for x in p] == r["moves"].tolist() and [x["visits"] for x in p] == [[160]] * D.MAX_MOVES
        assert max(max(x["accepted"]) for x in p) == 1  # a chain: the second descent always collides
    assert table.probes == sum(info["pending"]) == 2 * D.MAX_MOVES * 160
    assert table.hits > table.probes // 2 and table.stores > 0 and table.hits + table.stores <= table.probes
    print(f"probes / hits / stores {table.probes} / {table.hits} / {table.stores}")
    assert table.stores <= 8  # the line from either start holds four keys; everything else is a hit


def test_a_root_edge_after_64_advances_carries_what_it_took_at_depth():
    """The long session of tests/test_deep_lines_gpu.py. The first search of CHAIN passes the edge at depth j
    160 - j times, always at depth j. After j advances that edge is the root edge; each call in between gave it
    one more visit. So from j = 64 on, more than half of the root edge's 160 visits, and a part of its W that is
    not 0, were written at depth 64 or deeper: a backup that skips or negates W there shows in q."""
    from tests import _mcts_session as SS
    sims, plies = D.SIMS["CHAIN"], 70
    ses = SS.Session([D.CHAIN], ncap=D.SIMS["CHAIN_B"] + 2)
    ses.search(sims, 4)
    node, first = ses.trees[0].root, []  # first[j]: (N, W) of the edge at depth j after the first search
    for j in range(plies + 1):
        first.append((node.N[0], node.W[0]))
        node = node.child[0]
    assert [n for n, _ in first] == [sims - j for j in range(plies + 1)]
    for j in range(1, plies + 1):
        ses.advance([0])
        (r,), (kept,) = ses.resume(sims, 4)
        assert kept == sims - 1 and r["visits"] == [sims] and r["q"][0] != 0, j
        if j >= 64:
            n_first, w_first = first[j]
            assert n_first > sims // 2 and w_first != 0, j
