"""Search sessions (kv_search_advance / kv_search_continue,
knightvision_amd/csrc/kv_search.hip) on the GPU.

* Hash test evaluator: search -> advance -> resume lines against the
  plain-Python restatement (tests/_mcts_session.py): visits, q and prior bits,
  principal variation, sim-steps, network rows, kept visits, the states after
  the moves and the pool use of every tree.
* A dropped tree resumes exactly as kv_search searches the state after the
  move; a tree that already holds the visits runs no step; a long line stays
  inside the default pools; mixed edges in one call; errors.
* The real ChessNet: the properties that need no reference (the restatement
  with the network's rows: tests/test_mcts_search_net_gpu.py).
* play.SearchSession."""
import ctypes as C

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import EVAL_HASH, PositionSearch, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_search as S
from tests import _mcts_session as SS
from tests._mcts_compare import line as _line, same as _same, same_call as _same_call

pytestmark = pytest.mark.gpu

CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class
BEFORE_STALEMATE = S.make_state({S.sq("f7"): 1, S.sq("g1"): 2, S.sq("h8"): 7}, True)  # Qg6 stalemates


@pytest.fixture(scope="module")
def hash_search():
    with PositionSearch(synthetic_state_dict(42, "init"), max_positions=18, max_sims=64,
                        eval_mode=EVAL_HASH) as ps:
        yield ps


@pytest.mark.parametrize("leaves", [1, 8])
@pytest.mark.parametrize("which", ["all18", "one"])
def test_hash_line_equals_restatement(hash_search, which, leaves):
    """6 plies at 48 visits: 18 positions in one call (the > 16-tree shape) and one of them alone."""
    states = [s for s, _ in S.hash_positions()]
    if which == "one":
        states = states[7:8]
    _line(hash_search, states, [(48, leaves)] * 7)


def test_hash_line_short_last_step_and_changing_leaves(hash_search):
    states = [s for s, _ in S.hash_positions()[2::4]][:5] + [S.ONE_MOVE, S.MATE_IN_ONE, S.KPK_CAPTURE]
    _line(hash_search, states, [(50, 8)] * 4)                          # 50 visits: the last step is short
    _line(hash_search, states, [(48, 1), (48, 8), (48, 1), (64, 8)])   # leaves and sims differ from call to call


@pytest.mark.parametrize("leaves", [1, 8])
def test_dropped_tree_resumes_as_a_fresh_search(hash_search, leaves):
    """An edge without a visit, and moves into mate, stalemate and kings only: bit for bit kv_search of the
    states after the moves."""
    ps = hash_search
    states = [s for s, _ in S.hash_positions()[1::6]] + [S.MATE_IN_ONE, BEFORE_STALEMATE, S.KPK_CAPTURE]
    rows = ps.search(np.stack(states), 8, leaves=leaves)  # 8 visits leave every game root an unvisited edge
    edges = []
    for row in rows[:3]:
        n = row["n_moves"]
        assert (row["visits"][:n] == 0).any()
        edges.append(int(np.argmin(row["visits"][:n])))
    edges.append(rows["moves"][3].tolist().index(S.sq("a1") | (S.sq("a8") << 6)))               # Ra8#
    edges.append(rows["moves"][4].tolist().index(S.sq("g1") | (S.sq("g6") << 6)))               # Qg6 stalemate
    edges.append(rows["moves"][5].tolist().index(S.sq("e5") | (S.sq("e4") << 6) | (8 << 12)))   # ...Kxe4
    after = ps.advance(edges)
    assert [ps.tree_size(i) for i in range(6)] == [(0, 0)] * 6
    got, kept = ps.resume(48, leaves)
    assert kept.tolist() == [0] * 6 and got["status"].tolist() == [0, 0, 0, 1, 2, 3]
    fresh = ps.search(after, 48, leaves=leaves)
    assert got.tobytes() == fresh.tobytes()
    from oracle import oracle as O
    for st, k, a in zip(states, edges, after):
        assert np.array_equal(a, O.make_valid_move(st, k))


def test_zero_step_resume(hash_search):
    """A root that already holds the visits asked for runs no step: the result is the carried subtree."""
    ps = hash_search
    states = np.stack([s for s, _ in S.hash_positions()])
    prev = ps.search(states, 48, leaves=8)
    best = prev["best"].astype(np.int32)
    ps.advance(best)
    rows, kept = ps.resume(1, leaves=8)
    for i, (row, p) in enumerate(zip(rows, prev)):
        n = row["n_moves"]
        assert p["visits"][best[i]] > 1  # a well-visited edge
        assert row["steps"] == 0 and row["nn_rows"] == 0
        assert row["visits"][:n].sum() == kept[i] == p["visits"][best[i]] - 1 == row["sims"]
        if p["pv_len"] < 16:
            assert row["pv"][:row["pv_len"]].tolist() == p["pv"][1:p["pv_len"]].tolist(), i
    again, kept2 = ps.resume(1, leaves=1)
    assert again.tobytes() == rows.tobytes() and kept2.tolist() == kept.tolist()


def test_long_line_stays_inside_the_default_pools(hash_search):
    """30 plies at 64 visits (the engine's max_sims), L = 8: a re-root that only moved a pointer would run out
    of nodes after the second ply; the packed tree never holds more than sims + 1."""
    ps = hash_search
    row = ps.search(S.hash_positions()[0][0][None], 64, leaves=8)[0]
    plies = 0
    for _ in range(30):
        if row["status"] != 0:
            break
        assert ps.tree_size(0)[0] <= 65
        ps.advance([row["best"]])
        assert ps.tree_size(0)[0] <= 65
        rows, _ = ps.resume(64, leaves=8)  # KV_EOVERFLOW would raise
        row = rows[0]
        plies += 1
        if row["status"] == 0:
            assert row["visits"][:row["n_moves"]].sum() == 64
    assert plies >= 10 and ps.stats()["tree_overflows"] == 0


def test_mixed_edges_in_one_call(hash_search):
    """-1 for some trees, an unvisited edge for others, the best edge for the rest."""
    ps = hash_search
    states = [s for s, _ in S.hash_positions()]
    ses = SS.Session(states)
    prev = ps.search(np.stack(states), 16, leaves=4)
    ses.search(16, 4)
    edges = []
    for i, row in enumerate(prev):
        n = row["n_moves"]
        unvisited = np.flatnonzero(row["visits"][:n] == 0)
        edges.append(-1 if i % 3 == 0 or (i % 3 == 1 and len(unvisited) == 0) else
                     int(unvisited[0]) if i % 3 == 1 else int(row["best"]))
    assert sum(e >= 0 and prev["visits"][i][e] == 0 for i, e in enumerate(edges)) >= 3
    after = ps.advance(edges)
    assert np.array_equal(after, np.stack(ses.advance(edges)))
    rows, kept = ps.resume(16, leaves=4)
    ref, ref_kept = ses.resume(16, 4)
    assert kept.tolist() == ref_kept
    _same_call(ps, ses, rows, ref, "mixed")
    for i, e in enumerate(edges):
        if e >= 0:
            continue
        row, p = rows[i], prev[i]
        assert row["steps"] == 0 and row["nn_rows"] == 0 and kept[i] == 16
        for f in ("status", "n_moves", "sims", "best", "pv_len", "root_value", "best_q", "pv", "moves", "visits",
                  "q", "prior"):
            assert row[f].tobytes() == p[f].tobytes(), (i, f)


def test_errors(hash_search):
    ps = hash_search
    L = _lib.lib()
    with PositionSearch(synthetic_state_dict(42, "init"), max_positions=2, max_sims=64, eval_mode=EVAL_HASH) as new:
        with pytest.raises(_lib.KVError, match=r"\(-1\).*no session"):
            new.advance([0])
        with pytest.raises(_lib.KVError, match=r"\(-1\).*no session"):
            new.resume(48)
        with pytest.raises(_lib.KVError, match=r"\(-1\).*no session"):
            new.tree_size(0)
    states = np.stack([S.hash_positions()[3][0], S.CHECKMATED_ROOT, S.hash_positions()[11][0]])
    prev = ps.search(states, 48, leaves=8)
    with pytest.raises(_lib.KVError, match=r"\(-1\).*the session holds 3"):
        ps.advance([0, -1])
    ps._n = 2
    with pytest.raises(_lib.KVError, match=r"\(-1\).*the session holds 3"):
        ps.resume(48)
    ps._n = 3
    with pytest.raises(_lib.KVError, match=r"\(-1\).*whose root has"):
        ps.advance([0, -1, int(prev["n_moves"][2])])  # the good edge of tree 0 must not be played either
    with pytest.raises(_lib.KVError, match=r"\(-1\).*not searched"):
        ps.advance([-1, 0, -1])
    p = _lib.SearchParams(sims=48, leaves=8, eps=0.25, alpha=0.3, seed=0)
    out = (_lib.SearchResult * 3)()
    assert L.kv_search_continue(ps.h, 3, C.byref(p), out, None) == -1 and b"eps" in L.kv_last_error()
    with pytest.raises(_lib.KVError, match="kv_search_continue"):
        ps.resume(65)
    with pytest.raises(_lib.KVError, match="kv_search_continue"):
        ps.resume(48, leaves=65)
    # nothing changed: every tree resumes to its old result
    rows, kept = ps.resume(48, leaves=8)
    assert kept.tolist() == [48, 0, 48] and (rows["steps"] == 0).all()
    for f in ("status", "n_moves", "sims", "best", "pv_len", "root_value", "best_q", "pv", "moves", "visits", "q",
              "prior"):
        assert rows[f].tobytes() == prev[f].tobytes(), f
    before = ps.stats()
    ps.advance(prev["best"].astype(np.int32))
    rows, kept = ps.resume(48, leaves=8)
    after = ps.stats()  # the counters grow by the new backups and rows only
    assert after["sims"] - before["sims"] == int((48 - kept[[0, 2]]).sum())
    assert after["nn_rows"] - before["nn_rows"] == int(rows["nn_rows"].sum())


@pytest.fixture(scope="module")
def net_search():
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = PositionSearch(synthetic_state_dict(42, variant), max_positions=CLASS_ROWS, max_sims=64)
        return made[variant]

    yield get
    for ps in made.values():
        ps.close()


def _network_values(variant, boards, batch):
    """The HIP network's own value of every board, each from a forward of `batch` copies (the size of the
    search's leaf batches, so its batch class; tests/test_mcts_search_gpu.py's method)."""
    from knightvision_amd.model import KVNet
    net = KVNet(0, packed_from(synthetic_state_dict(42, variant)))
    out = []
    for b in boards:
        rows = torch.from_numpy(np.repeat(np.asarray(b, dtype=np.int8)[None], batch, axis=0)).cuda()
        _, val = net.forward_boards(rows)
        torch.cuda.synchronize()
        out.append(val.cpu().numpy().reshape(-1)[0])
    net.close()
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("leaves", [1, 8])
@pytest.mark.parametrize("variant", ["init", "peaked"])
def test_network_session_properties(net_search, variant, leaves):
    """17 positions with the real network: what holds without a reference."""
    from oracle import oracle as O
    ps = net_search(variant)
    states = np.stack([s for s, _ in S.hash_positions()[:17]])
    prev = ps.search(states, 48, leaves=leaves)
    best = prev["best"].astype(np.int32)
    after = ps.advance(best)
    carried = np.array([ps.tree_size(i)[0] > 0 for i in range(17)])
    assert carried.sum() >= 12
    zero, kept0 = ps.resume(1, leaves=leaves)  # the carried subtrees as they are
    boards = [O.valid_moves(a)[1][:64] for a in after]  # what the network saw: after getValidMoves
    values = _network_values(variant, boards, CLASS_ROWS * leaves)
    for i in np.flatnonzero(carried):
        n = zero["n_moves"][i]
        assert zero["steps"][i] == 0 and zero["visits"][i][:n].sum() == kept0[i] == prev["visits"][i][best[i]] - 1
        assert zero["root_value"][i] == values[i], i
        assert abs(float(zero["prior"][i][:n].astype(np.float64).sum()) - 1.0) <= 1e-5
        assert (zero["prior"][i][:n] >= 0).all()
    rows, kept = ps.resume(48, leaves=leaves)
    assert kept.tolist() == kept0.tolist()
    for i in range(17):
        n = rows["n_moves"][i]
        assert rows["status"][i] == 0 and rows["visits"][i][:n].sum() == 48 == rows["sims"][i]
        if carried[i]:
            assert rows["nn_rows"][i] == 48 - kept[i], i
            assert rows["prior"][i].tobytes() == zero["prior"][i].tobytes()
            assert rows["root_value"][i] == values[i]
        else:
            assert kept[i] == 0 and rows["root_value"][i] == values[i]


def test_play_search_session(hash_search):
    from knightvision_amd.chess_engine import GameState
    from knightvision_amd.play import SearchSession
    from oracle import oracle as O
    gs = GameState()
    game = SearchSession(gs, hash_search, sims=16, leaves=4)
    ses = SS.Session([O.initial_state()])
    for ply in range(8):
        mv = game.best_move()
        if ply == 0:
            ref, ref_kept = ses.search(16, 4)[0], 0
        else:
            (ref,), (ref_kept,) = ses.resume(16, 4)
        _same(game.row, ref, f"ply {ply}")
        assert game.kept == ref_kept
        valid = gs.getValidMoves()
        assert mv == valid[ref["best"]]
        game.push(mv)
        ses.advance([ref["best"]])
    # a move the search never visited: the tree starts fresh
    game.best_move()
    row = game.row
    k = int(np.flatnonzero(row["visits"][:row["n_moves"]] == 0)[0])
    game.push(gs.getValidMoves()[k])
    assert np.array_equal(gs._state(), O.make_valid_move(ses.trees[0].vec, k)[:80])
    game.best_move()
    assert game.kept == 0
    assert game.row.tobytes() == hash_search.search(gs._state()[None], 16, leaves=4)[0].tobytes()
