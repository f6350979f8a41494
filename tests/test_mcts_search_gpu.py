"""kv_search (knightvision_amd/csrc/kv_search.hip) on the GPU.

* Hash test evaluator, L = 1: the unchanged oracle's root visit vectors of the
  positions of its own eps = 0 games, and its Dirichlet root at eps = 0.25.
* Hash, L in {2, 8, 64}: the plain-Python restatement of the virtual-loss
  search (tests/_mcts_search.py): visits, q bit for bit, principal variation,
  sim-steps and network rows.
* The real ChessNet at L = 1: the oracle with the HIP network's own rows of
  the batch class (tests/test_mcts_gpu.py's method); at L = 8 the properties
  that hold without a reference (the restatement with the network's rows at
  L > 1: tests/test_mcts_search_net_gpu.py).
* Terminal roots, errors, play.search_move."""
import ctypes as C

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import EVAL_HASH, PositionSearch, SelfPlayEngine, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_search as S

pytestmark = pytest.mark.gpu

CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class
SPECIAL = [S.ONE_MOVE, S.MATE_IN_ONE, S.KPK_CAPTURE]


@pytest.fixture(scope="module")
def hash_search():
    with PositionSearch(synthetic_state_dict(42, "init"), max_positions=18, max_sims=64,
                        eval_mode=EVAL_HASH) as ps:
        yield ps


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


def _check_against_oracle(rows, pos):
    for k, (row, (_, visits)) in enumerate(zip(rows, pos)):
        n = int((visits >= 0).sum())
        assert row["status"] == 0 and row["n_moves"] == n, k
        assert np.array_equal(row["visits"], visits), f"position {k}: {row['visits'][:n]} oracle {visits[:n]}"
        assert row["best"] == int(np.argmax(visits[:n])), k
        assert row["sims"] == visits[:n].sum()


def test_hash_l1_equals_oracle(hash_search):
    """18 positions in one call (the > 16-tree shape) and one of them alone."""
    from oracle import oracle as O
    pos = S.hash_positions()
    states = np.stack([s for s, _ in pos])
    rows = hash_search.search(states, 48)
    _check_against_oracle(rows, pos)
    assert (rows["steps"] == 48).all()
    for k in range(len(pos)):  # the root lists are kv_dev_valid_moves' words
        m3, st = O.valid_moves(pos[k][0])
        assert rows["moves"][k][:len(m3)].tolist() == S.move_words(st, m3)
    _check_against_oracle(hash_search.search(states[7:8], 48), pos[7:8])


def test_hash_l1_dirichlet_root_equals_oracle(hash_search):
    from oracle import oracle as O
    r = O.mcts_play_game(48, O.MT(42, "numpy"), O.MT(42, "python"), None, max_moves=1, c_puct=1.5)
    row = hash_search.search(O.initial_state()[None], 48, eps=0.25, seed=42)[0]
    assert np.array_equal(row["visits"], r["visits"][0])


@pytest.mark.parametrize("sims", [50, 64])
@pytest.mark.parametrize("leaves", [2, 8, 64])
def test_hash_multi_leaf_equals_restatement(hash_search, leaves, sims):
    """sims 50: the last step is short for L = 8; 64: exact for L = 64. 5 game positions, the one-legal-move
    root, a mate in one (terminal leaves re-visited inside a step), K+P vs K (a capture leaves kings only)."""
    states = [s for s, _ in S.hash_positions()[2::4]][:5] + SPECIAL
    rows = hash_search.search(np.stack(states), sims, leaves=leaves)
    for k, (row, st) in enumerate(zip(rows, states)):
        r = S.search(st, sims, leaves)
        n = len(r["visits"])
        tag = f"position {k} L {leaves} sims {sims}"
        assert row["n_moves"] == n and row["sims"] == sims, tag
        assert row["visits"][:n].tolist() == r["visits"] and (row["visits"][n:] == -1).all(), tag
        assert row["q"][:n].view(np.uint32).tolist() == np.array(r["q"], dtype=np.float32).view(np.uint32).tolist(), tag
        assert row["prior"][:n].view(np.uint32).tolist() == \
            np.array(r["prior"], dtype=np.float32).view(np.uint32).tolist(), tag
        assert row["pv"][:row["pv_len"]].tolist() == r["pv"], tag
        assert (row["steps"], row["nn_rows"], row["best"]) == (r["steps"], r["nn_rows"], r["best"]), tag
        assert row["root_value"] == r["root_value"] and row["best_q"] == r["q"][r["best"]], tag


def test_terminal_roots(hash_search):
    pos = S.hash_positions()
    states = np.stack([pos[3][0], S.CHECKMATED_ROOT, S.STALEMATE_ROOT, pos[11][0], S.KINGS_ONLY_ROOT])
    for leaves in (1, 8):
        rows = hash_search.search(states, 48, leaves=leaves)
        assert rows["status"].tolist() == [0, 1, 2, 0, 3]
        for k in (1, 2, 4):
            assert rows["n_moves"][k] == 0 and rows["nn_rows"][k] == 0 and rows["best"][k] == -1
            assert rows["sims"][k] == 0 and (rows["visits"][k] == -1).all() and rows["pv_len"][k] == 0
        assert rows["root_value"][[1, 2, 4]].tolist() == [1.0, 0.0, 0.0]  # black is mated: +1 for white
        assert rows["visits"][0][:rows["n_moves"][0]].sum() == 48
    _check_against_oracle(hash_search.search(states, 48)[[0, 3]], [pos[3], pos[11]])


def _hip_eval(sd, class_rows=CLASS_ROWS):
    """Oracle evaluator: the HIP network's row for one board, computed in a batch of class_rows copies (the
    search's batch class: 17 = the > 16-board Winograd class, 1 = the <= 16-board direct class)."""
    from knightvision_amd.model import KVNet
    net = KVNet(0, packed_from(sd))

    def ev(planes):
        planes = np.asarray(planes, dtype=np.float32).reshape(-1, 12, 64)
        n = planes.shape[0]
        codes = np.zeros((n, 64), dtype=np.int8)
        b, c, sq = np.nonzero(planes)
        codes[b, sq] = c + 1
        rows = torch.from_numpy(np.repeat(codes, class_rows, axis=0)).cuda()
        pol, val = net.forward_boards(rows)
        torch.cuda.synchronize()
        return pol.cpu().numpy()[::class_rows], val.cpu().numpy().reshape(-1)[::class_rows]

    return ev, net


@pytest.mark.parametrize("variant", ["init", "peaked"])
def test_network_l1_equals_oracle(net_search, variant):
    """The first 3 plies of 4 oracle games (64 sims, eps = 0) played with the HIP evaluator of the batch class:
    12 positions + 5 copies in one call (> 16 boards), and one position alone (<= 16 boards)."""
    sd = synthetic_state_dict(42, variant)
    ev, net = _hip_eval(sd)
    pos = S.oracle_positions(4, 3, 64, ev)
    net.close()
    assert len(pos) == 12
    pos = pos + pos[:5]
    ps = net_search(variant)
    _check_against_oracle(ps.search(np.stack([s for s, _ in pos]), 64), pos)
    ev1, net1 = _hip_eval(sd, class_rows=1)
    one = S.oracle_positions(1, 2, 64, ev1)
    net1.close()
    _check_against_oracle(ps.search(one[1][0][None], 64), one[1:2])


def test_network_multi_leaf_properties(net_search):
    """L = 8 on 4 positions (32 rows) with the real network."""
    from oracle import oracle as O
    ps = net_search("peaked")
    states = np.stack([s for s, _ in S.hash_positions()[1::5]][:4])
    rows = ps.search(states, 64, leaves=8)
    for row, st in zip(rows, states):
        n = row["n_moves"]
        assert row["status"] == 0 and row["visits"][:n].sum() == 64
        assert (np.abs(row["q"][:n]) <= 1.0).all() and abs(row["best_q"]) <= 1.0
        assert row["best"] == int(np.argmax(row["visits"][:n]))
        assert 8 <= row["steps"] <= 64 and 1 <= row["nn_rows"] <= 65
        assert 1 <= row["pv_len"] <= 16 and row["pv"][0] == row["moves"][row["best"]]
        cur = st
        for w in row["pv"][:row["pv_len"]]:  # every pv move is legal where it is played
            m3, after = O.valid_moves(cur)
            words = S.move_words(after, m3)
            assert int(w) in words
            cur = O.make_valid_move(cur, words.index(int(w)))
    again = ps.search(states, 64, leaves=8)
    assert again.tobytes() == rows.tobytes()  # the trees reset
    rev = ps.search(states[::-1].copy(), 64, leaves=8)
    assert rev[::-1].tobytes() == rows.tobytes()  # no dependence on the order in the call


def test_errors(hash_search):
    st = S.hash_positions()[0][0][None]
    with PositionSearch(synthetic_state_dict(42, "init"), max_positions=2, max_sims=64, eval_mode=EVAL_HASH,
                        tree_edge_cap=_lib.MAXM + 40) as ps:
        with pytest.raises(_lib.KVError, match="tree pool full"):
            ps.search(st, 64)
        assert ps.stats()["tree_overflows"] > 0
        with pytest.raises(_lib.KVError, match="either kv_run or kv_search"):
            _lib.check(_lib.lib().kv_run(ps.h, 1, -1), "kv_run")
    with SelfPlayEngine(synthetic_state_dict(42, "init"), slots=2, n_games=2, max_moves=1, sims=8,
                        eval_mode=EVAL_HASH) as eng:
        eng.run()
        p = _lib.SearchParams(sims=8, leaves=1, eps=0.0, alpha=0.3, seed=0)
        out = (_lib.SearchResult * 1)()
        rc = _lib.lib().kv_search(eng.h, st.ctypes.data_as(C.POINTER(C.c_int8)), 1, C.byref(p), out)
        assert rc == -1 and b"either kv_run or kv_search" in _lib.lib().kv_last_error()
    for kw in (dict(leaves=0), dict(leaves=65), dict(sims=65), dict(sims=0), dict(alpha=1.0), dict(alpha=0.0)):
        args = dict(sims=48)
        args.update(kw)
        with pytest.raises(_lib.KVError, match="kv_search"):
            hash_search.search(st, **args)
    with pytest.raises(_lib.KVError, match="positions"):
        hash_search.search(np.repeat(st, 19, axis=0), 48)
    before = hash_search.stats()
    hash_search.search(st, 48, leaves=4)
    after = hash_search.stats()
    assert after["sims"] - before["sims"] == 48 and after["nn_rows"] > before["nn_rows"]


def test_play_search_move(hash_search):
    from knightvision_amd.chess_engine import GameState
    from knightvision_amd.play import search_move
    gs = GameState()
    mv = search_move(gs, hash_search, sims=64, leaves=8)
    valid = gs.getValidMoves()
    row = hash_search.search(gs._state()[None], 64, leaves=8)[0]
    assert mv in valid and mv == valid[int(row["best"])]
    assert row["moves"][row["best"]] & 63 == mv.startRow * 8 + mv.startCol
