"""The root move words the engine keeps beside the root visit counts
(keep_root_visits = 2, SelfPlayEngine(keep_root_moves=True)): every row must be
the move list kv_dev_valid_moves generates for the record's full game state
(castling flags and en-passant square included, which the record's 64 board
codes do not carry), in the order the visit counts are in."""
import ctypes as C

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import SelfPlayEngine
from knightvision_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

SIMS = 16
KW = dict(slots=8, n_games=8, sims=SIMS, max_moves=6, seed=42)


@pytest.fixture(scope="module")
def run():
    with SelfPlayEngine(synthetic_state_dict(42, "init"), keep_root_moves=True, **KW) as eng:
        eng.run()
        out = dict(recs=eng.records(), games=eng.games(), visits=eng.root_visits(), moves=eng.root_moves(),
                   recs_dev=eng.records_device(), visits_dev=eng.root_visits_device(),
                   moves_dev=eng.root_moves_device())
        torch.cuda.synchronize()
    return out


def policy_index(w):
    return (w & 63) * 64 + ((w >> 6) & 63)


def test_rows_are_the_move_lists_of_the_replayed_games(run):
    from knightvision_amd.chess_engine import GameState
    recs, visits, moves = run["recs"], run["visits"], run["moves"]
    assert moves.dtype == np.uint16 and moves.shape == (len(recs), _lib.MAXM) == visits.shape and len(recs) > 0
    for g in range(8):
        gs = GameState()
        rows = np.flatnonzero(recs["game_id"] == g)
        assert list(recs["ply"][rows]) == list(range(len(rows)))
        for k in rows:
            words, _, _ = gs._device_moves()  # kv_dev_valid_moves(gs._state())
            legal = gs.getValidMoves()
            n = len(words)
            assert np.array_equal(moves[k, :n], words) and (moves[k, n:] == 0xffff).all(), (g, k)
            assert (visits[k, :n] >= 0).all() and (visits[k, n:] == -1).all()
            # the move played: its policy index is in the row with a visit, and the counts are the search's sims
            idx = policy_index(moves[k, :n].astype(np.int64))
            hit = np.flatnonzero(idx == recs["move"][k])
            assert len(hit) >= 1 and visits[k, hit].sum() >= 1
            assert visits[k, :n].sum() == SIMS
            gs.makeMove(legal[int(hit[0])])


def test_device_rows_equal_host_rows(run):
    from knightvision_amd.distributed import record_order
    order = record_order(run["recs_dev"])
    md = run["moves_dev"]
    assert md.dtype == torch.uint8 and md.shape == (len(run["recs"]), 2 * _lib.MAXM)
    got = md[order].cpu().numpy().view(np.uint16)
    assert np.array_equal(got, run["moves"])
    vd = run["visits_dev"][order].cpu().numpy().view(np.uint16)
    assert np.array_equal(np.where(vd == 0xffff, -1, vd.astype(np.int32)), run["visits"])
    recs_sorted = run["recs_dev"][order].cpu().numpy().reshape(-1).view(run["recs"].dtype)
    assert np.array_equal(recs_sorted, run["recs"])


def test_visits_only_engine_is_unchanged_and_refuses_the_moves(run):
    with SelfPlayEngine(synthetic_state_dict(42, "init"), keep_root_visits=True, **KW) as eng:
        eng.run()
        assert eng.cfg.keep_root_visits == 1
        assert np.array_equal(eng.records(), run["recs"]) and np.array_equal(eng.games(), run["games"])
        assert np.array_equal(eng.root_visits(), run["visits"])
        L = _lib.lib()
        n = C.c_size_t()
        buf = (C.c_uint16 * _lib.MAXM)()
        assert L.kv_root_moves(eng.h, buf, 1, C.byref(n)) == -1
        assert "keep_root_visits" in L.kv_last_error().decode()
        assert L.kv_root_moves_device(eng.h, None, 0, C.byref(n), None) == -1
        assert "keep_root_visits" in L.kv_last_error().decode()
    with SelfPlayEngine(synthetic_state_dict(42, "init"), keep_root_moves=True, **KW) as eng:
        assert eng.cfg.keep_root_visits == 2  # the move words imply the visits
