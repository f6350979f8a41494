"""Arena without a GPU: arena.summarize on hand-made game tables, the plain-Python restatement of an arena game
(tests/_mcts_arena.py) against the self-play restatement it must reduce to when both players share an evaluator,
and the ctypes mirrors of kv_config / kv_stats against the library's sizes."""
import ctypes as C
import math

import numpy as np
import pytest

from knightvision_amd import _lib, arena
from knightvision_amd.engine import GAME_DTYPE

from tests import _mcts_arena as AR
from tests import _mcts_selfplay_reuse as R


def _table(rows):
    """[(game_id, outcome (white-perspective), plies, reason)] -> GAME_DTYPE array."""
    t = np.zeros(len(rows), dtype=GAME_DTYPE)
    for k, (gid, outcome, plies, reason) in enumerate(rows):
        t[k] = (gid, plies, outcome, {1: 1.0, 0: 0.2, -1: -1.0}[outcome], reason, 0, 0)
    return t


def test_summarize_attributes_colour_by_id_parity():
    # A is white in the even ids: a white win there is A's, a white win in an odd id is B's
    t = _table([(0, 1, 10, 2), (1, 1, 12, 2), (2, -1, 14, 1), (3, -1, 16, 1), (4, 0, 20, 0), (7, 0, 24, 3)])
    s = arena.summarize(t)
    assert (s["games"], s["wins"], s["draws"], s["losses"]) == (6, 2, 2, 2)
    assert s["as_white"] == (1, 1, 1) and s["as_black"] == (1, 1, 1)
    assert s["score"] == 0.5 and s["elo"] == 0.0
    assert s["reasons"] == {"Checkmate": 2, "Resignation": 2, "max_moves": 1, "Stalemate": 1}
    assert s["mean_plies"] == 16.0
    lo, hi = s["score_ci95"]
    half = 1.96 * math.sqrt(np.var([1, 0, 0, 1, .5, .5], ddof=1) / 6)
    assert lo == pytest.approx(0.5 - half) and hi == pytest.approx(0.5 + half)


def test_summarize_all_wins_has_no_elo():
    s = arena.summarize(_table([(0, 1, 10, 2), (1, -1, 10, 2), (2, 1, 10, 2)]))
    assert (s["wins"], s["draws"], s["losses"]) == (3, 0, 0) and s["score"] == 1.0 and s["elo"] is None
    assert s["as_white"] == (2, 0, 0) and s["as_black"] == (1, 0, 0)
    s = arena.summarize(_table([(0, -1, 10, 2), (1, 1, 10, 2)]))
    assert s["score"] == 0.0 and s["elo"] is None and s["losses"] == 2
    s = arena.summarize(_table([]))
    assert s["games"] == 0 and s["score"] is None and s["elo"] is None


def test_summarize_three_wins_one_draw():
    s = arena.summarize(_table([(10, 1, 10, 2), (11, -1, 10, 2), (12, 0, 10, 0), (13, -1, 10, 1)]))
    assert (s["wins"], s["draws"], s["losses"]) == (3, 1, 0)
    assert s["score"] == 3.5 / 4
    assert s["elo"] == pytest.approx(-400.0 * math.log10(1.0 / 0.875 - 1.0)) and s["elo"] == pytest.approx(338.04, abs=0.01)
    lo, hi = s["score_ci95"]
    assert lo < 0.875 < hi <= 1.0 and s["elo_ci95"][0] < s["elo"]


def test_summarize_refuses_other_arrays():
    with pytest.raises(ValueError):
        arena.summarize(np.zeros(3))


@pytest.mark.parametrize("gid", [4, 5])
def test_same_evaluator_is_the_selfplay_restatement(gid):
    """Both players on one evaluator: the arena game is the self-play game without carried trees, ply for ply
    (visits, move words, move), and the players alternate from the id's parity."""
    seed, sims, plies = 49 + gid, 16, 6
    got = AR.play(seed, gid, sims, plies, R.hash_eval, R.hash_eval, eps=0.25)
    want = R.play(seed, sims, plies, False)
    assert len(got) == len(want) == plies
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["visits"] == w["visits"] and g["words"] == w["words"] and g["move"] == w["move"], p
        assert g["player"] == (p + gid) % 2 and g["sampled"]


def test_negated_opponent_plays_another_game():
    seed, sims, plies = 49, 16, 6
    got = AR.play(seed, 0, sims, plies, eps=0.25)  # B: the hash evaluator with the value negated
    want = R.play(seed, sims, plies, False)
    assert [g["player"] for g in got] == [0, 1, 0, 1, 0, 1]
    assert got[0]["visits"] == want[0]["visits"]  # A's first ply is the self-play ply
    assert any(g["visits"] != w["visits"] or g["words"] != w["words"] for g, w in zip(got, want))
    assert [g["visits"] for g in got[1::2]] != [w["visits"] for w in want[1::2]]  # (where B searched)


def test_sample_plies_takes_the_first_maximum():
    seed, sims, plies = 51, 16, 6
    drawn = AR.play(seed, 0, sims, plies, sample_plies=0)
    two = AR.play(seed, 0, sims, plies, sample_plies=2)
    none = AR.play(seed, 0, sims, plies, sample_plies=-1)
    assert [g["sampled"] for g in two] == [True, True] + [False] * 4 and not any(g["sampled"] for g in none)
    assert [(g["visits"], g["move"]) for g in two[:2]] == [(g["visits"], g["move"]) for g in drawn[:2]]
    for g in two[2:] + none:
        j = g["visits"].index(max(g["visits"]))
        assert g["move"] == AR.policy_index(g["words"][j])
    many = AR.play_many([seed, seed + 1], [0, 1], sims, [plies, 4], lambda s: [AR.hash_eval(x) for x in s],
                        lambda s: [AR.hash_eval_b(x) for x in s], sample_plies=2)
    assert many[0] == two and many[1] == AR.play(seed + 1, 1, sims, 4, sample_plies=2)


def test_mirror_sizes_match_the_library():
    L = _lib._declare(C.CDLL(_lib.LIB_PATH))  # (no GPU is touched)
    assert L.kv_sizeof_config() == C.sizeof(_lib.Config)
    assert L.kv_sizeof_stats() == C.sizeof(_lib.Stats)
    names = [n for n, _ in _lib.Config._fields_]
    assert names[-4:] == ["arena", "sample_plies", "sim_groups", "reuse_tree"]  # kv.h's order
    cfg = _lib.Config()  # a zeroed config is self-play with every ply drawn
    assert cfg.arena == 0 and cfg.sample_plies == 0
    assert dict(_lib.Stats._fields_)["arena_rows"] is C.c_int64 * 2
    for name in ("kv_load_weights_b", "kv_engine_calibration_b"):
        assert hasattr(L, name) and name in _lib.EXPORTED


def test_sim_groups_for_an_arena():
    from knightvision_amd.engine import sim_groups_for
    assert sim_groups_for(34, 16, 2, arena=True) == 2 and sim_groups_for(34, 16, 1, arena=True) == 1
    with pytest.raises(_lib.KVError):
        sim_groups_for(33, 16, 2, arena=True)
    auto = [sim_groups_for(s, 16, 0, arena=True) for s in (18, 256, 2048)]
    assert set(auto) <= {1, 2} and auto[0] == 1
