"""Match play between two weight sets inside the MCTS engine (kv_config.arena,
DESIGN.md "Arena"): the candidate-against-incumbent evaluation of an
AlphaZero-style loop, in place of the reference's play_vs_stockfish
(scripts/learn.py:204-206). Player A is the first weight set, player B the
second; in the game with global id g A plays white iff g is even, and every
ply is searched on the net of the side to move.

summarize() is pure numpy over the engine's game table; play_match() runs the
engine. Reporting only: nothing here gates or reverts a weight set.
"""
from __future__ import annotations

import math

import numpy as np

from .engine import GAME_DTYPE, REASONS


def summarize(games) -> dict:
    """A's result over a GAME_DTYPE array of arena games. kv_game.outcome is white-perspective (+1 white win,
    0 draw, -1 black win); A is white in the games with an even id. Returns
      games, wins / draws / losses (A's), as_white / as_black ((W, D, L) of A with that colour),
      score = (W + D/2) / N, elo = -400 log10(1 / score - 1) (None at score 0 or 1, and without games),
      score_ci95 = score -+ 1.96 sqrt(var / N) with var the per-game sample variance of A's points (1, 1/2, 0),
      clipped to [0, 1] (None below 2 games), elo_ci95 = the interval's ends as Elo (None where an end is 0 or 1),
      reasons {end reason: games}, mean_plies."""
    games = np.asarray(games)
    if games.dtype != GAME_DTYPE:
        raise ValueError("summarize: expected an array of engine.GAME_DTYPE")
    n = int(len(games))
    a_white = (games["game_id"] % 2) == 0
    res = np.where(a_white, games["outcome"], -games["outcome"]).astype(np.int64)  # +1 A won, 0 draw, -1 A lost

    def wdl(sel):
        r = res[sel]
        return int((r == 1).sum()), int((r == 0).sum()), int((r == -1).sum())

    w, d, l = wdl(np.ones(n, dtype=bool))
    out = {"games": n, "wins": w, "draws": d, "losses": l, "as_white": wdl(a_white), "as_black": wdl(~a_white),
           "score": None, "elo": None, "score_ci95": None, "elo_ci95": None,
           "reasons": {REASONS.get(int(r), str(int(r))): int(c)
                       for r, c in zip(*np.unique(games["reason"], return_counts=True))},
           "mean_plies": float(games["plies"].mean()) if n else 0.0}
    if n == 0:
        return out
    points = (res + 1) / 2.0
    score = float(points.mean())
    out["score"] = score
    out["elo"] = elo_of(score)
    if n >= 2:
        half = 1.96 * math.sqrt(float(points.var(ddof=1)) / n)
        lo, hi = max(0.0, score - half), min(1.0, score + half)
        out["score_ci95"] = (lo, hi)
        out["elo_ci95"] = (elo_of(lo), elo_of(hi))
    return out


def elo_of(score: float):
    """The Elo difference a score stands for, -400 log10(1 / score - 1); None at 0 and 1."""
    if not 0.0 < score < 1.0:
        return None
    return -400.0 * math.log10(1.0 / score - 1.0)


def play_match(weights_a, weights_b, games: int, *, sims: int, slots: int = 256, seed: int = 0, max_moves=None,
               eps: float = 0.0, alpha: float = 0.3, sample_plies: int = 8, c_puct: float = 1.5, device: int = 0,
               game_id_base: int = 0, game_id_stride: int = 1, precision: str = "fp32", algo: str = "auto",
               sim_groups: int = 0, eval_mode: int = 0, leaves: int = 0, eval_cache: int = 0) -> dict:
    """`games` games of A (weights_a) against B (weights_b) on one GPU -> summarize() of the game table, plus
    "game_table" (the GAME_DTYPE array, for a caller that sums several ranks) and "stats" (the engine's).
    eps = 0 by default: a match takes no root noise; the openings differ through the first `sample_plies`
    plies, which draw the move from the root visit counts on the per-game seeds (seed + id), after which every
    move is the most visited one (sample_plies=0: every ply drawn, -1: none). leaves > 1: that many descents in
    flight per game and sim-step (kv_config.leaves), which fills the network batches of a match of few games.
    eval_cache (leaves >= 2): entries of each net's exact leaf-row cache (kv_config.eval_cache; 0: off) -- the same
    games, fewer network rows ("stats" reports cache_hits)."""
    from .engine import SelfPlayEngine
    games = int(games)
    with SelfPlayEngine(weights_a, opponent=weights_b, slots=max(1, min(int(slots), games)), n_games=games, seed=seed,
                        max_moves=max_moves, eps=eps, alpha=alpha, sims=sims, c_puct=c_puct, device=device,
                        game_id_base=game_id_base, game_id_stride=game_id_stride, precision=precision, algo=algo,
                        sim_groups=sim_groups, sample_plies=sample_plies, eval_mode=eval_mode, leaves=leaves,
                        eval_cache=eval_cache) as eng:
        eng.run()
        table = eng.games()
        out = summarize(table)
        out["game_table"] = table
        out["stats"] = eng.stats()
        out["nn_path"] = (eng.calibration()["path_large"], eng.calibration_b()["path_large"])
    return out
