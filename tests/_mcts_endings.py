"""The termination rules of an MCTS self-play or arena game, restated in plain Python over the oracle's rules
(oracle/kv_oracle.c mg_move_start, mg_commit and mg_result; on the device k_movegen, commit_move and k_finish
in knightvision_amd/csrc/kv_engine.hip), for the restatements that play a game to its end instead of the
number of plies the device reports (tests/_mcts_selfplay_leaves.py, _mcts_selfplay_reuse.py, _mcts_arena.py
with plies=None):

  * a ply begins with getValidMoves; no legal move ends the game there (no_moves);
  * after a move, in this order: isDraw (kings only), resignation (more than 15 plies played and the value of
    the root row the move was searched from below -0.7; the side to move after the move wins), max_moves;
  * the result of a game that ended neither by the cap nor by resignation: mate (inCheck and no move), then
    stalemate, then kings only, else the reference's material branch (always a draw).

tests/test_starts_cpu.py pins these to the C oracle. Not a test module itself."""
import numpy as np

from oracle import oracle as O

REWARD = {1: float(np.float32(1.0)), 0: float(np.float32(0.2)), -1: float(np.float32(-1.0))}


class Played(list):
    """The per-ply dicts of a game (played to its end: result and holds are set). result: (plies, outcome,
    reason, reward); holds: the ply-steps the game keeps its engine slot -- one per ply, and one more when it ended with no legal move
    (k_movegen finds that in a ply-step of its own)."""
    result = None
    holds = None

    def __init__(self, *a):
        super().__init__(*a)
        self.extra = []  # per ply: what the restatement knows beyond the dict its callers compare


def no_moves(st):
    """(outcome, reason) of a game whose position `st` (after the ply's getValidMoves) has no legal move."""
    return final(st)


def final(vec):
    """mg_result for a game that ended neither by max_moves nor by resignation."""
    g = np.array(vec, dtype=np.int8)
    chk = O.in_check(g)
    moves, g = O.valid_moves(g)
    if chk and len(moves) == 0:
        return (-1 if g[64] else 1), 2
    if chk:  # the reference asks getValidMoves a second time
        moves, g = O.valid_moves(g)
    if len(moves) == 0:
        return 0, 3
    return 0, (4 if O.is_draw(g) else 5)


def after_move(vec, plies, root_value, max_moves):
    """mg_commit's checks once a move is made: None (the game goes on) or (outcome, reason). vec: the state
    after the move, plies: moves played so far, root_value: the value of the root row of the ply just played."""
    if O.is_draw(vec):
        return final(vec)
    if plies > 15 and np.float64(np.float32(root_value)) < -0.7:
        return (-1 if vec[64] else 1), 1
    if max_moves and plies >= max_moves:
        return 0, 0
    return None


def finish(out, plies, end, on_move):
    """Fill a Played list's result and holds."""
    outcome, reason = end
    out.result = (plies, outcome, reason, REWARD[outcome])
    out.holds = plies + (0 if on_move else 1)
    return out


def start_state(start):
    return O.initial_state() if start is None else np.array(start, dtype=np.int8).reshape(80)
