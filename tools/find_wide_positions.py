"""Seeded search for the wide search-test roots WIDE_A / WIDE_B / WIDE_C of tests/_mcts_search.py.

    python tools/find_wide_positions.py

Random boards with queens on both sides, white to move, judged with the oracle's rules and the plain-Python
search restatement under the hash evaluator (tests/_mcts_search.search). A board is taken for its band of root
move counts (65-128, 129-192, above 192) when the root is not in check, no root move mates or stalemates, and
a search of 3 x n_moves visits at one leaf visits an edge at index 64 or above (128 or above in the two wider
bands) and, in the two narrower bands, expands a child with more than 64 edges. Black's king sits walled in on
a1 so that no root move can check it; the widest band's boards are hill-climbed, as random ones stay below
193 moves. Prints the three piece dicts as make_state literals."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402
from tests import _mcts_search as S  # noqa: E402

BANDS = {"WIDE_A": (65, 128), "WIDE_B": (129, 192), "WIDE_C": (193, 320)}
QUEENS = {"WIDE_A": (5, 9), "WIDE_B": (11, 15), "WIDE_C": (22, 30)}
BLACK = {"WIDE_A": (3, 7), "WIDE_B": (3, 7), "WIDE_C": (2, 4)}


def wide_children(state):
    """Root edges whose position has more than 64 moves; None if a root move ends the game."""
    m3, _ = O.valid_moves(state)
    out = []
    for k in range(len(m3)):
        after = O.make_valid_move(state, k)
        if O.is_draw(after):
            return None
        n = len(O.valid_moves(after)[0])
        if n == 0:
            return None
        if n > 64:
            out.append(k)
    return out


def main():
    rng = random.Random(20240)
    sq = S.sq
    # black's king cannot be checked in one move: a1 behind its own pawns and bishop, those behind white pawns
    fort = {sq("a1"): 7, sq("a2"): 12, sq("b2"): 12, sq("b1"): 10,
            sq("a3"): 6, sq("b3"): 6, sq("c3"): 6, sq("c2"): 6, sq("c1"): 6}
    free = [s for s in range(64) if s not in fort]
    for name, (lo, hi) in BANDS.items():
        for _ in range(200000):
            n_black = rng.randint(*BLACK[name])
            squares = rng.sample(free, 1 + rng.randint(*QUEENS[name]) + n_black)
            pieces = dict(fort)
            pieces[squares[0]] = 1
            for s in squares[1:1 + n_black]:
                pieces[s] = 8
            for s in squares[1 + n_black:]:
                pieces[s] = 2
            st = S.make_state(pieces, True)
            if name == "WIDE_C":  # random boards stay below 193 moves: move queens while the list grows
                best = len(O.valid_moves(st)[0])
                for _ in range(150):
                    a = rng.choice([s for s, c in pieces.items() if c == 2])
                    b = rng.choice([s for s in free if s not in pieces])
                    trial = dict(pieces)
                    del trial[a]
                    trial[b] = 2
                    got = len(O.valid_moves(S.make_state(trial, True))[0])
                    if got >= best:
                        best, pieces = got, trial
                st = S.make_state(pieces, True)
            m3, after = O.valid_moves(st)
            if not lo <= len(m3) <= hi or O.in_check(after):
                continue
            wide = wide_children(st)
            if wide is None or (not wide and name != "WIDE_C"):
                continue
            r = S.search(st, 3 * len(m3), 1)
            need = 64 if name == "WIDE_A" else 128
            if not any(v > 0 for v in r["visits"][need:]) or (wide and not any(r["visits"][k] > 0 for k in wide)):
                continue
            print(f"{name} = make_state({dict(sorted(pieces.items()))}, True)  # {len(m3)} moves, best {r['best']}")
            break
        else:
            raise SystemExit(f"no board found for {name}")


if __name__ == "__main__":
    main()
