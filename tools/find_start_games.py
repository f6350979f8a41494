"""Print, for every start position of tests/_mcts_starts.py and a range of seeds, how the C oracle's one-leaf
MCTS game from it ends on the hash evaluator (plies, reason, outcome), its widest root, whether a first-maximum
choice fell at a root index >= 64, and the special moves it played: the table the runs of
tests/_mcts_starts.py were picked from (tests/test_starts_cpu.py asserts what they hold). CPU only, seconds.

    python tools/find_start_games.py [--sims 16] [--seeds 100 116] [--sample-plies 0] [--max-moves 40]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle as O  # noqa: E402
from tests import _mcts_starts as ST  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=16)
    ap.add_argument("--seeds", type=int, nargs=2, default=(100, 116))
    ap.add_argument("--sample-plies", type=int, default=0)
    ap.add_argument("--max-moves", type=int, default=ST.MAX_MOVES)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    seeds = list(range(*a.seeds))
    for name, start in ST.POSITIONS.items():
        if a.only and name not in a.only:
            continue
        games = O.mcts_play_batch(a.sims, seeds, max_moves=a.max_moves, keep_visits=True,
                                  starts=[start] * len(seeds), sample_plies=a.sample_plies)
        for s, g in zip(seeds, games):
            d = ST.describe(start, g["moves"], g["visits"])
            print(f"{name:16s} sims {a.sims:3d} seed {s}: plies {g['plies']:2d} reason {g['reason']} outcome "
                  f"{g['outcome']:+d} widest root {max(d['widths'], default=0):3d}"
                  f"{' argmax>=64' if d['high'] else ''} {' '.join(sorted(d['special']))}")


if __name__ == "__main__":
    main()
