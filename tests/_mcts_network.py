"""What the GPU tests of MCTS self-play on the real ChessNet share (tests/test_mcts_gpu.py,
tests/test_starts_gpu.py): the oracle is fed the HIP network's own rows, evaluated in the batch class the
engine's batches are in, so root visit vectors and moves must be identical. Not a test module itself."""
import numpy as np
import torch

from knightvision_amd.engine import packed_from

CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class


def hip_eval(sd, class_rows=CLASS_ROWS):
    """Oracle evaluator: the HIP network's row for one board, computed in a
    batch of class_rows copies (the engine's batch class: 17 = the > 16-board
    Winograd class, 1 = the <= 16-board direct class of a one-slot engine)."""
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


def count_ties(tag, recs, visits, game_ids, play):
    """The engine's records and root visit rows of the games `game_ids` against play(g, plies) -> the oracle's
    game dict of at least that many plies -> (compared plies, plies that differ: a game parts at its first)."""
    ties = compared = 0
    for g in game_ids:
        sel = recs["game_id"] == g
        moves, vis = recs["move"][sel], visits[sel]
        n = len(moves)
        r = play(g, n)
        assert len(r["moves"]) >= n
        for p in range(n):
            compared += 1
            if not (np.array_equal(vis[p], r["visits"][p]) and moves[p] == r["moves"][p]):
                ties += 1
                print(f"{tag} game {g} ply {p}: GPU visits {vis[p][vis[p] >= 0]} oracle "
                      f"{r['visits'][p][r['visits'][p] >= 0]}")
                break  # the games part here
    return compared, ties
