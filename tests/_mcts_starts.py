"""The fixed set of start positions for self-play, arena and game-ending tests (kv_dev_set_starts;
tests/test_starts_cpu.py, tests/test_starts_gpu.py), and the runs built from it. Not a test module itself.

A run names one position per game: the engine gets the run's positions as its start list (game g starts from
positions[g % len(positions)], its two streams are seeded seed + g), and the references play the same
(position, seed) pairs. tests/test_starts_cpu.py asserts from the references alone that the runs below hold
every ending, root width and special move the GPU tests rely on; tools/find_start_games.py prints the table
the runs were picked from."""
import functools

import numpy as np

from oracle import oracle as O

from tests import _eval_cache as EC
from tests import _mcts_arena as AR
from tests import _mcts_search as S
from tests import _mcts_selfplay_leaves as SL
from tests import _mcts_selfplay_reuse as RU
from tests._mcts_search import (CHECKMATED_ROOT, KINGS_ONLY_ROOT, KPK_CAPTURE, MATE_IN_ONE, ONE_MOVE, STALEMATE_ROOT,
                                WIDE_A, WIDE_B, WIDE_C, make_state, sq)

# codes: 1..6 white K Q R B N p, 7..12 black K Q R B N p
KPH = make_state({sq("g6"): 1, sq("h6"): 6, sq("h8"): 7}, True)               # h7 stalemates
KBP = make_state({sq("b6"): 1, sq("d4"): 4, sq("a6"): 6, sq("a8"): 7}, True)
KPF = make_state({sq("e6"): 1, sq("f7"): 6, sq("f8"): 7}, True)
BQ = make_state({sq("h1"): 1, sq("f2"): 7, sq("g8"): 8}, False)               # black mates: ...Qg2 and others
KRK_B = make_state({sq("e8"): 1, sq("e1"): 7, sq("a2"): 9}, False)


def _with(state, ep=None, unmoved=False):
    v = state.copy()
    if ep is not None:
        v[75:77] = ((8 - int(ep[1])), "abcdefgh".index(ep[0]))
    if unmoved:
        v[69:75] = 0
    return v


# a7-a8 promotes (and b7xa8 does not exist: one promotion move, beside the king's)
PROMO = make_state({sq("e1"): 1, sq("a7"): 6, sq("g2"): 6, sq("h8"): 7, sq("h7"): 12, sq("c5"): 12}, True)
# black has just played d7-d5: e5xd6 en passant (the en-passant square is the one the pawn passed over)
EP = _with(make_state({sq("e1"): 1, sq("e5"): 6, sq("a2"): 6, sq("e8"): 7, sq("d5"): 12, sq("h7"): 12}, True),
           ep="d6")
# both of white's castlings are in the list, black's after any quiet white move
CASTLE = _with(make_state({sq("e1"): 1, sq("a1"): 3, sq("h1"): 3, sq("a2"): 6, sq("h2"): 6, sq("e8"): 7, sq("a8"): 9,
                           sq("h8"): 9, sq("a7"): 12, sq("h7"): 12}, True), unmoved=True)


def _after_e4_e5_nf3():
    v = O.initial_state()
    for a, b in (("e2", "e4"), ("e7", "e5"), ("g1", "f3")):
        v[sq(b)], v[sq(a)] = v[sq(a)], 0
    v[64] = 0
    return v


BLACK_MG = _after_e4_e5_nf3()  # 1. e4 e5 2. Nf3, black to move, nothing moved that castles
# a second black-to-move middlegame: queens and rooks on an open board, black's castlings gone
BLACK_OPEN = make_state({sq("g1"): 1, sq("d1"): 2, sq("f1"): 3, sq("c3"): 5, sq("f2"): 6, sq("g2"): 6, sq("h2"): 6,
                         sq("g8"): 7, sq("d8"): 8, sq("f8"): 9, sq("f6"): 11, sq("f7"): 12, sq("g7"): 12,
                         sq("h7"): 12}, False)

POSITIONS = dict(ONE_MOVE=ONE_MOVE, MATE_IN_ONE=MATE_IN_ONE, KPK_CAPTURE=KPK_CAPTURE, CHECKMATED_ROOT=CHECKMATED_ROOT,
                 STALEMATE_ROOT=STALEMATE_ROOT, KINGS_ONLY_ROOT=KINGS_ONLY_ROOT, WIDE_A=WIDE_A, WIDE_B=WIDE_B,
                 WIDE_C=WIDE_C, KPH=KPH, KBP=KBP, KPF=KPF, BQ=BQ, KRK_B=KRK_B, PROMO=PROMO, EP=EP, CASTLE=CASTLE,
                 BLACK_MG=BLACK_MG, BLACK_OPEN=BLACK_OPEN)
MAX_MOVES = 40
NAMES = list(POSITIONS)
C_PUCT, EPS, ALPHA = 1.5, 0.25, 0.3


def start_list():
    """The engine's start list: game g starts from start_list()[g % len(NAMES)]."""
    return np.stack([POSITIONS[n] for n in NAMES])


def start_of(g):
    return POSITIONS[NAMES[g % len(NAMES)]]


def describe(start, moves, visits):
    """Of one game from `start` (moves: the records' from * 64 + to per ply; visits: per ply the root visit
    counts in list order) -> dict(widths: the root's move count per ply, high: plies whose first maximum of
    the visit counts lies at a root index >= 64, special: the special moves played, 'ep' / 'castle' / 'promo',
    first_black: black moved first)."""
    vec, widths, high, special = np.array(start, dtype=np.int8), [], [], set()
    first_black = None
    for ply, mv in enumerate(moves):
        moves3, st = O.valid_moves(vec)
        if first_black is None:
            first_black = not st[64]
        widths.append(len(moves3))
        v = [int(x) for x in visits[ply][:len(moves3)]]
        idx = [i for i, (fr, to, fl) in enumerate(moves3) if int(fr) * 64 + int(to) == int(mv)]
        pick = idx[0] if len(idx) == 1 else [i for i in idx if v[i] > 0][0]
        if v.index(max(v)) >= 64:
            high.append(ply)
        fl = int(moves3[pick][2])
        special |= {n for b, n in ((1, "ep"), (2, "castle"), (4, "promo")) if fl & b}
        vec = O.make_valid_move(vec, pick)
    return dict(widths=widths, high=high, special=special, first_black=bool(first_black))


# ---- the references' games of a run (seed: the engine's; game g: start_of(g), both streams seeded seed + g),
# each as dict(moves, visits, boards, plies, outcome, reason, reward, n_evals) plus what its mode adds; cached,
# so the CPU and the GPU tests of one session play each run once
def _row(moves, visits, boards, result, n_evals, **more):
    plies, outcome, reason, reward = result
    return dict(moves=[int(m) for m in moves], visits=[[int(x) for x in v] for v in visits], boards=boards,
                plies=int(plies), outcome=int(outcome), reason=int(reason), reward=float(reward),
                n_evals=int(n_evals), **more)


def _boards(start, moves):
    """The root boards (64 codes as bytes) and root move words of an oracle game, replayed from its moves."""
    vec, out, words = np.array(start, dtype=np.int8), [], []
    for ply, mv in enumerate(moves):
        moves3, st = O.valid_moves(vec)
        out.append(bytes(st[:64]))
        words.append(S.move_words(st, moves3))
        idx = [i for i, (fr, to, fl) in enumerate(moves3) if int(fr) * 64 + int(to) == int(mv)]
        assert len(idx) == 1
        vec = O.make_valid_move(vec, idx[0])
    return out, words


@functools.lru_cache(maxsize=None)
def oracle_run(seed, n_games, sims, sample_plies=0):
    """The C oracle's one-leaf games (kvo_mcts_play_batch) on the hash evaluator."""
    games = O.mcts_play_batch(sims, [seed + g for g in range(n_games)], max_moves=MAX_MOVES, c_puct=C_PUCT, eps=EPS,
                              alpha=ALPHA, keep_visits=True, starts=[start_of(g) for g in range(n_games)],
                              sample_plies=sample_plies)
    out = []
    for g, r in enumerate(games):
        n = [int((v >= 0).sum()) for v in r["visits"]]
        boards, words = _boards(start_of(g), r["moves"])
        out.append(_row(r["moves"], [v[:k] for v, k in zip(r["visits"], n)], boards,
                        (r["plies"], r["outcome"], r["reason"], r["reward"]), r["n_evals"], words=words))
    return out


@functools.lru_cache(maxsize=None)
def leaves_run(seed, n_games, sims, leaves, sample_plies=0, arena=False):
    """tests/_mcts_selfplay_leaves.py played to the end (arena: B's value negated)."""
    out = []
    for g in range(n_games):
        p = SL.play(seed + g, g, sims, None, leaves, arena=arena, sample_plies=sample_plies, c_puct=C_PUCT, eps=EPS,
                    alpha=ALPHA, start=start_of(g), max_moves=MAX_MOVES)
        pend = sum(sum(map(sum, x["leaf_pending"])) for x in p)
        out.append(_row([x["move"] for x in p], [x["visits"] for x in p], [e["board"] for e in p.extra], p.result,
                        len(p) + pend, words=[x["words"] for x in p], players=[x["player"] for x in p],
                        leaf_pending=[x["leaf_pending"] for x in p], holds=p.holds,
                        steps=[len(x["accepted"]) for x in p], arena=arena))
    return out


@functools.lru_cache(maxsize=None)
def reuse_run(seed, n_games, sims, reuse=True):
    """tests/_mcts_selfplay_reuse.py played to the end."""
    out = []
    for g in range(n_games):
        p = RU.play(seed + g, sims, None, reuse, c_puct=C_PUCT, eps=EPS, alpha=ALPHA, start=start_of(g),
                    max_moves=MAX_MOVES)
        out.append(_row([x["move"] for x in p], [x["visits"] for x in p], [e["board"] for e in p.extra], p.result,
                        len(p) + sum(sum(x["pending"]) for x in p), words=[x["words"] for x in p],
                        kept=[x["kept"] for x in p], carried=[x["carried"] for x in p],
                        child_kept=[e["child_kept"] for e in p.extra], holds=p.holds))
    return out


@functools.lru_cache(maxsize=None)
def arena_run(seed, n_games, sims, sample_plies=0):
    """tests/_mcts_arena.py played to the end (one leaf; player B's value negated)."""
    out = []
    for g in range(n_games):
        p = AR.play(seed + g, g, sims, None, sample_plies=sample_plies, c_puct=C_PUCT, eps=EPS, alpha=ALPHA,
                    start=start_of(g), max_moves=MAX_MOVES)
        out.append(_row([x["move"] for x in p], [x["visits"] for x in p], [e["board"] for e in p.extra], p.result,
                        len(p) + sum(e["pending"] for e in p.extra), words=[x["words"] for x in p],
                        players=[x["player"] for x in p], holds=p.holds, arena=True))
    return out


def coverage(games):
    """The tags a list of reference games (game g from start_of(g)) holds; tests/test_starts_cpu.py asserts them."""
    tags = set()
    for g, r in enumerate(games):
        if r["outcome"]:
            tags.add(f"reason{r['reason']}{'+' if r['outcome'] > 0 else '-'}")
        if r["reason"] == 0:
            tags.add("reason0")
        if r["reason"] in (2, 3) and r["plies"] == 0:
            tags.add(f"reason{r['reason']}@0")
        if r["reason"] == 3 and r["plies"] >= 1:
            tags.add("reason3@1+")
        if r["reason"] == 4:
            tags.add("reason4@1" if r["plies"] == 1 else "reason4@2+")
        d = describe(start_of(g), r["moves"], r["visits"])
        tags |= {f"root>{w}" for w in (64, 96, 128) if any(x > w for x in d["widths"])}
        if d["high"]:
            tags.add("max@64+")
        tags |= d["special"]
        if r["plies"] and d["first_black"]:
            tags.add("first_black")
        if r.get("arena") and r["outcome"] != 0:
            a_white = g % 2 == 0
            a_won = (r["outcome"] > 0) == a_white
            tags.add(f"{'A' if a_won else 'B'}_wins_A_{'white' if a_white else 'black'}")
        if "carried" in r:
            if any(r["carried"]):
                tags.add("carried")
            if r["plies"] and r["child_kept"][-1] and r["holds"] == r["plies"]:
                tags.add("dropped_at_end")
        if "leaf_pending" in r:
            for ply, steps in enumerate(r["leaf_pending"]):
                last = ply == r["plies"] - 1
                if any(not p for s in steps for p in s) and not (last and r["reason"] in (2, 3, 4)):
                    tags.add("terminal_leaf_mid_game")
    return tags


def recycled_after(games, slots):
    """The games of a recycling run on `slots` slots after which their slot certainly starts another game: those
    that end while at least as many games wait as slots have been freed so far."""
    holds = [r["holds"] for r in games]
    ends = [s + h for s, h in zip(SL.starts_of(holds, slots, holds), holds)]
    return [g for g in range(len(games)) if sum(e <= ends[g] for e in ends) <= len(games) - slots]


# The runs of tests/test_starts_gpu.py: the engine's seed, the games (two rounds through the set, so the start
# list wraps) and the sims of every search; a third as many slots in the recycling runs
SEED, N_GAMES, SIMS, SLOTS_THIRD = 202, 2 * len(NAMES), 16, 13
GENERAL = {"reason2+", "reason2-", "reason3@1+", "reason3@0", "reason2@0", "reason4@1", "reason4@2+", "reason1+",
           "reason1-", "reason0", "root>64", "root>96", "root>128", "max@64+", "promo", "ep", "castle"}

# The evaluation cache under recycling (tests/test_eval_cache_cpu.py, tests/test_eval_cache_gpu.py): the first 22
# games of the set at 2 leaves on 2 slots, so that 20 games start in a recycled slot while the table is warm -- game
# 19 starts from game 0's position. On 2 slots no two slots of this run are freed in the same ply-step, so the
# slot every game sits in (and with it the order of a step's list) does not depend on the order in which freed
# slots draw their ids; tests/test_eval_cache_cpu.py asserts that, a hit across games and a claim contest.
RECYCLE = dict(n_games=22, slots=2, leaves=2, small=64, large=1 << 12)


def recycling_seating():
    """(starts, slot_of, ties) of the RECYCLE run, from the uncached restatement's games."""
    ref = leaves_run(SEED, N_GAMES, SIMS, RECYCLE["leaves"])[:RECYCLE["n_games"]]
    return EC.seating([r["holds"] for r in ref], RECYCLE["slots"])


def recycling_run(entries, table=None):
    """The RECYCLE run behind tests/_eval_cache.py's cache of `entries` entries (table: another table object in
    its place) -> (games, info, the CachedEval)."""
    n = RECYCLE["n_games"]
    starts, slot_of, _ = recycling_seating()
    cache = EC.CachedEval(EC._hash_many, entries, 0)
    if table is not None:
        cache.table = table
    games, info = EC.play_many_cached([SEED + g for g in range(n)], list(range(n)), SIMS, [None] * n,
                                      RECYCLE["leaves"], cache, c_puct=C_PUCT, eps=EPS, alpha=ALPHA,
                                      per_game=[dict(start=start_of(g), max_moves=MAX_MOVES) for g in range(n)],
                                      starts=starts, slot_of=slot_of)
    return games, info, cache


cached_recycling_run = functools.lru_cache(maxsize=None)(recycling_run)
