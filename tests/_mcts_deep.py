"""Two forced-line positions whose searches descend far deeper than a wavefront is wide, and the runs built from
them (tests/test_deep_lines_cpu.py, tests/test_deep_lines_gpu.py). Not a test module itself.

CHAIN (4b2k/3pPp1p/3P1P1P/8/8/p1p1p3/P1PpP3/K2B4): every pawn is blocked, both bishops are walled in, and either
king has one square to shuttle to -- Ka1-b1-a1, Kh8-g8-h8 -- so each side has exactly one legal move for ever. A
search of it is one chain: sim k descends k plies, every node is the only child of the one before it. CHAIN_B adds
a white pawn on b5 and a black one on b7: each side has a spare pawn move until the b-file locks, so the root has
two moves and the subtrees turn into chains of different lengths, several of them in flight at once.

What the GPU tests rely on -- the depths, the sim-steps with two deep descents in flight, one legal move at every
ply -- is asserted from the references alone in tests/test_deep_lines_cpu.py."""
import functools

from oracle import oracle as O

from tests import _eval_cache as EC
from tests import _mcts_arena as AR
from tests import _mcts_search as S
from tests import _mcts_selfplay_leaves as SL
from tests import _mcts_selfplay_pcr as PC
from tests import _mcts_selfplay_reuse as RU
from tests._mcts_search import make_state, sq

# codes: 1..6 white K Q R B N p, 7..12 black K Q R B N p
_CHAIN = {sq("a1"): 1, sq("d1"): 4, sq("a2"): 6, sq("c2"): 6, sq("e2"): 6, sq("e7"): 6, sq("d6"): 6, sq("f6"): 6,
          sq("h6"): 6, sq("h8"): 7, sq("e8"): 10, sq("a3"): 12, sq("c3"): 12, sq("e3"): 12, sq("d2"): 12,
          sq("d7"): 12, sq("f7"): 12, sq("h7"): 12}
CHAIN = make_state(_CHAIN, True)
CHAIN_BLACK = make_state(_CHAIN, False)  # the same line, black to move first
CHAIN_B = make_state({**_CHAIN, sq("b5"): 6, sq("b7"): 12}, True)

# the sizes every comparison runs at: the sims of a search of the position, games of 6 plies
SIMS = {"CHAIN": 160, "CHAIN_B": 400}
POSITIONS = {"CHAIN": CHAIN, "CHAIN_B": CHAIN_B}
MAX_MOVES, SEED = 6, 77
C_PUCT, EPS, ALPHA = 1.5, 0.25, 0.3
# playout cap randomization with carried trees: a fast ply's target is far below what its carried root holds
FAST_SIMS, Q16 = 8, 32768


def starts_of(name):
    """The start list of a self-play run from `name`: game g starts from starts_of(name)[g % 2]. CHAIN is played
    from both colours; CHAIN_B has no mirror image (its b-pawns are not symmetric), so both games start alike and
    differ by their streams."""
    return [CHAIN, CHAIN_BLACK] if name == "CHAIN" else [CHAIN_B, CHAIN_B]


def n_games(name, slow=False):
    """The games of a run: two, but one where a game from CHAIN_B costs the restatement seconds (slow: the
    several-leaves and arena restatements, numpy per node)."""
    return 1 if slow and name == "CHAIN_B" else 2


@functools.lru_cache(maxsize=None)
def search_ref(name, leaves, sims=None):
    """The restated hash-evaluator search of a position at its sims (or at `sims`: a kv_search call has one
    count for all its positions), with the path lengths."""
    return S.search(POSITIONS[name], sims or SIMS[name], leaves, depths=True)


def deepest(r):
    return max(d for step in r["depths"] for d in step)


def steps_with_two_deep(r, deeper_than=64):
    return sum(sum(d > deeper_than for d in step) >= 2 for step in r["depths"])


def _kw(name, g):
    return dict(c_puct=C_PUCT, eps=EPS, alpha=ALPHA, start=starts_of(name)[g % 2], max_moves=MAX_MOVES)


@functools.lru_cache(maxsize=None)
def oracle_games(name):
    """The C oracle's one-leaf games from the start list (hash evaluator)."""
    n = n_games(name)
    return O.mcts_play_batch(SIMS[name], [SEED + g for g in range(n)], max_moves=MAX_MOVES, c_puct=C_PUCT, eps=EPS,
                             alpha=ALPHA, keep_visits=True, starts=[starts_of(name)[g % 2] for g in range(n)])


@functools.lru_cache(maxsize=None)
def leaves_games(name, leaves):
    """tests/_mcts_selfplay_leaves.py's games played to the cap."""
    return [SL.play(SEED + g, g, SIMS[name], None, leaves, **_kw(name, g)) for g in range(n_games(name, True))]


@functools.lru_cache(maxsize=None)
def arena_games(name):
    """tests/_mcts_arena.py's one-leaf games (player B's value negated) played to the cap."""
    return [AR.play(SEED + g, g, SIMS[name], None, **_kw(name, g)) for g in range(n_games(name, True))]


@functools.lru_cache(maxsize=None)
def reuse_games(name):
    """tests/_mcts_selfplay_reuse.py's games with carried trees."""
    return [RU.play(SEED + g, SIMS[name], None, True, **_kw(name, g)) for g in range(n_games(name))]


@functools.lru_cache(maxsize=None)
def pcr_reuse_games(name):
    """tests/_mcts_selfplay_pcr.py's one-leaf games with carried trees and fast plies."""
    return [PC.play(SEED + g, SIMS[name], None, True, FAST_SIMS, Q16, **_kw(name, g)) for g in range(n_games(name))]


CACHE_LEAVES, CACHE_ENTRIES = 2, 64


@functools.lru_cache(maxsize=None)
def cached_games(name="CHAIN", entries=CACHE_ENTRIES):
    """tests/_eval_cache.py's run of the two games at CACHE_LEAVES leaves behind a table of `entries` entries
    (0: no cache) -> (games, info, the table)."""
    n = n_games(name)
    cache = EC.CachedEval(EC._hash_many, entries, 0)
    games, info = EC.play_many_cached([SEED + g for g in range(n)], list(range(n)), SIMS[name], [None] * n,
                                      CACHE_LEAVES, cache, c_puct=C_PUCT, eps=EPS, alpha=ALPHA,
                                      per_game=[dict(start=starts_of(name)[g % 2], max_moves=MAX_MOVES)
                                                for g in range(n)])
    return games, info, cache.table
