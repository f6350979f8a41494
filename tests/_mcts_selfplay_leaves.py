"""Plain-Python restatement of MCTS self-play and arena games with several leaves
in flight per game (DESIGN.md "Several leaves per game in self-play",
kv_config.leaves; k_leaves_* in knightvision_amd/csrc/kv_search.hip,
k_leaves_compact and eng_leaves_ply in kv_engine.hip) over the oracle's rules.

The game loop is that of tests/_mcts_selfplay_reuse.py (without carried trees)
and tests/_mcts_arena.py: the two MT19937 streams of the game, the root's mixed
priors, the move choice (random.choices over the visit counts, or their first
maximum from ply `sample_plies` on), the player per ply, and the ply count told
from outside -- or, with plies=None, the game played to its end by the rules of
tests/_mcts_endings.py from any start position. Each ply's search is the
sim-step loop of tests/_mcts_search.search: up to `leaves` descents per step
under the in-flight counts V, the collision rule, backups in descent order.
Every score is a numpy float32 operation in the kernel's order.

The game is a generator. It yields ("root", player, state) and is sent (logits,
value); per sim-step it yields ("step", player, [states of the step's pending
leaves in descent order]) -- also when the list is empty -- and is sent one
(logits, value) per state, so that play_many can form one batch per step and
player as the device does, and count the steps a batch of games runs. Shared
by tests/test_mcts_leaves_cpu.py and tests/test_mcts_leaves_gpu.py; not a test
module itself."""
import heapq

import numpy as np

from oracle import oracle as O

from tests import _mcts_endings as E
from tests import _mcts_search as S
from tests._mcts_arena import A, B, hash_eval_b, player_of  # noqa: F401  (also this module's names)
from tests._mcts_search import leaf_priors, policy_index, root_priors
from tests._mcts_selfplay_reuse import hash_eval  # noqa: F401

F = np.float32

# The hash-evaluator runs tests/test_mcts_leaves_gpu.py compares with the restatement (the engine's seed is SEED,
# game g's streams are seeded SEED + g; base: the first game id; plies: each game's length, all ended by
# max_moves). tests/test_mcts_leaves_cpu.py asserts that these very games hold a collision, a last step with a
# budget below `leaves`, and a search that reaches a terminal leaf (game 15 of "small_class", at ply 5).
SEED = 49
HASH_RUNS = {
    "tail": dict(slots=18, n_games=22, base=0, sims=22, leaves=4, max_moves=8, plies=(8,) * 22),
    "small_class": dict(slots=3, n_games=3, base=15, sims=150, leaves=4, max_moves=7, plies=(7,) * 3),
    "class_edge": dict(slots=5, n_games=5, base=0, sims=22, leaves=4, max_moves=4, plies=(4,) * 5),
    "wide": dict(slots=2, n_games=2, base=0, sims=70, leaves=64, max_moves=4, plies=(4,) * 2),
}


class _Node:
    __slots__ = ("state", "words", "P", "N", "V", "W", "child", "cstate")

    def __init__(self, state, words, priors):
        n = len(words)
        self.state = state  # after getValidMoves
        self.words = words
        self.P = np.asarray(priors, dtype=F)
        self.N = np.zeros(n, dtype=np.int32)
        self.V = np.zeros(n, dtype=np.int32)
        self.W = np.zeros(n, dtype=F)
        self.child = [None] * n
        self.cstate = [None] * n


def game(seed, gid, sims, plies, leaves, arena=False, sample_plies=0, c_puct=1.5, eps=0.25, alpha=0.3, start=None,
         max_moves=None):
    """`plies` plies of the game with global id `gid` whose two streams are seeded `seed` (the engine's seed +
    gid) at `leaves` descents per sim-step; arena: the player of a ply is the root's mover's (A is white iff gid
    is even), else always A. Returns one dict per ply: player, visits (root edge counts, list order), words (the
    root's move words), move (the record's index from * 64 + to), sampled (the move was drawn), accepted (per
    sim-step: the descents it accepted), leaf_pending (per sim-step: per accepted descent, the leaf went to the
    network), root_value (the root row's value, which the engine's resignation rule reads); the list's `extra`
    holds per ply the root's board (its 64 codes as bytes). start: the state vector the game starts from
    (None: the initial position). plies None: the game is played to its end under max_moves by tests/_mcts_endings.py's rules and the list returned is an
    E.Played with result (plies, outcome, reason, reward) and holds."""
    c = F(c_puct)
    ncap = sims + 2
    np_mt, py_mt = O.MT(seed, "numpy"), O.MT(seed, "python")
    sqt = [F(np.sqrt(np.float64(k))) for k in range(sims + 4)]
    vec = E.start_state(start)
    out = E.Played()
    ply = -1
    while plies is None or ply + 1 < plies:
        ply += 1
        moves3, st = O.valid_moves(vec)
        if plies is None and len(moves3) == 0:
            return E.finish(out, ply, E.no_moves(st), False)
        assert len(moves3) > 0, "the game the device recorded goes on here"
        words = S.move_words(st, moves3)
        root_wtm = int(st[64])
        who = player_of(gid, root_wtm) if arena else A
        logits, root_value = yield "root", who, st
        root, root_n, done = _Node(st, words, root_priors(logits, words, np_mt, eps, alpha)), 1, 0
        acc_steps, pend_steps = [], []
        while done < sims:
            r = min(leaves, sims - done)
            vroot, accepted, held = 0, [], []
            for _ in range(r):
                node, n_par, path = root, root_n + vroot, []
                while True:
                    nv = node.N + node.V
                    u = c * node.P * sqt[n_par] / (1 + nv).astype(F)
                    q = np.where(nv > 0, (node.W - node.V.astype(F)) / np.maximum(nv, 1).astype(F), F(0.0)).astype(F)
                    bi = int(np.argmax(q + u))  # the first maximum in list order
                    path.append((node, bi))
                    if node.cstate[bi] is None:
                        node.cstate[bi] = O.make_valid_move(node.state, bi)
                    child = node.child[bi]
                    if child is None or len(path) >= ncap:
                        break
                    n_par = int(nv[bi])
                    node = child
                leaf_node, leaf_j = path[-1]
                if any(ln is leaf_node and lj == leaf_j for ln, lj in held):
                    break  # collision: dropped, the step's descents end
                ls = leaf_node.cstate[leaf_j]
                if O.is_draw(ls):
                    rec = (path, False, F(0.0))
                else:
                    lm, lst = O.valid_moves(ls)
                    if len(lm) == 0:
                        rec = (path, False, F((-1.0 if lst[64] else 1.0) if O.in_check(lst) else 0.0))
                    else:
                        rec = (path, True, (lst, S.move_words(lst, lm)))
                        held.append((leaf_node, leaf_j))
                for nd, j in path:
                    nd.V[j] += 1
                vroot += 1
                accepted.append(rec)
            # the step's pending leaves go out together, in descent order
            rows = yield "step", who, [val[0] for _, pending, val in accepted if pending]
            rows = iter(rows)
            for path, pending, val in accepted:
                if pending:
                    llog, v = next(rows)
                    v = F(v)
                    lst, lw = val
                    leaf_node, leaf_j = path[-1]
                    leaf_node.child[leaf_j] = _Node(lst, lw, leaf_priors(llog, lw))
                else:
                    v = val
                for d, (nd, j) in enumerate(path):
                    white_moved = (root_wtm != 0) ^ bool(d & 1)
                    nd.V[j] -= 1
                    nd.N[j] += 1
                    nd.W[j] = nd.W[j] + (v if white_moved else -v)
                root_n += 1
            done += len(accepted)
            acc_steps.append(len(accepted))
            pend_steps.append([pending for _, pending, _ in accepted])
        visits = [int(x) for x in root.N]
        sampled = sample_plies == 0 or (sample_plies > 0 and ply < sample_plies)
        if sampled:
            total = np.float64(0.0)
            for x in visits:
                total = total + np.float64(x)
            pick = py_mt.choices_index(np.array(visits, dtype=np.float64) / total)
        else:
            pick = visits.index(max(visits))
        out.append(dict(player=who, visits=visits, words=list(words), move=policy_index(words[pick]),
                        sampled=sampled, accepted=acc_steps, leaf_pending=pend_steps, root_value=F(root_value)))
        out.extra.append(dict(board=bytes(st[:64])))
        vec = O.make_valid_move(vec, pick)
        if plies is None:
            end = E.after_move(vec, ply + 1, root_value, max_moves)
            if end is not None:
                return E.finish(out, ply + 1, end, True)
    return out


def play(seed, gid, sims, plies, leaves, evaluate_a=hash_eval, evaluate_b=hash_eval_b, **kw):
    """game() with one evaluator per player, evaluate_x(state) -> (logits[4096], value)."""
    g = game(seed, gid, sims, plies, leaves, **kw)
    ev = (evaluate_a, evaluate_b)
    try:
        kind, who, req = next(g)
        while True:
            kind, who, req = g.send(ev[who](req) if kind == "root" else [ev[who](st) for st in req])
    except StopIteration as done:
        return done.value


def starts_of(plies, slots, holds=None):
    """The engine ply-step at which each game of a recycling run begins: the first `slots` games at 0, every
    later id in the slot that is free first (a game of n plies that ends on a committed move holds its slot for
    n ply-steps, one that ends with no legal move for n + 1: k_movegen finds that in a ply-step of its own --
    holds: the ply-steps per game where they differ from plies, E.Played.holds; which of the slots freed in one
    ply-step takes which id does not matter here)."""
    free = [0] * slots
    heapq.heapify(free)
    out = []
    for n in (plies if holds is None else holds):
        t = heapq.heappop(free)
        out.append(t)
        heapq.heappush(free, t + n)
    return out


def play_many(seeds, gids, sims, plies, leaves, evaluate_many_a, evaluate_many_b=None, starts=None, **kw):
    """play() of several games (plies: one count per game; starts: the ply-step each begins at, default 0) that
    share an engine: per ply-step one root batch per player, then per sim-step one batch per player of the
    pending leaves of all games, until no game of the ply-step is left searching. evaluate_many_x(list of
    states) -> list of (logits, value). Each game is play()'s own, whatever the others are.
    -> (per-game outputs, dict(steps: the sim-steps the batch ran, pending: [A's, B's] pending leaf rows,
    batches: per sim-step (A's, B's) rows))."""
    gens = [game(s, g, sims, n, leaves, **kw) for s, g, n in zip(seeds, gids, plies)]
    ev = (evaluate_many_a, evaluate_many_b or evaluate_many_a)
    starts = list(starts) if starts is not None else [0] * len(gens)
    out, req = [None] * len(gens), {}
    info = dict(steps=0, pending=[0, 0], batches=[])

    def advance(k, val=None):
        try:
            req[k] = next(gens[k]) if val is None else gens[k].send(val)
        except StopIteration as done:
            out[k] = done.value
            req.pop(k, None)

    eply = 0
    while req or any(s >= eply for s in starts):
        for k, s in enumerate(starts):
            if s == eply:
                advance(k)
        assert all(kind == "root" for kind, _, _ in req.values())
        for x in (A, B):  # the root rows, one batch per player
            ks = sorted(k for k in req if req[k][1] == x)
            if ks:
                for k, row in zip(ks, ev[x]([req[k][2] for k in ks])):
                    advance(k, row)
        while True:
            stepping = sorted(k for k in req if req[k][0] == "step")
            if not stepping:
                break
            info["steps"] += 1
            got, counts = {k: [] for k in stepping}, [0, 0]
            for x in (A, B):
                ks = [k for k in stepping if req[k][1] == x]
                states = [st for k in ks for st in req[k][2]]
                counts[x] = len(states)
                rows = iter(ev[x](states) if states else [])
                for k in ks:
                    got[k] = [next(rows) for _ in req[k][2]]
            info["pending"][A] += counts[A]
            info["pending"][B] += counts[B]
            info["batches"].append(tuple(counts))
            for k in stepping:
                advance(k, got[k])
        eply += 1
    return out, info
