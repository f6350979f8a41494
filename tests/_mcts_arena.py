"""Plain-Python restatement of an arena game (DESIGN.md "Arena", kv_config.arena /
kv_config.sample_plies; k_arena_split and eng_arena_ply in kv_engine.hip,
k_mcts_choose in kv_mcts.hip) over the oracle's rules: the self-play search of
tests/_mcts_selfplay_reuse.py without carried trees, in which every evaluation
of a ply -- the root row and each leaf row -- belongs to the player whose move
it is at the root. In the game with global id g player A (0) is white iff g is
even. From ply `sample_plies` on (-1: from the first) the move is the first
maximum of the root visit counts and the CPython stream is not advanced.

Built from that file's node, the priors of tests/_mcts_search.py and the
oracle's rules and streams. The game is a generator that yields (player, state
after getValidMoves) per evaluation and is sent (logits[4096], value). It is
told how many plies to play, or (plies=None) plays to the end by the rules of
tests/_mcts_endings.py from any start position. Shared by
tests/test_arena_cpu.py and tests/test_arena_gpu.py; not a test module itself."""
import numpy as np

from oracle import oracle as O

from tests import _mcts_endings as E
from tests import _mcts_search as S
from tests._mcts_selfplay_reuse import _Node, hash_eval, leaf_priors, policy_index, root_priors

F = np.float32
A, B = 0, 1


def hash_eval_b(state):
    """Player B's row under KV_EVAL_HASH: the hash evaluator's with the value negated."""
    lg, v = hash_eval(state)
    return lg, F(-v)


def player_of(gid, wtm):
    """The player to move: A is white iff the game's global id is even."""
    return A if ((gid % 2 == 0) == bool(wtm)) else B


def game(seed, gid, sims, plies, sample_plies=0, c_puct=1.5, eps=0.0, alpha=0.3, start=None, max_moves=None):
    """`plies` plies of the arena game with global id `gid` whose two streams are seeded `seed` (the engine's
    seed + gid), as a generator: yields (player, state) per evaluation, is sent (logits, value); returns one
    dict per ply: player, visits (root edge counts, list order), words (the root's move words), move (the
    record's index from * 64 + to), sampled (the move was drawn); the list's `extra` holds per ply board (the root's
    64 codes as bytes), root_value and pending (the leaf rows the ply sent to the network). start: the state
    vector the game starts from (None: the initial position). plies None: the game is played to its end under max_moves by
    tests/_mcts_endings.py's rules and the list returned is an E.Played with result (plies, outcome, reason,
    reward) and holds."""
    c = F(c_puct)
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
        who = player_of(gid, root_wtm)
        logits, root_value = yield who, st
        root, root_n, n_pending = _Node(st, words, root_priors(logits, words, np_mt, eps, alpha)), 1, 0
        for _ in range(sims):
            node, n_par, path = root, root_n, []
            while True:
                u = c * node.P * sqt[n_par] / (1 + node.N).astype(F)
                q = np.where(node.N > 0, node.W / np.maximum(node.N, 1).astype(F), F(0.0)).astype(F)
                bi = int(np.argmax(q + u))  # the first maximum in list order
                path.append((node, bi))
                if node.cstate[bi] is None:
                    node.cstate[bi] = O.make_valid_move(node.state, bi)
                child = node.child[bi]
                if child is None:
                    break
                n_par = int(node.N[bi])
                node = child
            leaf_node, leaf_j = path[-1]
            ls = leaf_node.cstate[leaf_j]
            v = F(0.0)
            if not O.is_draw(ls):
                lm, lst = O.valid_moves(ls)
                if len(lm) == 0:
                    v = F((-1.0 if lst[64] else 1.0) if O.in_check(lst) else 0.0)
                else:
                    lw = S.move_words(lst, lm)
                    llog, v = yield who, lst  # the leaf row too is the root mover's net's
                    v = F(v)
                    n_pending += 1
                    leaf_node.child[leaf_j] = _Node(lst, lw, leaf_priors(llog, lw))
            for d, (nd, j) in enumerate(path):
                white_moved = (root_wtm != 0) ^ bool(d & 1)
                nd.N[j] += 1
                nd.W[j] = nd.W[j] + (v if white_moved else -v)
            root_n += 1
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
                        sampled=sampled))
        out.extra.append(dict(board=bytes(st[:64]), root_value=F(root_value), pending=n_pending))
        vec = O.make_valid_move(vec, pick)
        if plies is None:
            end = E.after_move(vec, ply + 1, root_value, max_moves)
            if end is not None:
                return E.finish(out, ply + 1, end, True)
    return out


def play(seed, gid, sims, plies, evaluate_a=hash_eval, evaluate_b=hash_eval_b, **kw):
    """game() with one evaluator per player, evaluate_x(state) -> (logits[4096], value)."""
    g = game(seed, gid, sims, plies, **kw)
    ev = (evaluate_a, evaluate_b)
    try:
        who, st = next(g)
        while True:
            who, st = g.send(ev[who](st))
    except StopIteration as done:
        return done.value


def play_many(seeds, gids, sims, plies, evaluate_many_a, evaluate_many_b, **kw):
    """play() of several games (plies: one count per game) whose evaluations go out together, per round one
    batch per player: evaluate_many_x(list of states) -> list of (logits, value). Each game is play()'s own,
    whatever the others are."""
    gens = [game(s, g, sims, n, **kw) for s, g, n in zip(seeds, gids, plies)]
    ev = (evaluate_many_a, evaluate_many_b)
    out, want = [None] * len(gens), {}
    for k, g in enumerate(gens):
        try:
            want[k] = next(g)
        except StopIteration as done:
            out[k] = done.value
    while want:
        got = {}
        for x in (A, B):
            ks = sorted(k for k in want if want[k][0] == x)
            if ks:
                got.update(zip(ks, ev[x]([want[k][1] for k in ks])))
        for k in sorted(got):
            try:
                want[k] = gens[k].send(got[k])
            except StopIteration as done:
                out[k] = done.value
                del want[k]
    return out
