"""Plain-Python restatement of MCTS self-play with playout cap randomization
(DESIGN.md "Playout cap randomization", kv_config.fast_sims / full_q16;
ply_target in knightvision_amd/csrc/kv_engine.h, k_mcts_root / k_mcts_choose /
k_mcts_carry / k_mcts_targets in kv_mcts.hip, the per-slot targets of the
several-leaves sim-step in kv_search.hip) over the oracle's rules.

Every ply of a game is searched to a visit target of its own: `sims` on a full
ply, `fast_sims` on a fast one, the kind a pure function of the value the
game's two streams are seeded with and the ply (kind / target below). The root
is built as ever -- the Dirichlet draw is made at every root -- and a fast ply
mixes it in with eps = 0.

The game loops are those of tests/_mcts_selfplay_reuse.py (one leaf, trees built
from nothing or carried; a carried root that already holds a fast ply's target
runs no step, rem = 0) and tests/_mcts_selfplay_leaves.py (several leaves, the
step's budget min(leaves, target - done)), built from the pieces they export:
_Node, root_priors with the ply's eps, leaf_priors, policy_index and the endings
of tests/_mcts_endings.py. They return what those return, plus per ply `full`,
`target`, `kept` and `rem`. With every ply full (full_q16 = 65536) they are those
two restatements ply for ply (tests/test_mcts_pcr_cpu.py), which chains them to
the C oracle. Shared by tests/test_mcts_pcr_cpu.py and tests/test_mcts_pcr_gpu.py;
not a test module itself."""
import numpy as np

from oracle import oracle as O

from tests import _mcts_endings as E
from tests import _mcts_search as S
from tests import _mcts_selfplay_leaves as L
from tests import _mcts_selfplay_reuse as R
from tests._mcts_search import leaf_priors, policy_index, root_priors
from tests._mcts_selfplay_reuse import hash_eval, net_eval  # noqa: F401  (also this module's names)

F = np.float32
M64 = (1 << 64) - 1

# The runs tests/test_mcts_pcr_gpu.py compares with this restatement (the engine's seed; game g's streams and kind
# key are seed + g), picked on the CPU: tests/test_mcts_pcr_cpu.py asserts that at Q16 the hash-evaluator games
# (SEED, 6 games x 12 plies) hold both kinds and, with reuse on at 2 / 64 sims, a ply with rem = 0, and that the
# network games (NET_SEED, 17 games x 6 plies) hold both kinds in games 0-3 and a ply at which all 17 are fast.
SEED, NET_SEED, Q16 = 49, 129, 16384


def kind(key, ply, full_q16):
    """True: ply `ply` of the game whose streams are seeded `key` (the engine's seed + the game id) is full."""
    x = ((key & M64) * 0x9E3779B97F4A7C15 + ((ply + 1) & M64) * 0xD1B54A32D192ED03) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return (x >> 48) < full_q16


def target(key, ply, sims, fast_sims, full_q16):
    """(full, the ply's visit target); fast_sims 0: the feature is off, every ply full."""
    full = fast_sims == 0 or kind(key, ply, full_q16)
    return full, (sims if full else fast_sims)


def play(seed, sims, plies, reuse, fast_sims, full_q16, evaluate=hash_eval, **kw):
    """tests/_mcts_selfplay_reuse.play with per-ply targets: one leaf, `reuse` False (every tree built from
    nothing) or True. The per-ply dicts gain full, target, and rem = max(target - kept, 0)."""
    g = _play(seed, sims, plies, reuse, fast_sims, full_q16, **kw)
    try:
        st = next(g)
        while True:
            st = g.send(evaluate(st))
    except StopIteration as done:
        return done.value


def play_many(seeds, sims, plies, reuse, fast_sims, full_q16, evaluate_many, **kw):
    """play() of several games whose evaluations go out together (tests/_mcts_selfplay_reuse.play_many)."""
    gens = [_play(s, sims, n, reuse, fast_sims, full_q16, **kw) for s, n in zip(seeds, plies)]
    out, want = [None] * len(gens), {}
    for k, g in enumerate(gens):
        try:
            want[k] = next(g)
        except StopIteration as done:
            out[k] = done.value
    while want:
        ks = sorted(want)
        got = evaluate_many([want[k] for k in ks])
        for k, r in zip(ks, got):
            try:
                want[k] = gens[k].send(r)
            except StopIteration as done:
                out[k] = done.value
                del want[k]
    return out


def _play(seed, sims, plies, reuse, fast_sims, full_q16, c_puct=1.5, eps=0.25, alpha=0.3, start=None,
          max_moves=None):
    """The one-leaf game as a generator: yields each position to evaluate, is sent (logits, value)."""
    c = F(c_puct)
    np_mt, py_mt = O.MT(seed, "numpy"), O.MT(seed, "python")
    sqt = [F(np.sqrt(np.float64(k))) for k in range(sims + 4)]
    vec = E.start_state(start)
    root, root_n, root_wtm = None, 1, 1
    out = E.Played()
    ply = -1
    while plies is None or ply + 1 < plies:
        ply += 1
        moves3, st = O.valid_moves(vec)
        if plies is None and len(moves3) == 0:
            return E.finish(out, ply, E.no_moves(st), False)
        assert len(moves3) > 0, "the game the device recorded goes on here"
        words = S.move_words(st, moves3)
        full, tgt = target(seed, ply, sims, fast_sims, full_q16)
        logits, root_value = yield st
        priors = root_priors(logits, words, np_mt, eps if full else 0.0, alpha)  # the draw is made either way
        carried = root is not None
        if root is None:
            root, root_n, root_wtm = R._Node(st, words, priors), 1, int(st[64])
        else:  # a carried tree: node 0 keeps N, W and its children and takes only the fresh priors
            assert root.words == words, "the carried root's move words are not the position's move list"
            assert root_wtm == int(st[64])
            root.P = np.asarray(priors, dtype=F)
        kept = root_n - 1
        rem = max(tgt - kept, 0)  # 0: a fast ply whose carried root already holds its target
        pending = []
        for _ in range(rem):
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
            v, sent = F(0.0), False
            if not O.is_draw(ls):
                lm, lst = O.valid_moves(ls)
                if len(lm) == 0:
                    v = F((-1.0 if lst[64] else 1.0) if O.in_check(lst) else 0.0)
                else:
                    lw = S.move_words(lst, lm)
                    llog, v = yield lst
                    v = F(v)
                    leaf_node.child[leaf_j] = R._Node(lst, lw, leaf_priors(llog, lw))
                    sent = True
            pending.append(sent)
            for d, (nd, j) in enumerate(path):
                white_moved = (root_wtm != 0) ^ bool(d & 1)
                nd.N[j] += 1
                nd.W[j] = nd.W[j] + (v if white_moved else -v)
            root_n += 1
        visits = [int(x) for x in root.N]
        assert sum(visits) == max(tgt, kept)
        total = np.float64(0.0)
        for x in visits:
            total = total + np.float64(x)
        pick = py_mt.choices_index(np.array(visits, dtype=np.float64) / total)
        out.append(dict(visits=visits, words=list(words), move=policy_index(words[pick]), kept=kept, rem=rem,
                        carried=carried, pending=pending, nodes=R._count_nodes(root), played_n=visits[pick],
                        full=full, target=tgt))
        out.extra.append(dict(board=bytes(st[:64]), root_value=F(root_value),
                              child_kept=bool(reuse) and root.child[pick] is not None))
        vec = O.make_valid_move(vec, pick)
        if plies is None:
            end = E.after_move(vec, ply + 1, root_value, max_moves)
            if end is not None:
                return E.finish(out, ply + 1, end, True)
        child = root.child[pick] if reuse else None
        if child is None:  # dropped: the next ply builds a fresh root
            root, root_n = None, 1
        else:  # carried: the child is the root, its visit count the played edge's
            root, root_n, root_wtm = child, visits[pick], 1 - root_wtm
    return out


def leaves_game(seed, sims, plies, leaves, fast_sims, full_q16, c_puct=1.5, eps=0.25, alpha=0.3, start=None,
                max_moves=None):
    """tests/_mcts_selfplay_leaves.game (self-play: one player, every ply drawn) with per-ply targets, the same
    generator protocol: yields ("root", 0, state) and ("step", 0, [pending leaf states]). The per-ply dicts gain
    full, target, kept (0: every tree is built from nothing) and rem (the target)."""
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
        full, tgt = target(seed, ply, sims, fast_sims, full_q16)
        logits, root_value = yield "root", L.A, st
        root = L._Node(st, words, root_priors(logits, words, np_mt, eps if full else 0.0, alpha))
        root_n, done = 1, 0
        acc_steps, pend_steps = [], []
        while done < tgt:
            r = min(leaves, tgt - done)
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
            rows = yield "step", L.A, [val[0] for _, pending, val in accepted if pending]
            rows = iter(rows)
            for path, pending, val in accepted:
                if pending:
                    llog, v = next(rows)
                    v = F(v)
                    lst, lw = val
                    leaf_node, leaf_j = path[-1]
                    leaf_node.child[leaf_j] = L._Node(lst, lw, leaf_priors(llog, lw))
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
        assert sum(visits) == tgt
        total = np.float64(0.0)
        for x in visits:
            total = total + np.float64(x)
        pick = py_mt.choices_index(np.array(visits, dtype=np.float64) / total)
        out.append(dict(player=L.A, visits=visits, words=list(words), move=policy_index(words[pick]), sampled=True,
                        accepted=acc_steps, leaf_pending=pend_steps, root_value=F(root_value), full=full,
                        target=tgt, kept=0, rem=tgt))
        out.extra.append(dict(board=bytes(st[:64])))
        vec = O.make_valid_move(vec, pick)
        if plies is None:
            end = E.after_move(vec, ply + 1, root_value, max_moves)
            if end is not None:
                return E.finish(out, ply + 1, end, True)
    return out


def play_leaves(seed, sims, plies, leaves, fast_sims, full_q16, evaluate=hash_eval, **kw):
    """leaves_game() with one evaluator, evaluate(state) -> (logits[4096], value)."""
    g = leaves_game(seed, sims, plies, leaves, fast_sims, full_q16, **kw)
    try:
        what, _, req = next(g)
        while True:
            what, _, req = g.send(evaluate(req) if what == "root" else [evaluate(st) for st in req])
    except StopIteration as done:
        return done.value
