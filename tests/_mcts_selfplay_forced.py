"""Plain-Python restatement of MCTS self-play with forced playouts and policy
target pruning (DESIGN.md "Forced playouts and policy target pruning",
kv_config.forced_k; forced_edge in knightvision_amd/csrc/kv_engine.h,
mcts_select_slot / pruned_count / k_mcts_choose in kv_mcts.hip,
search_select_tree in kv_search.hip) over the oracle's rules.

On a full ply a root edge that holds n > 0 visits (the descents in flight
counting) while n * n < (k * P) * S -- S the root's visit sum as the descent sees
it -- scores +inf, so the first such edge in list order is taken. At the move
choice the forced visits PUCT would not have made are taken out again (prune):
the move is drawn from the pruned counts T, the raw counts N stay what the
records, the carried subtree and every counter see. A fast ply of fast_sims has
no forcing and T = N.

The game loops are those of tests/_mcts_selfplay_pcr.py (one leaf, trees built
from nothing or carried, per-ply targets; several leaves), built from the pieces
it and the older restatements export. They return what those return, plus per
ply `targets` (T), `forced` (the accepted descents at whose root an edge was
forced), `pruned` (sum N - sum T), `raw_pick` (the root edge the same draw would
have picked from the raw counts) and `pick`, and two figures the CPU tests use to
show that the GPU tests' seeds exercise the rule: `forced_diff` (descents whose
forced edge is not the plain PUCT first maximum) and `v_decides` (descents at
which an edge is forced on N + V and not on N alone, or the other way round).
With forced_k = 0 they are tests/_mcts_selfplay_pcr.py's games ply for ply
(tests/test_mcts_forced_cpu.py), which chains them to the C oracle. Shared by
tests/test_mcts_forced_cpu.py and tests/test_mcts_forced_gpu.py; not a test
module itself."""
import ctypes as C

import numpy as np

from oracle import oracle as O

from tests import _mcts_endings as E
from tests import _mcts_search as S
from tests import _mcts_selfplay_leaves as L
from tests import _mcts_selfplay_pcr as P
from tests import _mcts_selfplay_reuse as R
from tests._mcts_search import leaf_priors, policy_index, root_priors
from tests._mcts_selfplay_reuse import hash_eval, net_eval  # noqa: F401  (also this module's names)

F = np.float32
ADDED = ("targets", "forced", "pruned", "raw_pick", "pick", "forced_diff", "v_decides")

# The runs tests/test_mcts_forced_gpu.py compares with this restatement, picked on the CPU
# (tests/test_mcts_forced_cpu.py asserts what they hold): the engine's seed, game g's streams seeded SEED + g.
SEED, NET_SEED, K, Q16 = 49, 129, 2.0, P.Q16
GAMES = 4
HASH_RUNS = {
    "fresh": dict(sims=48, plies=10, reuse=False, fast=0, leaves=0),
    "carried": dict(sims=48, plies=10, reuse=True, fast=0, leaves=0),
    "pcr": dict(sims=48, plies=12, reuse=False, fast=4, leaves=0),
    "leaves": dict(sims=48, plies=10, reuse=False, fast=0, leaves=4),
}


def forced_mask(k, prior, n, total):
    """forced_edge over a node's edges: n > 0 and n * n < (k * P) * S, in fp32."""
    n = np.asarray(n)
    nf = n.astype(F)
    thr = ((F(k) * np.asarray(prior, dtype=F)).astype(F) * F(total)).astype(F)
    return (n > 0) & ((nf * nf).astype(F) < thr)


def prune(k, c, prior, visits, value_sums, sq):
    """pruned_count over a root's edges -> T (list of ints). c, sq: fp32 scalars (c_puct, sqrt_tab[root N])."""
    c, sq, k = F(c), F(sq), F(k)
    visits = [int(x) for x in visits]
    n = len(visits)
    total = sum(visits)
    b = visits.index(max(visits)) if n else 0
    q_b = F(value_sums[b]) / F(visits[b]) if visits[b] > 0 else F(0.0)
    best = F(q_b + F(F(F(c * F(prior[b])) * sq) / F(1 + visits[b])))
    out = []
    for j in range(n):
        nj = visits[j]
        if j == b or nj == 0:
            out.append(nj)
            continue
        pj = F(prior[j])
        thr = F(F(k * pj) * F(total))
        f = 0
        while f < nj and F(F(f) * F(f)) < thr:
            f += 1
        q = F(F(value_sums[j]) / F(nj))
        t = nj
        for _ in range(f):
            s = F(q + F(F(F(c * pj) * sq) / F(1 + (t - 1))))
            if not s < best:
                break
            t -= 1
        if t < nj and t == 1:
            t = 0
        out.append(t)
    return out


def _twin(mt):
    """A copy of an oracle MT19937 stream at its present position."""
    tw = O.MT(0, "python")
    C.memmove(tw.buf, mt.buf, len(mt.buf))
    return tw


def _choose(py_mt, visits, targets, sampled):
    """The move choice over the pruned counts -> (pick, the pick the same draw gives on the raw counts)."""
    if not sampled:
        return targets.index(max(targets)), visits.index(max(visits))
    tw = _twin(py_mt)

    def draw(mt, counts):
        total = np.float64(0.0)
        for x in counts:
            total = total + np.float64(x)
        return mt.choices_index(np.array(counts, dtype=np.float64) / total)

    return draw(py_mt, targets), draw(tw, visits)


def play(seed, sims, plies, reuse, fast_sims, full_q16, forced_k, evaluate=hash_eval, **kw):
    """tests/_mcts_selfplay_pcr.play with the forced rule and the pruning: one leaf, `reuse` False or True."""
    g = _play(seed, sims, plies, reuse, fast_sims, full_q16, forced_k, **kw)
    try:
        st = next(g)
        while True:
            st = g.send(evaluate(st))
    except StopIteration as done:
        return done.value


def play_many(seeds, sims, plies, reuse, fast_sims, full_q16, forced_k, evaluate_many, **kw):
    """play() of several games whose evaluations go out together (tests/_mcts_selfplay_pcr.play_many)."""
    gens = [_play(s, sims, n, reuse, fast_sims, full_q16, forced_k, **kw) for s, n in zip(seeds, plies)]
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


def _play(seed, sims, plies, reuse, fast_sims, full_q16, forced_k, c_puct=1.5, eps=0.25, alpha=0.3, start=None,
          max_moves=None, sample_plies=0):
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
        full, tgt = P.target(seed, ply, sims, fast_sims, full_q16)
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
        force = forced_k > 0 and full  # a fast ply has no forcing
        pending, forced, forced_diff = [], 0, 0
        for _ in range(rem):
            node, n_par, path = root, root_n, []
            while True:
                u = c * node.P * sqt[n_par] / (1 + node.N).astype(F)
                q = np.where(node.N > 0, node.W / np.maximum(node.N, 1).astype(F), F(0.0)).astype(F)
                sc = (q + u).astype(F)
                if force and node is root:
                    mask = forced_mask(forced_k, node.P, node.N, root_n - 1)
                    if mask.any():
                        forced += 1
                        forced_diff += int(np.argmax(mask)) != int(np.argmax(sc))
                        sc = np.where(mask, F(np.inf), sc)
                bi = int(np.argmax(sc))  # the first maximum in list order
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
        targets = prune(forced_k, c, root.P, visits, root.W, sqt[root_n]) if force else list(visits)
        sampled = sample_plies == 0 or (sample_plies > 0 and ply < sample_plies)
        pick, raw_pick = _choose(py_mt, visits, targets, sampled)
        out.append(dict(visits=visits, words=list(words), move=policy_index(words[pick]), kept=kept, rem=rem,
                        carried=carried, pending=pending, nodes=R._count_nodes(root), played_n=visits[pick],
                        full=full, target=tgt, targets=targets, forced=forced, pruned=sum(visits) - sum(targets),
                        raw_pick=raw_pick, pick=pick, forced_diff=forced_diff, v_decides=0))
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
        else:  # carried: the child is the root, its visit count the played edge's raw one
            root, root_n, root_wtm = child, visits[pick], 1 - root_wtm
    return out


def leaves_game(seed, sims, plies, leaves, fast_sims, full_q16, forced_k, c_puct=1.5, eps=0.25, alpha=0.3,
                start=None, max_moves=None, sample_plies=0):
    """tests/_mcts_selfplay_pcr.leaves_game with the forced rule on N + V and the root's visit sum root_n + vroot
    - 1, and the pruning; the same generator protocol."""
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
        full, tgt = P.target(seed, ply, sims, fast_sims, full_q16)
        logits, root_value = yield "root", L.A, st
        root = L._Node(st, words, root_priors(logits, words, np_mt, eps if full else 0.0, alpha))
        root_n, done = 1, 0
        force = forced_k > 0 and full
        acc_steps, pend_steps, forced, forced_diff, v_decides = [], [], 0, 0, 0
        while done < tgt:
            r = min(leaves, tgt - done)
            vroot, accepted, held = 0, [], []
            for _ in range(r):
                node, n_par, path = root, root_n + vroot, []
                by_force = differs = by_v = False
                while True:
                    nv = node.N + node.V
                    u = c * node.P * sqt[n_par] / (1 + nv).astype(F)
                    q = np.where(nv > 0, (node.W - node.V.astype(F)) / np.maximum(nv, 1).astype(F), F(0.0)).astype(F)
                    sc = (q + u).astype(F)
                    if force and node is root:
                        mask = forced_mask(forced_k, node.P, nv, root_n + vroot - 1)
                        by_v = bool((mask != forced_mask(forced_k, node.P, node.N, root_n + vroot - 1)).any())
                        if mask.any():
                            by_force = True
                            differs = int(np.argmax(mask)) != int(np.argmax(sc))
                            sc = np.where(mask, F(np.inf), sc)
                    bi = int(np.argmax(sc))  # the first maximum in list order
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
                    break  # collision: dropped, the step's descents end (and it counts nowhere)
                forced += by_force
                forced_diff += differs
                v_decides += by_v
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
        targets = prune(forced_k, c, root.P, visits, root.W, sqt[root_n]) if force else list(visits)
        sampled = sample_plies == 0 or (sample_plies > 0 and ply < sample_plies)
        pick, raw_pick = _choose(py_mt, visits, targets, sampled)
        out.append(dict(player=L.A, visits=visits, words=list(words), move=policy_index(words[pick]), sampled=sampled,
                        accepted=acc_steps, leaf_pending=pend_steps, root_value=F(root_value), full=full,
                        target=tgt, kept=0, rem=tgt, targets=targets, forced=forced,
                        pruned=sum(visits) - sum(targets), raw_pick=raw_pick, pick=pick, forced_diff=forced_diff,
                        v_decides=v_decides))
        out.extra.append(dict(board=bytes(st[:64])))
        vec = O.make_valid_move(vec, pick)
        if plies is None:
            end = E.after_move(vec, ply + 1, root_value, max_moves)
            if end is not None:
                return E.finish(out, ply + 1, end, True)
    return out


def play_leaves(seed, sims, plies, leaves, fast_sims, full_q16, forced_k, evaluate=hash_eval, **kw):
    """leaves_game() with one evaluator, evaluate(state) -> (logits[4096], value)."""
    g = leaves_game(seed, sims, plies, leaves, fast_sims, full_q16, forced_k, **kw)
    try:
        what, _, req = next(g)
        while True:
            what, _, req = g.send(evaluate(req) if what == "root" else [evaluate(st) for st in req])
    except StopIteration as done:
        return done.value
