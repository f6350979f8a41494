"""Plain-Python restatement of MCTS self-play with carried subtrees (DESIGN.md
"Carried subtrees in self-play", kv_config.reuse_tree; k_mcts_root / k_mcts_carry
in knightvision_amd/csrc/kv_mcts.hip) over the oracle's rules. The C oracle
plays every move on a tree built from nothing; here the subtree under the move
just played becomes the next ply's tree, its root takes the priors a fresh root
gets (the reference's mixed distribution from the same numpy stream), and the
search tops the root up to `sims` visits.

Built from the oracle's rules (valid_moves, make_valid_move, is_draw,
in_check), its two MT19937 streams (dirichlet, choices_index), its
softmax_det_4096 / det_expf and the fp32 PUCT of tests/_mcts_search.py at one
leaf, every score a numpy float32 operation in the kernel's order. The game is
told how many plies to play (the device's own record count), or (plies=None)
plays to the end by the rules of tests/_mcts_endings.py from any start
position. Shared by tests/test_mcts_reuse_cpu.py and
tests/test_mcts_reuse_gpu.py; not a test module itself."""
import numpy as np

from oracle import oracle as O

from tests import _mcts_endings as E
from tests import _mcts_search as S
from tests._mcts_search import leaf_priors, policy_index, root_priors  # noqa: F401  (also this module's names)

F = np.float32


class _Node:
    __slots__ = ("state", "words", "P", "N", "W", "child", "cstate")

    def __init__(self, state, words, priors):
        n = len(words)
        self.state = state  # after getValidMoves
        self.words = words
        self.P = np.asarray(priors, dtype=F)
        self.N = np.zeros(n, dtype=np.int32)
        self.W = np.zeros(n, dtype=F)
        self.child = [None] * n
        self.cstate = [None] * n


def hash_eval(state):
    """KV_EVAL_HASH's row of a position (after getValidMoves): all logits 0, the board's hash value."""
    return np.zeros(4096, dtype=F), S.hash_value(state[:64])


def net_eval(eval_fn):
    """An evaluator of lists of positions from one of planes (oracle.mcts_play_game's eval_fn:
    planes[n, 12, 8, 8] -> logits[n, 4096], values[n]), for play_many."""
    def ev(states):
        lg, vl = eval_fn(np.stack([O.encode_board(st) for st in states]))
        lg, vl = np.asarray(lg, dtype=F).reshape(len(states), 4096), np.asarray(vl, dtype=F).reshape(-1)
        return [(lg[k], vl[k]) for k in range(len(states))]
    return ev


def _count_nodes(root):
    n, todo = 0, [root]
    while todo:
        nd = todo.pop()
        n += 1
        todo.extend(c for c in nd.child if c is not None)
    return n


def play(seed, sims, plies, reuse, evaluate=hash_eval, **kw):
    """`plies` plies of the game seeded `seed` (both streams), every position evaluated by
    evaluate(state after getValidMoves) -> (logits[4096], value) -> one dict per ply:
    visits (root edge counts, list order), words (the root's move words), move (the record's index
    from * 64 + to), played_n (the played edge's count), carried (the root was a carried tree), kept (root
    visits carried in), rem (sim-steps run = sims - kept), pending (per sim-step: the leaf went to the
    network), nodes (the tree's nodes at the choice); the list's `extra` holds per ply board (the
    root's 64 codes as bytes), root_value and child_kept (the played edge had a child: the tree the next ply of
    the game carries). Keywords: start (the state vector
    the game starts from; None: the initial position), max_moves; plies None: the game is played to its end
    under max_moves by tests/_mcts_endings.py's rules and the list returned is an E.Played with result
    (plies, outcome, reason, reward) and holds."""
    g = _play(seed, sims, plies, reuse, **kw)
    try:
        st = next(g)
        while True:
            st = g.send(evaluate(st))
    except StopIteration as done:
        return done.value


def play_many(seeds, sims, plies, reuse, evaluate_many, **kw):
    """play() of several games (plies: one count per game) whose evaluations go out together:
    evaluate_many(list of states) -> list of (logits, value), one network batch per round as on the device.
    Each game is play()'s own, whatever the others are."""
    gens = [_play(s, sims, n, reuse, **kw) for s, n in zip(seeds, plies)]
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


def _play(seed, sims, plies, reuse, c_puct=1.5, eps=0.25, alpha=0.3, start=None, max_moves=None):
    """The game as a generator: yields each position to evaluate, is sent (logits, value)."""
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
        logits, root_value = yield st
        priors = root_priors(logits, words, np_mt, eps, alpha)
        carried = root is not None
        if root is None:
            root, root_n, root_wtm = _Node(st, words, priors), 1, int(st[64])
        else:  # a carried tree: node 0 keeps N, W and its children and takes only the fresh priors
            assert root.words == words, "the carried root's move words are not the position's move list"
            assert root_wtm == int(st[64])
            root.P = np.asarray(priors, dtype=F)
        kept = root_n - 1
        rem = sims - kept
        assert rem >= 1
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
                    leaf_node.child[leaf_j] = _Node(lst, lw, leaf_priors(llog, lw))
                    sent = True
            pending.append(sent)
            for d, (nd, j) in enumerate(path):
                white_moved = (root_wtm != 0) ^ bool(d & 1)
                nd.N[j] += 1
                nd.W[j] = nd.W[j] + (v if white_moved else -v)
            root_n += 1
        visits = [int(x) for x in root.N]
        total = np.float64(0.0)
        for x in visits:
            total = total + np.float64(x)
        pick = py_mt.choices_index(np.array(visits, dtype=np.float64) / total)
        out.append(dict(visits=visits, words=list(words), move=policy_index(words[pick]), kept=kept, rem=rem,
                        carried=carried, pending=pending, nodes=_count_nodes(root), played_n=visits[pick]))
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
