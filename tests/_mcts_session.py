"""Plain-Python restatement of search sessions (DESIGN.md "Search sessions",
kv_search_advance / kv_search_continue in knightvision_amd/csrc/kv_search.hip)
for any evaluator (tests/_mcts_search.py's: a list of positions -> their logits
and values; none: the hash test evaluator): persistent trees over the oracle's
rules with the scoring loop of tests/_mcts_search.py, advance (re-root on the
played edge's child, or drop the tree) and the top-up continue. A carried root
keeps the priors its node was expanded with (the leaf softmax over the legal
logits) and the value the evaluator gave it then; a dropped tree's root is
built as kv_search builds one (k_mcts_root's priors at eps = 0). Every score is
built from numpy float32 scalars in the kernel's operation order, so visits, q,
priors and the principal variation must equal the device's bit for bit. Shared
by the test_mcts_session_* modules and tests/test_mcts_search_net_gpu.py; not a
test module itself."""
import itertools

import numpy as np

from oracle import oracle as O

from tests import _mcts_search as S

F = np.float32
SEARCHED, CHECKMATED, STALEMATE, DRAW = S.SEARCHED, S.CHECKMATED, S.STALEMATE, S.DRAW
_SESSION = object()  # search / resume: the session's own evaluator


_SERIAL = itertools.count()


class _Node(S._Node):
    __slots__ = ("value", "serial")

    def __init__(self, state, words, priors, value):
        super().__init__(state, words, priors)
        self.value = value  # the evaluator's value of the position, kept for a later re-root
        self.serial = next(_SERIAL)  # creation order: a tree's later node has the larger device id


class _Tree:
    """One position of the session: vec is its state vector as given (or as make_valid_move left it)."""

    def __init__(self, vec):
        self.vec = np.array(vec, dtype=np.int8)
        self.fresh = True  # no root yet: the next run builds it and takes its network row
        self.root = None
        self.root_n = 1
        if O.is_draw(self.vec):
            self.status, self.root_value, self.n_moves = DRAW, F(0.0), 0
            return
        moves3, st = O.valid_moves(self.vec)
        self.n_moves = len(moves3)
        if self.n_moves == 0:
            mated = O.in_check(st)
            self.status = CHECKMATED if mated else STALEMATE
            self.root_value = F((-1.0 if st[64] else 1.0) if mated else 0.0)
            return
        self.status = SEARCHED
        self._st, self._moves3 = st, moves3

    def build_root(self, evaluate):
        # k_mcts_root at eps = 0 on the position's own network row
        words = S.move_words(self._st, self._moves3)
        priors, value = S.fresh_root_row(evaluate, self._st, words)
        self.root = _Node(self._st, words, priors, value)
        self.root_wtm = int(self._st[64])
        self.root_value = self.root.value
        self.root_n = 1
        self.fresh = False

    def nodes(self):
        out, todo = [], [self.root] if self.root is not None and not self.fresh else []
        while todo:
            nd = todo.pop()
            out.append(nd)
            todo.extend(c for c in nd.child if c is not None)
        return out


class Session:
    """search(sims, leaves) / advance(edges) / resume(sims, leaves) / tree_size(i) over n positions, as
    engine.PositionSearch gives them. ncap: the engine's node capacity (max_sims + 2). evaluate: the
    evaluator of tests/_mcts_search.search (None: hash); search and resume take one for their call alone, as
    the network's batch class is the call's."""

    def __init__(self, states, c_puct=1.5, ncap=66, evaluate=None):
        self.c = F(c_puct)
        self.ncap = ncap
        self.evaluate = evaluate
        self.states = [np.array(s, dtype=np.int8) for s in states]
        self.trees = None

    def search(self, sims, leaves=1, evaluate=_SESSION):
        ev = self.evaluate if evaluate is _SESSION else evaluate
        self.trees = [_Tree(s) for s in self.states]
        return [self._run(t, sims, leaves, ev)[0] for t in self.trees]

    def resume(self, sims, leaves=1, evaluate=_SESSION):
        ev = self.evaluate if evaluate is _SESSION else evaluate
        got = [self._run(t, sims, leaves, ev) for t in self.trees]
        return [r for r, _ in got], [k for _, k in got]

    def advance(self, edges):
        """-> the state vectors after the moves (the current ones where the edge is -1)."""
        for t, k in zip(self.trees, edges):
            if k >= 0 and (t.status != SEARCHED or k >= t.n_moves):
                raise IndexError(k)
        for i, k in enumerate(edges):
            if k < 0:
                continue
            t = self.trees[i]
            after = O.make_valid_move(t.vec, k)
            child = None if t.fresh else t.root.child[k]
            if child is None:
                self.trees[i] = _Tree(after)  # dropped: an unvisited edge or a move into a terminal position
                continue
            nt = _Tree.__new__(_Tree)
            nt.vec, nt.fresh, nt.status = after, False, SEARCHED
            nt.root, nt.n_moves = child, len(child.words)
            nt.root_n = t.root.N[k]  # 1 + the sum of the child's own edge visits
            nt.root_wtm = 1 - t.root_wtm
            nt.root_value = child.value
            self.trees[i] = nt
        return [t.vec.copy() for t in self.trees]

    def tree_size(self, i):
        """(nodes, sum of the nodes' edge counts each rounded up to 16)."""
        nodes = self.trees[i].nodes() if self.trees[i].status == SEARCHED else []
        return len(nodes), sum((len(nd.words) + 15) & ~15 for nd in nodes)

    def _run(self, t, sims, leaves, evaluate):
        """The top-up search of one tree -> (result dict as _mcts_search.search's, kept)."""
        if t.status != SEARCHED:
            return dict(status=t.status, visits=[], q=[], prior=[], moves=[], best=-1, pv=[], steps=0, nn_rows=0,
                        accepted=[], root_value=t.root_value, sims=0), 0
        root_row = 0
        if t.fresh:
            t.build_root(evaluate)
            root_row = 1
        c, root = self.c, t.root
        kept = t.root_n - 1
        done, steps, leaf_rows, per_step = kept, 0, 0, []
        sqt = [F(np.sqrt(np.float64(k))) for k in range(max(sims, t.root_n) + leaves + 4)]
        while done < sims:
            r = min(leaves, sims - done)
            vroot = 0
            accepted = []
            held = []
            for _ in range(r):
                node, n_par, path = root, t.root_n + vroot, []
                while True:
                    s = sqt[n_par]
                    best, bi = F(-np.inf), 0
                    for j in range(len(node.words)):
                        nv = node.N[j] + node.V[j]
                        u = c * node.P[j] * s / F(1 + nv)
                        q = (node.W[j] - F(node.V[j])) / F(nv) if nv > 0 else F(0.0)
                        sc = q + u
                        if sc > best:
                            best, bi = sc, j
                    path.append((node, bi))
                    if node.cstate[bi] is None:
                        node.cstate[bi] = O.make_valid_move(node.state, bi)
                    child = node.child[bi]
                    if child is None or len(path) >= self.ncap:
                        break
                    n_par = node.N[bi] + node.V[bi]
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
                        rec = (path, True, (lst, lm))
                        held.append((leaf_node, leaf_j))
                for nd, j in path:
                    nd.V[j] += 1
                vroot += 1
                accepted.append(rec)
            # the step's network batch: its pending leaves in descent order
            batch = [(val[0], S.move_words(*val)) for _, pending, val in accepted if pending]
            rows = iter(zip(batch, S.leaf_rows_of(evaluate, batch)))
            for path, pending, val in accepted:
                if pending:
                    (lst, lw), (lp, v) = next(rows)
                    leaf_node, leaf_j = path[-1]
                    leaf_node.child[leaf_j] = _Node(lst, lw, lp, v)
                    leaf_rows += 1
                else:
                    v = val
                for d, (nd, j) in enumerate(path):
                    white_moved = (t.root_wtm != 0) ^ bool(d & 1)
                    nd.V[j] -= 1
                    nd.N[j] += 1
                    nd.W[j] = nd.W[j] + (v if white_moved else -v)
                t.root_n += 1
            done += len(accepted)
            steps += 1
            per_step.append(len(accepted))
        n = len(root.words)
        visits = list(root.N)
        q = [root.W[j] / F(root.N[j]) if root.N[j] > 0 else F(0.0) for j in range(n)]
        pv, node = [], root
        while len(pv) < 16:
            m = max(node.N)
            if m == 0:
                break
            j = node.N.index(m)
            pv.append(node.words[j])
            if node.child[j] is None:
                break
            node = node.child[j]
        return dict(status=SEARCHED, visits=visits, q=q, prior=list(root.P), moves=list(root.words),
                    best=visits.index(max(visits)), pv=pv, steps=steps, nn_rows=root_row + leaf_rows,
                    accepted=per_step, root_value=t.root_value, sims=t.root_n - 1), kept
