"""Plain-Python restatement of the position search (DESIGN.md "MCTS semantics",
knightvision_amd/csrc/kv_search.hip) over the oracle's rules, for any
evaluator: evaluate(list of states after getValidMoves) -> [(logits[4096],
value)], one call for the root and one per sim-step for the step's pending
leaves in descent order, as the device batches them. The root's priors are
k_mcts_root's (root_priors: the softmax over the 4,096 logits, restricted to
the legal moves, mixed with the Dirichlet noise of the position's own stream
and renormalised in double), an expanded leaf's are the backup's (leaf_priors:
the softmax over the legal logits only). Without an evaluator it is the hash
test evaluator: all logits 0, so the leaf priors are exactly 1/n and the
root's (eps = 0) the float of the double 1/n; the value of a position is the
FNV-1a hash of the 64 board codes after getValidMoves, as k_hash_eval computes
it. Every score is built from numpy float32 scalars in the kernel's operation
order, so visit counts, q, priors and the principal variation must equal the
device's bit for bit. Shared by the test_mcts_search_* / test_mcts_session_*
modules and tests/_mcts_selfplay_reuse.py; not a test module itself."""
import functools

import numpy as np

from oracle import oracle as O

F = np.float32
SEARCHED, CHECKMATED, STALEMATE, DRAW = 0, 1, 2, 3


def hash_value(codes) -> np.float32:
    """k_hash_eval's value of a 64-code board."""
    h = 2166136261
    for q in codes:
        h ^= int(q) & 0xFF
        h = (h * 16777619) & 0xFFFFFFFF
    return F(F((h % 129) - 64) / F(64.0))


def hash_eval(states):
    """KV_EVAL_HASH's rows of positions (after getValidMoves): all logits 0, the board's hash value."""
    return [(np.zeros(4096, dtype=F), hash_value(st[:64])) for st in states]


def synthetic_logits(codes):
    """4,096 non-uniform logits of a 64-code board: multiples of 1/8 in [-4, 4), the level of logit i taken
    from a multiplicative mix of the board's FNV-1a hash and i. Dyadic, so every difference of two is exact."""
    h = 2166136261
    for q in codes:
        h ^= int(q) & 0xFF
        h = (h * 16777619) & 0xFFFFFFFF
    x = (np.arange(4096, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(h)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    return ((x & np.uint64(63)).astype(F) / F(8.0) - F(4.0)).astype(F)


def synthetic_eval(state):
    """A deterministic evaluator of one position (after getValidMoves) for the CPU tests: synthetic_logits
    and the board's hash value."""
    return synthetic_logits(state[:64]), hash_value(state[:64])


def synthetic_eval_many(states):
    """synthetic_eval as search()'s evaluate."""
    return [synthetic_eval(st) for st in states]


def synthetic_eval_planes(planes):
    """synthetic_eval as oracle.mcts_play_game's eval_fn: planes[n, 12, 8, 8] -> logits[n, 4096], values[n]."""
    planes = np.asarray(planes, dtype=F).reshape(-1, 12, 64)
    codes = np.zeros((planes.shape[0], 64), dtype=np.int8)
    b, c, s = np.nonzero(planes)
    codes[b, s] = c + 1
    rows = [synthetic_eval(cd) for cd in codes]
    return np.stack([lg for lg, _ in rows]), np.array([v for _, v in rows], dtype=F)


def rotated(evaluate):
    """The evaluator that hands every row of a call its neighbour's logits (row k gets row k + 1's, the last
    the first's) and keeps the values: what a search that pairs a step's leaves with the wrong logits rows
    computes. The inputs of the multi-leaf tests must tell it from `evaluate`."""
    def ev(states):
        rows = evaluate(states)
        return [(rows[(k + 1) % len(rows)][0], rows[k][1]) for k in range(len(rows))]
    return ev


def policy_index(word):
    return (word & 63) * 64 + ((word >> 6) & 63)


def root_priors(logits, words, np_mt, eps, alpha):
    """k_mcts_root: softmax with det_expf over the 4,096 logits, the reference's mixed legal weights
    (fp32 keep x p + fp64 eps x Dirichlet), normalised by their serial sum, one rounding to float."""
    probs = O.softmax_det_4096(logits)
    noise, _ = np_mt.dirichlet(alpha, 4096)
    keep = F(1.0 - eps)
    w = []
    for wd in words:
        idx = policy_index(wd)
        w.append(np.float64(F(keep * probs[idx])) + np.float64(eps) * noise[idx])
    total = np.float64(0.0)
    for x in w:
        total = total + x
    n = len(words)
    if total == 0.0:
        return [F(1.0) / F(n)] * n
    return [F(x / total) for x in w]


def leaf_priors(logits, words):
    """mcts_backup_slot: softmax over the legal moves' logits only; lane l sums entries l, l + 64, ... in
    order, then the xor butterfly over the 64 lanes."""
    lg = np.array([logits[policy_index(wd)] for wd in words], dtype=F)
    n = len(lg)
    mx = lg.max()
    e = np.array([O.det_expf(float(F(x - mx))) for x in lg], dtype=F)
    part = np.zeros(64, dtype=F)
    for lane in range(64):
        s = F(0.0)
        for j in range(lane, n, 64):
            s = F(s + e[j])
        part[lane] = s
    m = 32
    while m >= 1:
        part = (part + part[np.arange(64) ^ m]).astype(F)
        m >>= 1
    total = part[0]
    if total > 0:
        return (e / total).astype(F)
    return np.full(n, F(1.0) / F(n), dtype=F)


def move_words(state, moves3):
    """The device's move words (from | to << 6 | flags << 12; flags bit 0 ep, 1 castle, 2 promotion, 3 king
    move) of an oracle move list of `state`."""
    return [int(fr) | (int(to) << 6) | ((int(fl) | (8 if state[fr] in (1, 7) else 0)) << 12)
            for fr, to, fl in moves3]


def make_state(pieces, wtm):
    """An 80-byte state vector from {square (row * 8 + col, row 0 = rank 8): code}; every castling piece
    counts as moved, no en-passant square."""
    v = np.zeros(80, dtype=np.int8)
    for sq, code in pieces.items():
        v[sq] = code
    wk = [s for s, c in pieces.items() if c == 1][0]
    bk = [s for s, c in pieces.items() if c == 7][0]
    v[64] = 1 if wtm else 0
    v[65:69] = (wk // 8, wk % 8, bk // 8, bk % 8)
    v[69:75] = 1
    v[75:77] = -1
    return v


def sq(name):
    return (8 - int(name[1])) * 8 + "abcdefgh".index(name[0])


# codes: 1..6 white K Q R B N p, 7..12 black K Q R B N p
ONE_MOVE = make_state({sq("a1"): 1, sq("a8"): 9, sq("c3"): 7}, True)          # Ka1 in check, b1 the one escape
MATE_IN_ONE = make_state({sq("g1"): 1, sq("a1"): 3, sq("g8"): 7, sq("f7"): 12, sq("g7"): 12, sq("h7"): 12}, True)
KPK_CAPTURE = make_state({sq("e1"): 1, sq("e4"): 6, sq("e5"): 7}, False)      # ...Kxe4 leaves kings only
CHECKMATED_ROOT = make_state({sq("g1"): 1, sq("a8"): 3, sq("g8"): 7, sq("f7"): 12, sq("g7"): 12, sq("h7"): 12},
                             False)
STALEMATE_ROOT = make_state({sq("f7"): 1, sq("g6"): 2, sq("h8"): 7}, False)
KINGS_ONLY_ROOT = make_state({sq("e1"): 1, sq("e8"): 7}, True)
# Roots wider than a wavefront, found by tools/find_wide_positions.py (seeded): queens on both sides, white to
# move, black's king walled in on a1 so that no root move mates. 96, 137 and 206 root moves; WIDE_A and WIDE_B
# have children of more than 64 moves (tests/test_mcts_wide_cpu.py asserts what the GPU tests rely on).
WIDE_A = make_state({2: 2, 3: 2, 5: 2, 8: 1, 13: 2, 14: 8, 16: 2, 17: 2, 22: 2, 26: 8, 28: 8, 31: 8, 33: 8, 36: 2,
                     40: 6, 41: 6, 42: 6, 45: 8, 48: 12, 49: 12, 50: 6, 51: 2, 56: 7, 57: 10, 58: 6}, True)
WIDE_B = make_state({4: 2, 8: 8, 9: 2, 14: 2, 15: 1, 16: 2, 19: 2, 20: 2, 21: 2, 25: 8, 32: 8, 34: 2, 35: 8, 38: 8,
                     40: 6, 41: 6, 42: 6, 44: 2, 46: 2, 48: 12, 49: 12, 50: 6, 52: 2, 53: 8, 56: 7, 57: 10, 58: 6,
                     61: 2, 62: 2}, True)
WIDE_C = make_state({0: 2, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 8, 7: 2, 8: 2, 14: 2, 16: 2, 20: 2, 23: 2, 26: 2, 31: 2,
                     32: 1, 33: 2, 39: 2, 40: 6, 41: 6, 42: 6, 43: 2, 45: 2, 47: 2, 48: 12, 49: 12, 50: 6, 51: 2,
                     55: 2, 56: 7, 57: 10, 58: 6, 60: 2, 62: 2, 63: 8}, True)


class _Node:
    __slots__ = ("state", "words", "P", "N", "V", "W", "child", "cstate")

    def __init__(self, state, words, priors):
        n = len(words)
        self.state = state  # after getValidMoves
        self.words = words
        self.P = [F(p) for p in priors]
        assert len(self.P) == n
        self.N = [0] * n
        self.V = [0] * n
        self.W = [F(0.0)] * n
        self.child = [None] * n
        self.cstate = [None] * n


def fresh_root_row(evaluate, st, words, eps=0.0, alpha=0.3, seed=0):
    """(priors, value) of a root built from nothing (k_mcts_root on the position's network row; seed: the
    position's own numpy stream, k_search_load's seed + i). Without an evaluator and at eps = 0 the closed form
    of the hash evaluator's row: every weight 2^-12, normalised in double, one rounding to float."""
    if evaluate is None and eps == 0.0:
        n = len(words)
        return [F(np.float64(2.0 ** -12) / (np.float64(n) * np.float64(2.0 ** -12)))] * n, hash_value(st[:64])
    logits, value = (evaluate or hash_eval)([st])[0]
    return root_priors(logits, words, O.MT(seed, "numpy"), eps, alpha), F(value)


def leaf_rows_of(evaluate, pending):
    """[(priors, value)] of a sim-step's pending leaves [(state after getValidMoves, move words)], evaluated
    together in descent order (the step's network batch). Without an evaluator the hash evaluator's closed
    form: e = 1 for every move, their sum n."""
    if evaluate is None:
        return [([F(1.0) / F(len(w))] * len(w), hash_value(lst[:64])) for lst, w in pending]
    if not pending:
        return []
    rows = evaluate([lst for lst, _ in pending])
    assert len(rows) == len(pending)
    return [(leaf_priors(lg, w), F(v)) for (lg, v), (_, w) in zip(rows, pending)]


def search(state, sims, leaves=1, c_puct=1.5, ncap=None, evaluate=None, eps=0.0, alpha=0.3, seed=0, depths=False):
    """-> dict(status, visits, q, prior, moves, best, pv, steps, nn_rows, root_value, sims: the root's visits,
    accepted: the descents each sim-step accepted). evaluate(list of states after getValidMoves) -> [(logits[4096] float32, value
    float32)], None: the hash evaluator; seed: the position's own stream (the call's seed + its index).
    depths: the dict also holds `depths`, per sim-step the path lengths of its accepted descents."""
    c = F(c_puct)
    ncap = sims + 2 if ncap is None else ncap
    state = np.array(state, dtype=np.int8)
    term = dict(visits=[], q=[], prior=[], moves=[], best=-1, pv=[], steps=0, nn_rows=0, accepted=[], sims=0)
    if O.is_draw(state):
        return dict(term, status=DRAW, root_value=F(0.0))
    moves3, st = O.valid_moves(state)
    if len(moves3) == 0:
        if O.in_check(st):
            return dict(term, status=CHECKMATED, root_value=F(-1.0 if st[64] else 1.0))
        return dict(term, status=STALEMATE, root_value=F(0.0))
    n = len(moves3)
    words = move_words(st, moves3)
    priors, root_value = fresh_root_row(evaluate, st, words, eps, alpha, seed)
    root = _Node(st, words, priors)
    root_wtm = int(st[64])
    root_n, done, steps, leaf_rows, per_step, path_lens = 1, 0, 0, 0, [], []
    sqt = [F(np.sqrt(np.float64(k))) for k in range(sims + 4)]
    while done < sims:
        r = min(leaves, sims - done)
        vroot = 0
        accepted = []  # (path, pending, value or (leaf state after getValidMoves, moves))
        held = []
        for _ in range(r):
            node, n_par, path = root, root_n + vroot, []
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
                if child is None or len(path) >= ncap:
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
        batch = [(val[0], move_words(*val)) for _, pending, val in accepted if pending]
        rows = iter(zip(batch, leaf_rows_of(evaluate, batch)))
        for path, pending, val in accepted:
            if pending:
                (lst, lw), (lp, v) = next(rows)
                leaf_node, leaf_j = path[-1]
                leaf_node.child[leaf_j] = _Node(lst, lw, lp)
                leaf_rows += 1
            else:
                v = val
            for d, (nd, j) in enumerate(path):
                white_moved = (root_wtm != 0) ^ bool(d & 1)
                nd.V[j] -= 1
                nd.N[j] += 1
                nd.W[j] = nd.W[j] + (v if white_moved else -v)
            root_n += 1
        done += len(accepted)
        steps += 1
        per_step.append(len(accepted))
        path_lens.append([len(path) for path, _, _ in accepted])
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
    more = dict(depths=path_lens) if depths else {}
    return dict(status=SEARCHED, visits=visits, q=q, prior=list(root.P), moves=list(root.words),
                best=visits.index(max(visits)), pv=pv, steps=steps, nn_rows=1 + leaf_rows, accepted=per_step,
                root_value=root_value, sims=done, **more)


def oracle_positions(n_games, plies, sims, eval_fn=None, seed0=42):
    """The positions of the first `plies` plies of `n_games` oracle games at eps = 0 (game g seeded seed0 + g)
    and the oracle's root visit vector of each: [(state[80], visits[MAXM])]."""
    out = []
    for g in range(n_games):
        r = O.mcts_play_game(sims, O.MT(seed0 + g, "numpy"), O.MT(seed0 + g, "python"), eval_fn, max_moves=plies,
                             c_puct=1.5, eps=0.0)
        st = O.initial_state()
        for p in range(len(r["moves"])):
            out.append((st.copy(), r["visits"][p].copy()))
            moves3, _ = O.valid_moves(st)
            idx = [int(fr) * 64 + int(to) for fr, to, _ in moves3].index(int(r["moves"][p]))
            st = O.make_valid_move(st, idx)
    return out


@functools.lru_cache(maxsize=None)
def hash_positions():
    """3 games x 6 plies at 48 sims with the hash evaluator: the 18 positions both test files use."""
    return oracle_positions(3, 6, 48)


@functools.lru_cache(maxsize=None)
def synthetic_positions():
    """The same 3 games x 6 plies at 48 sims played with the synthetic evaluator: other games, as the priors
    differ."""
    return oracle_positions(3, 6, 48, synthetic_eval_planes)
