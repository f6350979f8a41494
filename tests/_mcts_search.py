"""Plain-Python restatement of the position search (DESIGN.md "MCTS semantics",
knightvision_amd/csrc/kv_search.hip) over the oracle's rules, for the hash test
evaluator: all logits 0, so the leaf priors are exactly 1/n and the root's
(eps = 0) the float of the double 1/n; the value of a position is the FNV-1a
hash of the 64 board codes after getValidMoves, as k_hash_eval computes it.
Every score is built from numpy float32 scalars in the kernel's operation
order, so visit counts, q and the principal variation must equal the
device's bit for bit. Shared by tests/test_mcts_search_cpu.py and
tests/test_mcts_search_gpu.py; not a test module itself."""
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


class _Node:
    __slots__ = ("state", "words", "P", "N", "V", "W", "child", "cstate")

    def __init__(self, state, words, prior):
        n = len(words)
        self.state = state  # after getValidMoves
        self.words = words
        self.P = [prior] * n
        self.N = [0] * n
        self.V = [0] * n
        self.W = [F(0.0)] * n
        self.child = [None] * n
        self.cstate = [None] * n


def search(state, sims, leaves=1, c_puct=1.5, ncap=None):
    """-> dict(status, visits, q, prior, moves, best, pv, steps, nn_rows, root_value, accepted: the descents
    each sim-step accepted)."""
    c = F(c_puct)
    ncap = sims + 2 if ncap is None else ncap
    state = np.array(state, dtype=np.int8)
    term = dict(visits=[], q=[], prior=[], moves=[], best=-1, pv=[], steps=0, nn_rows=0, accepted=[])
    if O.is_draw(state):
        return dict(term, status=DRAW, root_value=F(0.0))
    moves3, st = O.valid_moves(state)
    if len(moves3) == 0:
        if O.in_check(st):
            return dict(term, status=CHECKMATED, root_value=F(-1.0 if st[64] else 1.0))
        return dict(term, status=STALEMATE, root_value=F(0.0))
    n = len(moves3)
    # k_mcts_root at eps = 0: every weight 2^-12, normalised in double, one rounding to float
    root = _Node(st, move_words(st, moves3), F(np.float64(2.0 ** -12) / (np.float64(n) * np.float64(2.0 ** -12))))
    root_wtm = int(st[64])
    root_n, done, steps, leaf_rows, per_step = 1, 0, 0, 0, []
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
        for path, pending, val in accepted:
            if pending:
                lst, lm = val
                v = hash_value(lst[:64])
                leaf_node, leaf_j = path[-1]
                leaf_node.child[leaf_j] = _Node(lst, move_words(lst, lm), F(1.0) / F(len(lm)))
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
                best=visits.index(max(visits)), pv=pv, steps=steps, nn_rows=1 + leaf_rows, accepted=per_step,
                root_value=hash_value(st[:64]))


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
