"""What tests/test_mcts_wide_cpu.py and tests/test_mcts_wide_gpu.py share: the wide roots of
tests/_mcts_search.py, the visit counts of their searches, and the choice of the edges a session advances
along, taken from the restated trees (tests/_mcts_session.py). Not a test module itself."""
import functools

from oracle import oracle as O

from tests import _mcts_search as S
from tests import _mcts_session as SS

WIDE = [S.WIDE_A, S.WIDE_B, S.WIDE_C]
N_MOVES = [len(O.valid_moves(st)[0]) for st in WIDE]
SIMS = 3 * max(N_MOVES)        # the hash searches: every root edge of the widest can be visited
NET_SIMS = 2 * max(N_MOVES)    # the searches on the real network
MAX_SIMS = 700                 # the engines' capacity
# Sessions: fewer visits than the widest root has moves, so that it keeps unvisited edges to drop along
SESSION_STATES = [S.WIDE_A, S.WIDE_B, S.WIDE_C, S.WIDE_C]
SESSION_SIMS = 180
assert SIMS <= MAX_SIMS and SESSION_SIMS < N_MOVES[2]


@functools.lru_cache(maxsize=None)
def hash_ref(i, sims, leaves, eps=0.0, alpha=0.3, seed=0):
    """The restated hash search of WIDE[i], computed once per case."""
    return S.search(WIDE[i], sims, leaves, ncap=MAX_SIMS + 2, eps=eps, alpha=alpha, seed=seed)


def child_edges(root, k):
    ch = root.child[k]
    return 0 if ch is None else len(ch.words)


def session_edges(ses):
    """The four kinds of advance over SESSION_STATES after the first search, from the restated trees:
    tree 0 an edge whose child has more than 64 edges (the most visited such), tree 1 a visited edge at index
    64 or above (the most visited such), tree 2 the best edge, tree 3 the first unvisited edge."""
    roots = [t.root for t in ses.trees]
    wide = [k for k in range(len(roots[0].words)) if child_edges(roots[0], k) > 64]
    high = [k for k in range(64, len(roots[1].words)) if roots[1].N[k] > 0]
    unvisited = [k for k in range(len(roots[3].words)) if roots[3].N[k] == 0]
    assert wide and high and unvisited
    return [max(wide, key=lambda k: roots[0].N[k]), max(high, key=lambda k: roots[1].N[k]),
            roots[2].N.index(max(roots[2].N)), unvisited[0]]


def last_expanded_edge(root):
    """The root edge whose child was expanded last: on the device the child with the largest node id."""
    made = [k for k in range(len(root.words)) if root.child[k] is not None]
    return max(made, key=lambda k: root.child[k].serial)
