"""What the GPU tests of kv_search and of search sessions compare between a
device result row (engine.SEARCH_DTYPE) and the plain-Python restatements
(tests/_mcts_search.py, tests/_mcts_session.py): every field, floats as bits.
Shared by tests/test_mcts_session_gpu.py and tests/test_mcts_search_net_gpu.py;
not a test module itself."""
import numpy as np

from tests import _mcts_session as SS


def bits(a):
    return np.array(a, dtype=np.float32).view(np.uint32).tolist()


def same(row, r, tag):
    """A device row against the restatement's result of the same call."""
    n = len(r["visits"])
    assert (row["status"], row["n_moves"], row["sims"]) == (r["status"], n, r["sims"]), tag
    assert row["visits"][:n].tolist() == r["visits"] and (row["visits"][n:] == -1).all(), tag
    assert row["moves"][:n].tolist() == r["moves"], tag
    assert bits(row["q"][:n]) == bits(r["q"]) and bits(row["prior"][:n]) == bits(r["prior"]), tag
    assert row["pv"][:row["pv_len"]].tolist() == r["pv"], tag
    assert (row["steps"], row["nn_rows"], row["best"]) == (r["steps"], r["nn_rows"], r["best"]), tag
    assert row["root_value"] == r["root_value"], tag
    if n:
        assert row["best_q"] == r["q"][r["best"]], tag


def same_call(ps, ses, rows, ref, tag):
    for i, (row, r) in enumerate(zip(rows, ref)):
        same(row, r, f"{tag} tree {i}")
        assert ps.tree_size(i) == ses.tree_size(i), f"{tag} tree {i}"


def line(ps, states, plan, evaluator=None):
    """search at plan[0], then advance(best) -> resume for every further (sims, leaves) of the plan, every call
    against the restated session. evaluator(n, leaves) -> the restatement's evaluator of a call of n trees at
    `leaves` leaves (the network's batch class is the call's); None: the hash evaluator."""
    ev = (lambda leaves: None) if evaluator is None else (lambda leaves: evaluator(len(states), leaves))
    ses = SS.Session(states)
    rows = ps.search(np.stack(states), *plan[0])
    same_call(ps, ses, rows, ses.search(*plan[0], evaluate=ev(plan[0][1])), "search")
    for ply, (sims, leaves) in enumerate(plan[1:]):
        edges = rows["best"].astype(np.int32)  # -1 at a root that is not searched
        after = ps.advance(edges)
        assert np.array_equal(after, np.stack(ses.advance(edges.tolist()))), ply
        for i in range(len(states)):
            assert ps.tree_size(i) == ses.tree_size(i), (ply, i)
        rows, kept = ps.resume(sims, leaves)
        ref, ref_kept = ses.resume(sims, leaves, evaluate=ev(leaves))
        assert kept.tolist() == ref_kept, ply
        same_call(ps, ses, rows, ref, f"ply {ply}")
    return rows
