"""Descents deeper than a wavefront is wide, on the GPU: kv_search, search sessions and self-play from the two
forced-line positions of tests/_mcts_deep.py, every field against the plain-Python restatements (and the C oracle
at one leaf), floats as bits.

On CHAIN sim k descends k plies, so the 64-strided path loops of search_select_tree / search_backup_tree and of
k_mcts_select / mcts_backup_slot run a second and a third pass per lane, with the mover's sign taken at depths past
64; k_search_result cuts a principal variation of 16 moves out of a line hundreds deep; kv_search_advance packs a
tree in which every kept node is the only child of the one before it; and with reuse_tree a carried root already
holds sims - 1 visits (rem 1), with fast plies more than the ply's target (rem 0). On CHAIN_B the sim-steps hold
two and more deep descents in flight. tests/test_deep_lines_cpu.py asserts all of that from the references alone.
Each test prints its engine time."""
import functools
import time

import numpy as np
import pytest
import torch

from knightvision_amd.engine import EVAL_HASH, PositionSearch, SelfPlayEngine, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_deep as D
from tests import _mcts_search as S
from tests import _mcts_session as SS
from tests import _mcts_starts as ST
from tests._mcts_compare import same, same_call

pytestmark = pytest.mark.gpu

NAMES = ("CHAIN", "CHAIN_B")
CALL_SIMS = D.SIMS["CHAIN_B"]  # kv_search has one visit count per call: both positions at CHAIN_B's 400
STATES = [D.POSITIONS[n] for n in NAMES]


@pytest.fixture(scope="module")
def hash_search():
    with PositionSearch(synthetic_state_dict(42, "init"), max_positions=2, max_sims=CALL_SIMS,
                        eval_mode=EVAL_HASH) as ps:
        yield ps


# ---- 1. position search
@pytest.mark.parametrize("leaves", [1, 4, 8])
def test_hash_search_of_both_lines_in_one_call(hash_search, leaves):
    t0 = time.perf_counter()
    rows = hash_search.search(np.stack(STATES), CALL_SIMS, leaves=leaves)
    print(f"kv_search, 2 positions x {CALL_SIMS} sims at {leaves} leaves: {time.perf_counter() - t0:.2f} s")
    for name, row in zip(NAMES, rows):
        r = D.search_ref(name, leaves, CALL_SIMS)
        same(row, r, f"{name} L {leaves}")
        assert D.deepest(r) >= 130
    assert rows["pv_len"][0] == 16 and rows["visits"][0][0] == CALL_SIMS  # the cut of a line 400 deep
    if leaves > 1:
        assert D.steps_with_two_deep(D.search_ref("CHAIN_B", leaves, CALL_SIMS)) >= 10
    # CHAIN alone at its own 160 visits
    row = hash_search.search(D.CHAIN[None], D.SIMS["CHAIN"], leaves=leaves)[0]
    same(row, D.search_ref("CHAIN", leaves), f"CHAIN alone L {leaves}")
    assert row["pv_len"] == 16


def _hip_eval(net):
    """The restatements' evaluator: the HIP network's rows of a list of positions, one forward in the <= 16-board
    class (2 trees at 4 leaves are 8 rows)."""
    def ev(states):
        codes = np.stack([np.asarray(st[:64], dtype=np.int8) for st in states])
        assert len(codes) <= 16
        pol, val = net.forward_boards(torch.from_numpy(np.ascontiguousarray(codes)).cuda())
        torch.cuda.synchronize()
        pol, val = pol.cpu().numpy(), val.cpu().numpy().reshape(-1)
        return [(pol[j], val[j]) for j in range(len(codes))]

    return ev


def test_network_search_of_both_lines_at_4_leaves():
    """The real network's rows: priors and values differ from node to node down the lines (under the hash
    evaluator every prior is 1/n)."""
    from knightvision_amd.model import KVNet
    sd = synthetic_state_dict(42, "init")
    net = KVNet(0, packed_from(sd))
    try:
        with PositionSearch(sd, max_positions=2, max_sims=CALL_SIMS) as ps:
            t0 = time.perf_counter()
            rows = ps.search(np.stack(STATES), CALL_SIMS, leaves=4)
            print(f"kv_search on the network, 2 positions x {CALL_SIMS} sims at 4 leaves: "
                  f"{time.perf_counter() - t0:.2f} s")
        ev = _hip_eval(net)
        deep = []
        for name, row in zip(NAMES, rows):
            r = S.search(D.POSITIONS[name], CALL_SIMS, 4, ncap=CALL_SIMS + 2, evaluate=ev, depths=True)
            same(row, r, f"network {name}")
            deep.append(D.deepest(r))
        print(f"deepest descents on the network: {deep}")
        assert deep[0] == CALL_SIMS and rows["pv_len"][0] == 16  # (CHAIN_B's depth depends on the weights)
    finally:
        net.close()


# ---- 2. sessions: down the line three times
@pytest.mark.parametrize("leaves", [1, 4])
def test_session_down_the_lines(hash_search, leaves):
    ps = hash_search
    ses = SS.Session(STATES, ncap=CALL_SIMS + 2)
    t0 = time.perf_counter()
    rows = ps.search(np.stack(STATES), CALL_SIMS, leaves=leaves)
    ref = ses.search(CALL_SIMS, leaves)
    same_call(ps, ses, rows, ref, "search")
    gpu = time.perf_counter() - t0
    for ply in range(3):
        edges = [r["best"] for r in ref]
        played_n = [r["visits"][r["best"]] for r in ref]
        t0 = time.perf_counter()
        after = ps.advance(edges)
        sizes = [ps.tree_size(i) for i in range(2)]
        rows, kept = ps.resume(CALL_SIMS, leaves)
        gpu += time.perf_counter() - t0
        assert np.array_equal(after, np.stack(ses.advance(edges))), ply
        assert sizes == [ses.tree_size(i) for i in range(2)], ply
        # the pack of a chain: every node but the old root is kept, each the only child of the one before it
        assert sizes[0] == (CALL_SIMS, 16 * CALL_SIMS), ply
        ref, ref_kept = ses.resume(CALL_SIMS, leaves)
        assert kept.tolist() == ref_kept == [n - 1 for n in played_n], ply
        assert kept[0] == CALL_SIMS - 1 and rows["steps"][0] == 1, ply  # CHAIN: one visit short, one step
        same_call(ps, ses, rows, ref, f"ply {ply}")
        assert rows["pv_len"][0] == 16
    print(f"session at {leaves} leaves, search + 3 x (advance, continue): {gpu:.2f} s with the restatement between")


LONG_PLIES = 70


@pytest.mark.parametrize("leaves", [1, 4])
def test_session_70_plies_down_the_chain(hash_search, leaves):
    """What a backup writes into W at depth d shows in an output only once the edge is a root edge: on a forced
    line no choice depends on it. So CHAIN is searched to 160 visits and advanced 70 times, each time topped up
    by the one missing visit: after k advances the root edge's q is built from the W updates it took at depths
    k, k - 1, ..., 0 -- from k = 64 on, from the second pass of the backup's path loop and its sign."""
    ps, sims = hash_search, D.SIMS["CHAIN"]
    ses = SS.Session([D.CHAIN], ncap=CALL_SIMS + 2)
    t0 = time.perf_counter()
    rows = ps.search(D.CHAIN[None], sims, leaves=leaves)
    gpu = time.perf_counter() - t0
    same_call(ps, ses, rows, ses.search(sims, leaves), "search")
    for ply in range(LONG_PLIES):
        t0 = time.perf_counter()
        after = ps.advance([0])
        rows, kept = ps.resume(sims, leaves)
        gpu += time.perf_counter() - t0
        assert np.array_equal(after, np.stack(ses.advance([0]))), ply
        ref, ref_kept = ses.resume(sims, leaves)
        assert kept.tolist() == ref_kept == [sims - 1], ply
        same_call(ps, ses, rows, ref, f"ply {ply}")  # q as bits
        assert rows["pv_len"][0] == 16 and rows["steps"][0] == 1 and ref[0]["q"][0] != 0, ply
    print(f"session of {LONG_PLIES} advances at {leaves} leaves: {gpu:.2f} s on the GPU")


# ---- 3. self-play from the lines
def _norm(p, n_evals):
    """A restated game (tests/_mcts_endings.Played) as tests/_mcts_starts._row gives one."""
    return ST._row([x["move"] for x in p], [x["visits"] for x in p], [e["board"] for e in p.extra], p.result,
                   n_evals, words=[x["words"] for x in p])


@functools.lru_cache(maxsize=None)
def _run(name, n, **kw):
    sd = synthetic_state_dict(42, "init")
    arena = kw.pop("arena", False)
    t0 = time.perf_counter()
    with SelfPlayEngine(sd, opponent=sd if arena else None, slots=n, n_games=n, seed=D.SEED, max_moves=D.MAX_MOVES,
                        sims=D.SIMS[name], c_puct=D.C_PUCT, eps=D.EPS, alpha=D.ALPHA, keep_root_moves=True,
                        eval_mode=EVAL_HASH, **kw) as eng:
        eng._set_starts(np.stack(D.starts_of(name)))
        t1 = time.perf_counter()
        eng.run()
        out = eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()
    print(f"self-play from {name}, {n} games x {D.MAX_MOVES} plies x {D.SIMS[name]} sims, {kw or 'one leaf'}"
          f"{', arena' if arena else ''}: create {t1 - t0:.2f} s, run {time.perf_counter() - t1:.2f} s")
    return out


def _same_games(run, ref):
    recs, visits, words, games, st = run
    row = {int(g["game_id"]): g for g in games}
    assert sorted(row) == list(range(len(ref)))
    for gid, r in enumerate(ref):
        g = row[gid]
        got = (int(g["plies"]), int(g["outcome"]), float(g["reward"]), int(g["reason"]), int(g["n_evals"]))
        assert got == (r["plies"], r["outcome"], r["reward"], r["reason"], r["n_evals"]), gid
        sel = recs["game_id"] == gid
        assert recs["ply"][sel].tolist() == list(range(r["plies"])) and r["plies"] == D.MAX_MOVES, gid
        assert recs["move"][sel].tolist() == r["moves"], gid
        assert [bytes(b) for b in recs["board"][sel]] == r["boards"], gid
        for p in range(r["plies"]):
            n = len(r["visits"][p])
            assert visits[sel][p][:n].tolist() == r["visits"][p] and (visits[sel][p][n:] == -1).all(), (gid, p)
            assert words[sel][p][:n].tolist() == r["words"][p] and (words[sel][p][n:] == 0xffff).all(), (gid, p)
    plies = sum(r["plies"] for r in ref)
    assert len(recs) == plies == st["plies"] and st["games_done"] == len(ref) and st["tree_overflows"] == 0
    assert st["nn_rows"] == sum(r["n_evals"] for r in ref)


@pytest.mark.parametrize("name", NAMES)
def test_one_leaf_games_are_the_oracles(name):
    n = D.n_games(name)
    ref = []
    for g, r in enumerate(D.oracle_games(name)):
        boards, words = ST._boards(D.starts_of(name)[g % 2], r["moves"])
        k = [int((v >= 0).sum()) for v in r["visits"]]
        ref.append(ST._row(r["moves"], [v[:m] for v, m in zip(r["visits"], k)], boards,
                           (r["plies"], r["outcome"], r["reason"], r["reward"]), r["n_evals"], words=words))
    run = _run(name, n)
    _same_games(run, ref)
    st = run[4]
    assert st["sims"] == n * D.MAX_MOVES * D.SIMS[name] and st["sims_kept"] == st["roots_carried"] == 0
    assert st["plies_fast"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_carried_trees_one_visit_short(name):
    n = D.n_games(name)
    games = D.reuse_games(name)
    ref = [_norm(p, len(p) + sum(sum(x["pending"]) for x in p)) for p in games]
    run = _run(name, n, reuse_tree=True)
    _same_games(run, ref)
    st = run[4]
    assert st["sims_kept"] == sum(x["kept"] for p in games for x in p)
    assert st["sims"] == sum(x["rem"] for p in games for x in p)
    assert st["roots_carried"] == sum(x["carried"] for p in games for x in p) == n * (D.MAX_MOVES - 1)
    assert st["sims"] + st["sims_kept"] == n * D.MAX_MOVES * D.SIMS[name]
    if name == "CHAIN":
        assert st["sims_kept"] == n * (D.MAX_MOVES - 1) * 159 and st["sims"] == n * (160 + D.MAX_MOVES - 1)


@pytest.mark.parametrize("name", NAMES)
def test_carried_trees_with_fast_plies(name):
    """reuse_tree with fast_sims: a fast ply whose carried root holds more than its target runs no sim-step."""
    n = D.n_games(name)
    games = D.pcr_reuse_games(name)
    ref = [_norm(p, len(p) + sum(sum(x["pending"]) for x in p)) for p in games]
    run = _run(name, n, reuse_tree=True, fast_sims=D.FAST_SIMS, full_prob=D.Q16 / 65536.0)
    _same_games(run, ref)
    st, plies = run[4], [x for p in games for x in p]
    assert sum(x["rem"] == 0 for x in plies) >= 2
    assert st["plies_fast"] == sum(not x["full"] for x in plies) and st["plies_full"] == sum(x["full"] for x in plies)
    assert st["sims"] == sum(x["rem"] for x in plies) and st["sims_kept"] == sum(x["kept"] for x in plies)
    assert st["roots_carried"] == sum(x["carried"] for x in plies)
    for gid, p in enumerate(games):
        sel = run[0]["game_id"] == gid
        assert run[0]["pad"][sel].tolist() == [0 if x["full"] else 1 for x in p], gid
        assert [int(v[v >= 0].sum()) for v in run[1][sel]] == [max(x["target"], x["kept"]) for x in p], gid


@pytest.mark.parametrize("name", NAMES)
def test_four_leaves_in_flight(name):
    n = D.n_games(name, True)
    games = D.leaves_games(name, 4)
    ref = [_norm(p, len(p) + sum(sum(map(sum, x["leaf_pending"])) for x in p)) for p in games]
    run = _run(name, n, leaves=4)
    _same_games(run, ref)
    st = run[4]
    assert st["sims"] == n * D.MAX_MOVES * D.SIMS[name] and st["sims_kept"] == st["roots_carried"] == 0
    assert st["leaf_rows_pending"] == st["nn_rows"] - st["plies"]
    # the games step together: a ply's sim loop runs until the slowest game of the ply is done
    assert st["sim_steps"] == sum(max(len(p[ply]["accepted"]) for p in games) for ply in range(D.MAX_MOVES))
    if name == "CHAIN":
        assert st["sim_steps"] == D.MAX_MOVES * 160  # one accepted descent per step in both games


@pytest.mark.parametrize("name", NAMES)
def test_arena_games(name):
    n = D.n_games(name, True)
    games = D.arena_games(name)
    ref = [_norm(p, len(p) + sum(e["pending"] for e in p.extra)) for p in games]
    run = _run(name, n, arena=True)
    _same_games(run, ref)
    st = run[4]
    assert st["sims"] == n * D.MAX_MOVES * D.SIMS[name]
    assert st["arena_rows"][0] > 0 and st["arena_rows"][1] > 0
    assert [x["player"] for x in games[0]] == [0, 1] * (D.MAX_MOVES // 2)


# ---- 4. the evaluation cache on a line that repeats
def test_eval_cache_on_the_repeating_line():
    n = D.n_games("CHAIN")
    off = _run("CHAIN", n, leaves=D.CACHE_LEAVES)
    on = _run("CHAIN", n, leaves=D.CACHE_LEAVES, eval_cache=D.CACHE_ENTRIES)
    for k in range(3):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert np.array_equal(np.sort(on[3], order="game_id"), np.sort(off[3], order="game_id"))
    for key in ("plies", "sims", "nn_rows", "leaf_rows_pending", "sim_steps", "games_done"):
        assert on[4][key] == off[4][key], key
    games, info, table = D.cached_games()
    ref = [_norm(p, len(p) + sum(sum(map(sum, x["leaf_pending"])) for x in p)) for p in games]
    _same_games(on, ref)
    print(f"eval_cache {D.CACHE_ENTRIES}: probes / hits / stores {on[4]['cache_probes']} / {on[4]['cache_hits']} / "
          f"{on[4]['cache_stores']} (restated {table.probes} / {table.hits} / {table.stores})")
    assert (on[4]["cache_probes"], on[4]["cache_hits"], on[4]["cache_stores"]) == \
        (table.probes, table.hits, table.stores)
    assert (off[4]["cache_probes"], off[4]["cache_hits"], off[4]["cache_stores"]) == (0, 0, 0)
    assert on[4]["sim_steps"] == info["steps"] and table.hits > table.probes // 2
