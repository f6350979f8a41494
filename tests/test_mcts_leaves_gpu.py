"""Self-play and arena with several leaves in flight per game (kv_config.leaves; k_leaves_* in kv_search.hip,
k_leaves_compact and eng_leaves_ply in kv_engine.hip) through the C ABI, against the plain-Python restatement
(tests/_mcts_selfplay_leaves.py). Every comparison is exact:

* leaves 0 and 1 are the same engine byte for byte.
* Hash evaluator: every PUCT score is bit-reproducible on both sides, so visits, move words and moves must be
  identical, and the sim-steps, pending rows and padded batch rows the engine counts are the restatement's.
* Real ChessNet: the restatement is fed the HIP network's own rows in the run's batch class.
* Arena: A against A is the self-play run byte for byte; hash A against B equals the restatement per player.

The engine runs and the restated games are computed once per configuration and shared by the tests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import EVAL_HASH, EVAL_LAZY, SelfPlayEngine, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_selfplay_leaves as SL

pytestmark = pytest.mark.gpu

SEED = SL.SEED
CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class


@functools.lru_cache(maxsize=None)
def _run(a, b, slots, n_games, sims, steps, leaves, max_moves=None, hash_eval=False, base=0, sample_plies=0):
    """One engine run (b None: self-play of a) -> (records, root visits, root move words, games, stats)."""
    opp = None if b is None else synthetic_state_dict(42, b)
    with SelfPlayEngine(synthetic_state_dict(42, a), opponent=opp, slots=slots, n_games=n_games, seed=SEED,
                        max_moves=max_moves, sims=sims, c_puct=1.5, keep_root_moves=True, leaves=leaves,
                        sample_plies=sample_plies, game_id_base=base, eval_mode=EVAL_HASH if hash_eval else 0) as eng:
        eng.run(steps)
        return eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()


def _hash_many(states):
    return [SL.hash_eval(st) for st in states]


def _hash_many_b(states):
    return [SL.hash_eval_b(st) for st in states]


_NETS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_nets():
    yield
    while _NETS:
        _NETS.popitem()[1].close()


def _hip_eval_many(variant):
    """The HIP network's rows of a list of positions as one batch of the > 16-board class (fewer than 17 positions
    are padded with copies of the first, as the engine pads a short batch)."""
    from knightvision_amd.model import KVNet
    if variant not in _NETS:
        _NETS[variant] = KVNet(0, packed_from(synthetic_state_dict(42, variant)))
    net = _NETS[variant]

    def ev(states):
        codes = np.stack([np.asarray(st[:64], dtype=np.int8) for st in states])
        n = len(codes)
        if n < CLASS_ROWS:
            codes = np.concatenate([codes, np.repeat(codes[:1], CLASS_ROWS - n, axis=0)])
        pol, val = net.forward_boards(torch.from_numpy(np.ascontiguousarray(codes)).cuda())
        torch.cuda.synchronize()
        pol, val = pol.cpu().numpy(), val.cpu().numpy().reshape(-1)
        return [(pol[k], val[k]) for k in range(n)]

    return ev


def _plies_of(run, games):
    return tuple(int((run[0]["game_id"] == g).sum()) for g in games)


def _padded(n, big):
    return CLASS_ROWS if big and 0 < n < CLASS_ROWS else n


def _divergences(run, restated, sims):
    """Plies at which a game's record, root visit vector or root move words differ from the restatement's."""
    recs, visits, words = run[0], run[1], run[2]
    bad = []
    for g, plies in restated.items():
        sel = recs["game_id"] == g
        assert (np.diff(recs["ply"][sel]) == 1).all() and sel.sum() == len(plies)
        for p, ply in enumerate(plies):
            n = len(ply["visits"])
            ok = (recs["move"][sel][p] == ply["move"] and np.array_equal(visits[sel][p][:n], ply["visits"])
                  and (visits[sel][p][n:] == -1).all() and np.array_equal(words[sel][p][:n], ply["words"])
                  and (words[sel][p][n:] == 0xffff).all() and visits[sel][p][:n].sum() == sims)
            if not ok:
                bad.append((g, p))
                print(f"game {g} ply {p}: GPU visits {visits[sel][p][:n]} move {recs['move'][sel][p]}, restated "
                      f"{ply['visits']} move {ply['move']} (accepted per step {ply['accepted']})")
                break  # the games part here
    return bad


def _check_counts(st, info, plies, sims, slots, leaves, arena):
    """The engine's counters against the restatement's batch: steps, pending rows, padded rows, identities."""
    big = slots * leaves > 16
    rows = [sum(_padded(b[x], big) for b in info["batches"]) for x in (0, 1)]
    print(f"sim_steps {st['sim_steps']} (restated {info['steps']}), leaf_rows_pending {st['leaf_rows_pending']} "
          f"(restated {info['pending']}), leaf_batch_rows {st['leaf_batch_rows']} (restated {rows}), arena_rows "
          f"{st['arena_rows']}")
    assert st["sim_steps"] == info["steps"]
    assert st["leaf_rows_pending"] == sum(info["pending"])
    assert st["leaf_batch_rows"] == sum(rows)
    assert st["arena_rows"] == (tuple(rows) if arena else (0, 0))
    assert st["plies"] == sum(plies) and st["sims"] == sum(plies) * sims
    assert st["nn_rows"] == sum(plies) + sum(info["pending"])  # the root rows + the pending leaves
    assert st["tree_overflows"] == 0


# ---- 5. leaves 0 against 1
def test_leaves_0_and_1_are_the_same_engine():
    zero = _run("init", None, 18, 22, 16, -1, 0, max_moves=4, hash_eval=True)
    one = _run("init", None, 18, 22, 16, -1, 1, max_moves=4, hash_eval=True)
    assert len(zero[3]) == 22 and len(zero[0]) == 88
    for k, name in enumerate(("records", "root visits", "root moves", "game table")):
        assert zero[k].tobytes() == one[k].tobytes(), name
    for key in ("steps", "plies", "games_done", "nn_rows", "sims", "records", "tree_overflows", "arena_rows",
                "sim_steps", "leaf_rows_pending", "sims_kept", "roots_carried", "leaf_batch_rows"):
        assert zero[4][key] == one[4][key], key
    st = zero[4]
    assert st["sim_steps"] == st["steps"] * 16 == 8 * 16
    assert st["nn_rows"] == st["plies"] + st["leaf_rows_pending"] and 0 < st["leaf_rows_pending"] <= 88 * 16


# ---- 6. hash evaluator against the restatement
@pytest.mark.parametrize("name", sorted(SL.HASH_RUNS))
def test_hash_games_identical_to_restatement(name):
    cfg = SL.HASH_RUNS[name]
    slots, n_games, base, sims, leaves = cfg["slots"], cfg["n_games"], cfg["base"], cfg["sims"], cfg["leaves"]
    run = _run("init", None, slots, n_games, sims, -1, leaves, max_moves=cfg["max_moves"], hash_eval=True,
               base=base)
    games = tuple(range(base, base + n_games))
    plies = _plies_of(run, games)
    print(f"{name}: game lengths {plies}, reasons {run[3]['reason'].tolist()}")
    assert plies == cfg["plies"], "the CPU test's tuples are these games"
    assert (run[3]["reason"] == 0).all()  # max_moves: every game holds its slot for its plies (starts_of)
    rest, info = SL.play_many([SEED + g for g in games], games, sims, plies, leaves, _hash_many,
                              starts=SL.starts_of(plies, slots))
    assert _divergences(run, dict(zip(games, rest)), sims) == []
    _check_counts(run[4], info, plies, sims, slots, leaves, False)
    if n_games > slots:  # the tail: steps whose batch holds fewer games than slots
        assert run[4]["games_done"] == n_games and len(set(SL.starts_of(plies, slots))) > 1


# ---- 7. the real network
@pytest.mark.parametrize("variant,slots", [("init", 6), ("stress", 6), ("init", 5)])
def test_network_games_identical_to_restatement(variant, slots):
    sims, leaves, steps = 20, 4, 3
    run = _run(variant, None, slots, slots, sims, steps, leaves)
    games = tuple(range(slots))
    plies = _plies_of(run, games)
    assert plies == (steps,) * slots
    ev = _hip_eval_many(variant)
    rest, info = SL.play_many([SEED + g for g in games], games, sims, plies, leaves, ev)
    bad = _divergences(run, dict(zip(games, rest)), sims)
    print(f"leaves network parity ({variant}, {slots} slots): {sum(len(g) for g in rest)} root vectors compared, "
          f"divergences {len(bad)}")
    assert bad == []
    _check_counts(run[4], info, plies, sims, slots, leaves, False)


# ---- 8. arena
def test_arena_same_weights_is_selfplay_byte_for_byte():
    arena = _run("init", "init", 18, 22, 16, -1, 4, max_moves=4)
    solo = _run("init", None, 18, 22, 16, -1, 4, max_moves=4)
    one = _run("init", None, 18, 22, 16, -1, 1, max_moves=4)
    assert len(solo[3]) == 22 and len(solo[0]) == 88
    for k, name in enumerate(("records", "root visits", "root moves", "game table")):
        assert arena[k].tobytes() == solo[k].tobytes(), name
    for key in ("plies", "sims", "nn_rows", "records", "games_done", "sim_steps", "leaf_rows_pending"):
        assert arena[4][key] == solo[4][key], key
    st = arena[4]
    assert st["arena_rows"][0] + st["arena_rows"][1] == st["leaf_batch_rows"] and min(st["arena_rows"]) > 0
    assert solo[4]["sim_steps"] < one[4]["sim_steps"]  # fewer, larger steps
    assert solo[1].tobytes() != one[1].tobytes()  # another search than one leaf's


def test_arena_hash_identical_to_restatement():
    slots, n_games, sims, leaves, mm = 18, 22, 22, 4, 6
    run = _run("init", "init", slots, n_games, sims, -1, leaves, max_moves=mm, hash_eval=True, sample_plies=2)
    games = tuple(range(n_games))
    plies = _plies_of(run, games)
    assert plies == (mm,) * n_games
    rest, info = SL.play_many([SEED + g for g in games], games, sims, plies, leaves, _hash_many, _hash_many_b,
                              starts=SL.starts_of(plies, slots), arena=True, sample_plies=2)
    assert _divergences(run, dict(zip(games, rest)), sims) == []
    assert min(info["pending"]) > 0
    _check_counts(run[4], info, plies, sims, slots, leaves, True)
    st = run[4]
    assert st["arena_rows"][0] + st["arena_rows"][1] == st["leaf_batch_rows"]
    # B's negated value matters: the games are not the self-play games of the hash evaluator
    solo = _run("init", None, slots, n_games, sims, -1, leaves, max_moves=mm, hash_eval=True, sample_plies=2)
    assert solo[0].tobytes() != run[0].tobytes()


# ---- 9. refusals
def _cfg(**kw):
    base = dict(device=0, slots=4, n_games=4, game_id_base=0, game_id_stride=1, seed=SEED, seed_mode=0, max_moves=0,
                batch=16, eps=0.25, alpha=0.3, sims=8, c_puct=1.5, eval_mode=EVAL_HASH, record_cap=1 << 10,
                recycle=1, precision=0, algo=0, tree_edge_cap=0, keep_root_visits=0)
    base.update(kw)
    return _lib.Config(**base)


@pytest.mark.parametrize("kw,text", [
    (dict(leaves=-1), "leaves -1 out of range"),
    (dict(leaves=65), "leaves 65 out of range"),
    (dict(leaves=2, sims=0), "leaves 2 with sims 0"),
    (dict(leaves=2, reuse_tree=1), "leaves 2 with reuse_tree 1"),
    (dict(leaves=2, sims=0, eval_mode=EVAL_LAZY), "leaves 2 with eval_mode KV_EVAL_LAZY"),
    (dict(leaves=2, sims=8, eval_mode=EVAL_LAZY), "leaves 2 with eval_mode KV_EVAL_LAZY"),
    (dict(leaves=2, slots=64, n_games=64, sim_groups=2), "leaves 2 with sim_groups 2"),
    (dict(leaves=2, arena=1, slots=64, n_games=64, sim_groups=2), "leaves 2 with sim_groups 2"),
])
def test_create_refusals(kw, text):
    h = C.c_void_p()
    rc = _lib.lib().kv_create(C.byref(_cfg(**kw)), C.byref(h))
    assert rc == -1, rc  # KV_EINVAL
    msg = _lib.lib().kv_last_error().decode()
    assert text in msg, msg
    assert not h.value


# ---- 10. a shrunk pool
def test_tree_overflow_is_an_error():
    """An edge pool smaller than the search needs fails kv_run loudly at 4 leaves as it does at 1."""
    cap = _lib.MAXM + 40
    with SelfPlayEngine(synthetic_state_dict(42, "init"), slots=4, n_games=4, seed=42, max_moves=4, sims=64,
                        eval_mode=EVAL_HASH, tree_edge_cap=cap, leaves=4) as eng:
        with pytest.raises(_lib.KVError, match="tree pool full"):
            eng.run()
        assert eng.stats()["tree_overflows"] > 0


# ---- the Python surface
def test_play_match_and_the_loop_take_leaves():
    from knightvision_amd import arena
    from knightvision_amd.learn import reinforcement_loop
    from knightvision_amd.model import ChessNet
    a, b = synthetic_state_dict(42, "init"), synthetic_state_dict(42, "peaked")
    r = arena.play_match(a, b, 18, sims=8, slots=18, seed=SEED, max_moves=6, sample_plies=2, leaves=4)
    one = arena.play_match(a, b, 18, sims=8, slots=18, seed=SEED, max_moves=6, sample_plies=2)
    assert r["games"] == 18 == r["wins"] + r["draws"] + r["losses"] and r["reasons"] == {"max_moves": 18}
    assert 6 * 2 <= r["stats"]["sim_steps"] < one["stats"]["sim_steps"] == 6 * 8
    assert r["stats"]["sims"] == one["stats"]["sims"] == 18 * 6 * 8
    torch.manual_seed(0)
    m = ChessNet()
    stats = reinforcement_loop(m, iterations=1, games_per_iter=8, device="cuda:0", epochs=1, batch_size=64,
                               max_moves=6, slots=8, log=None, sims=8, leaves=4, arena_games=6, arena_leaves=2)
    assert stats[0]["arena"]["games"] == 6 and 0 < stats[0]["sim_steps"] < 6 * 8
