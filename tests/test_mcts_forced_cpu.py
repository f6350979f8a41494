"""Forced playouts and policy target pruning (kv_config.forced_k, DESIGN.md "Forced playouts and policy target
pruning"), the parts that need no GPU: the config validation and the ctypes mirrors, the plain-Python restatement
(tests/_mcts_selfplay_forced.py) pinned with forced_k = 0 to the restatements it is built from, the rule and the
pruning on hand-computed roots, and what the seeds of tests/test_mcts_forced_gpu.py must hold for its comparisons
to exercise the rule."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _mcts_selfplay_forced as FP
from tests import _mcts_selfplay_pcr as P

F = np.float32
SEED, K, Q16, GAMES = FP.SEED, FP.K, FP.Q16, FP.GAMES


def _cfg(**kw):
    from knightvision_amd import _lib
    base = dict(device=0, slots=4, n_games=4, game_id_base=0, game_id_stride=1, seed=42, seed_mode=0, max_moves=0,
                batch=16, eps=0.25, alpha=0.3, sims=16, c_puct=1.5, eval_mode=0, record_cap=0, recycle=1,
                precision=0, algo=0, tree_edge_cap=0, keep_root_visits=0)
    base.update(kw)
    return _lib.Config(**base)


@pytest.mark.parametrize("kw, msg", [
    (dict(forced_k=-1.0), "forced_k -1 out of range"),
    (dict(forced_k=-0.001), "out of range: 0 (off) or 0 < forced_k <= 16"),
    (dict(forced_k=16.5), "forced_k 16.5 out of range"),
    (dict(forced_k=float("inf")), "out of range: 0 (off) or 0 < forced_k <= 16"),
    (dict(forced_k=float("-inf")), "out of range: 0 (off) or 0 < forced_k <= 16"),
    (dict(forced_k=float("nan")), "out of range: 0 (off) or 0 < forced_k <= 16"),
    (dict(forced_k=2.0, sims=0), "forced_k 2 with sims 0"),
    (dict(forced_k=2.0, arena=1), "forced_k 2 with arena 1"),
])
def test_kv_create_rejects_bad_forced_configs(kw, msg):
    """Validated before the device is touched: KV_EINVAL, the reason in kv_last_error(), a NULL handle."""
    from knightvision_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _cfg(**kw)
    assert L.kv_create(C.byref(cfg), C.byref(h)) == -1  # KV_EINVAL
    err = L.kv_last_error().decode()
    assert msg in err and "forced_k" in err
    assert not h.value


def test_config_and_stats_mirrors():
    from knightvision_amd import _lib
    L = _lib.lib()
    assert L.kv_sizeof_config() == C.sizeof(_lib.Config)
    assert L.kv_sizeof_stats() == C.sizeof(_lib.Stats)
    names = [n for n, _ in _lib.Config._fields_]
    k = names.index("forced_k")
    assert names[k - 1:k + 2] == ["tree_edge_cap", "forced_k", "keep_root_visits"]
    assert dict(_lib.Config._fields_)["forced_k"] is C.c_float
    assert _lib.Config.forced_k.offset == _lib.Config.tree_edge_cap.offset + 4
    assert _lib.Config.keep_root_visits.offset == _lib.Config.forced_k.offset + 4
    stats = [n for n, _ in _lib.Stats._fields_]
    a = stats.index("plies_full")
    assert stats[a - 3:a + 1] == ["dom_kernel", "forced_descents", "visits_pruned", "plies_full"]
    assert dict(_lib.Stats._fields_)["forced_descents"] is C.c_int64
    assert dict(_lib.Stats._fields_)["visits_pruned"] is C.c_int64
    assert _lib.Config().forced_k == 0.0  # a zeroed config: the feature is off
    for name in ("kv_root_targets", "kv_root_targets_device"):
        assert name in _lib.EXPORTED and hasattr(L, name)


def test_engine_options_default_to_off():
    import inspect

    from knightvision_amd import learn
    from knightvision_amd.engine import SelfPlayEngine
    for fn in (SelfPlayEngine.__init__, learn.selfplay_shard, learn.reinforcement_loop):
        assert inspect.signature(fn).parameters["forced_k"].default == 0.0
    assert callable(SelfPlayEngine.root_targets) and callable(SelfPlayEngine.root_targets_device)


def _strip(plies):
    return [{k: v for k, v in d.items() if k not in FP.ADDED} for d in plies]


# ---- off equals today
@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("fast, q16", [(0, 0), (4, Q16)])
def test_forced_off_is_the_pcr_restatement(reuse, fast, q16):
    """3 seeds x 6 plies x 16 sims on the hash evaluator with forced_k = 0: ply for ply
    tests/_mcts_selfplay_pcr.play, which tests/test_mcts_pcr_cpu.py chains to the C oracle."""
    for seed in (49, 50, 51):
        a, b = FP.play(seed, 16, 6, reuse, fast, q16, 0.0), P.play(seed, 16, 6, reuse, fast, q16)
        assert len(a) == len(b) == 6
        assert _strip(a) == list(b)
        assert a.extra == b.extra
        for d in a:
            assert d["targets"] == d["visits"] and d["pick"] == d["raw_pick"]
            assert d["forced"] == 0 and d["pruned"] == 0


@pytest.mark.parametrize("fast, q16", [(0, 0), (4, Q16)])
def test_forced_off_is_the_pcr_leaves_restatement(fast, q16):
    for seed in (49, 50, 51):
        a, b = FP.play_leaves(seed, 16, 6, 4, fast, q16, 0.0), P.play_leaves(seed, 16, 6, 4, fast, q16)
        assert len(a) == len(b) == 6
        assert _strip(a) == list(b)
        assert a.extra == b.extra
        for d in a:
            assert d["targets"] == d["visits"] and d["pick"] == d["raw_pick"] and d["forced"] == d["pruned"] == 0


# ---- the rule and the pruning on hand-computed roots (c_puct 1.5, k 2; every figure below is exact or far from
# its comparison: the priors, value sums and square roots are dyadic where a margin is small)
def test_forced_mask_golden():
    # S = 16: thresholds k * P * S = 16, 8, 4, 4, 16; n * n = 9, 4, 1, 0, 16 -- an unvisited edge is never forced,
    # and equality is not below
    got = FP.forced_mask(2.0, [0.5, 0.25, 0.125, 0.125, 0.5], [3, 2, 1, 0, 4], 16)
    assert got.tolist() == [True, True, True, False, False]
    # the threshold moves with S: n = 3 at P = 0.25 is forced from S = 19 on (k * P * S = 9.5 > 9)
    assert [bool(FP.forced_mask(2.0, [0.25], [3], s)[0]) for s in (16, 18, 19)] == [False, False, True]
    assert not FP.forced_mask(2.0, [0.25, 0.5], [0, 0], 0).any()  # the first descent of a fresh root


@pytest.mark.parametrize("prior, visits, sums, sq, want", [
    # S = 16 (in play sq would be sqrt(17); 4 keeps the arithmetic dyadic). best = 0.5 + 3/11 = 0.773.
    # edge 1: f = 3, scores 0, 0.25 below best, 1.0 not: 3 -> 1 -> 0. edge 2: 0.875 at once: kept. edge 3: f = 1,
    # -0.25 below best: 1 -> 0. edge 4 unvisited.
    ([0.5, 0.25, 0.125, 0.125, 0.0], [10, 3, 2, 1, 0], [5.0, -1.5, 1.0, -1.0, 0.0], 4.0, [10, 0, 2, 0, 0]),
    # S = 63, sq 8, best = 0.5 + 6/41 = 0.646. edge 1: f = 6, 0.5 and 0.6 below, 0.75 not: 6 -> 4 (the PUCT bound
    # stops it). edge 2: f = 4, 0.588, 0.594, 0.6, 0.607 all below: 17 -> 13 (the forced count stops it)
    ([0.5, 0.25, 0.125], [40, 6, 17], [20.0, 0.0, 8.5], 8.0, [40, 4, 13]),
    # a tie of the raw counts: b is the first. S = 12, sq = sqrt(13), best = 0.2254. edge 1 (the other 5): 0.2704
    # not below: kept whole. edge 2: f = 2, -0.324 below, 0.352 not: 2 -> 1 -> 0
    ([0.25, 0.25, 0.25], [5, 5, 2], [0.0, 0.0, -2.0], float(F(np.sqrt(np.float64(13)))), [5, 5, 0]),
    # nothing visited but the best edge
    ([0.5, 0.5], [7, 0], [1.0, 0.0], float(F(np.sqrt(np.float64(8)))), [7, 0]),
])
def test_prune_golden_rows(prior, visits, sums, sq, want):
    got = FP.prune(2.0, 1.5, np.array(prior, dtype=F), visits, np.array(sums, dtype=F), sq)
    assert got == want
    b = visits.index(max(visits))
    assert got[b] == visits[b] and all(0 <= t <= n and t != 1 or t == n for t, n in zip(got, visits))


def test_prune_with_k_zero_and_one_visit():
    # k = 0: the forced count is 0 everywhere, nothing is taken out
    assert FP.prune(0.0, 1.5, np.array([0.5, 0.5], dtype=F), [9, 3], np.array([0.0, -3.0], dtype=F), 3.0) == [9, 3]
    # an edge at one visit that the bound keeps stays at 1 (only a *pruned* edge left at 1 goes to 0)
    assert FP.prune(2.0, 1.5, np.array([0.5, 0.5], dtype=F), [3, 1], np.array([-3.0, 1.0], dtype=F), 2.0) == [3, 1]


# ---- the seeds of the GPU tests
@functools.lru_cache(maxsize=None)
def _games(name):
    r = FP.HASH_RUNS[name]
    q16 = Q16 if r["fast"] else 0
    if r["leaves"] > 1:
        return [FP.play_leaves(SEED + g, r["sims"], r["plies"], r["leaves"], r["fast"], q16, K) for g in range(GAMES)]
    return [FP.play(SEED + g, r["sims"], r["plies"], r["reuse"], r["fast"], q16, K) for g in range(GAMES)]


def _plies(name):
    return [d for g in _games(name) for d in g]


def _edges(plies):
    """(N, T, is the ply's first maximum) of every root edge of the full plies."""
    for d in plies:
        if d["full"]:
            b = d["visits"].index(max(d["visits"]))
            for j, (n, t) in enumerate(zip(d["visits"], d["targets"])):
                yield n, t, j == b


def test_gpu_test_games_exercise_the_rule_and_the_pruning():
    plies = _plies("fresh")
    assert sum(d["forced_diff"] for d in plies) > 0                      # (a) the forced edge beat PUCT's choice
    edges = list(_edges(plies))
    assert any(n > 0 and t == 0 for n, t, _ in edges)                    # (b) pruned to 0
    assert any(1 < t < n for n, t, _ in edges)                           # (c) the PUCT bound stopped it
    assert any(n > 0 and t == n and not top for n, t, top in edges)      # (d) visited, nothing pruned
    assert any(d["pick"] != d["raw_pick"] for d in plies)                # (e) the draw lands elsewhere
    for d in plies:
        assert sum(d["visits"]) == d["target"] and d["pruned"] == sum(d["visits"]) - sum(d["targets"])
        assert all(0 <= t <= n for n, t in zip(d["visits"], d["targets"])) and sum(d["targets"]) > 0
        assert d["targets"][d["pick"]] > 0 and d["played_n"] == d["visits"][d["pick"]]


def test_gpu_test_games_with_fast_sims_hold_both_kinds():
    plies = _plies("pcr")                                                # (f)
    full, fast = [d for d in plies if d["full"]], [d for d in plies if not d["full"]]
    assert full and fast
    assert all(d["targets"] == d["visits"] and d["forced"] == 0 and d["pruned"] == 0 for d in fast)
    assert sum(d["forced"] for d in full) > 0 and sum(d["pruned"] for d in full) > 0


def test_gpu_test_games_with_reuse_fire_on_a_carried_root():
    plies = _plies("carried")                                            # (g)
    assert any(d["carried"] and d["full"] and d["kept"] > 0 and d["forced"] > 0 for d in plies)
    assert any(d["carried"] and d["pruned"] > 0 for d in plies)
    for d in plies:
        assert sum(d["visits"]) == max(d["target"], d["kept"])


def test_gpu_test_games_at_four_leaves_force_on_the_in_flight_counts():
    plies = _plies("leaves")                                             # (h)
    assert sum(d["v_decides"] for d in plies) > 0
    assert sum(d["forced_diff"] for d in plies) > 0 and sum(d["pruned"] for d in plies) > 0
    assert any(step < 4 for d in plies for step in d["accepted"][:-1])   # a collision beside the rule


def test_first_maximum_of_the_targets_under_sample_plies():
    """sample_plies: from that ply on the move is the first maximum of T and the CPython stream is not drawn from,
    so the drawn plies before it are those of the game without it."""
    a = FP.play(SEED, 32, 6, False, 0, 0, K, sample_plies=3)
    b = FP.play(SEED, 32, 3, False, 0, 0, K)
    assert _strip(a[:3]) == _strip(b) and [d["pick"] for d in a[:3]] == [d["pick"] for d in b]
    for d in a[3:]:
        assert d["pick"] == d["targets"].index(max(d["targets"]))
        assert d["raw_pick"] == d["visits"].index(max(d["visits"]))
        assert d["pick"] == d["raw_pick"] and d["pruned"] > 0  # T_b = N_b, T_j <= N_j: the same first maximum
    # tests/test_mcts_forced_gpu.py's run: among the drawn plies of its games the draw lands elsewhere
    drawn = [d for g in range(GAMES) for d in FP.play(SEED + g, 48, 3, False, 0, 0, K, sample_plies=3)]
    assert any(d["pick"] != d["raw_pick"] for d in drawn)
