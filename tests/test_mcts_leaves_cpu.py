"""Several leaves per game in self-play and arena (kv_config.leaves), the part that needs no GPU: the ctypes
mirrors of kv_config / kv_stats, kv_sim_groups_for, and the restatement (tests/_mcts_selfplay_leaves.py) against the
restatements it is built from -- one leaf must be the self-play and arena games of tests/_mcts_selfplay_reuse.py and
tests/_mcts_arena.py, several leaves the position search of tests/_mcts_search.py on the self-play root -- and the
fixed inputs of the GPU tests, which must hold the cases those tests are there for."""
import ctypes as C
import functools

import pytest

from knightvision_amd import _lib
from knightvision_amd.engine import sim_groups_for

from oracle import oracle as O

from tests import _mcts_arena as AR
from tests import _mcts_search as S
from tests import _mcts_selfplay_leaves as SL
from tests import _mcts_selfplay_reuse as RU


# ---- 1. mirrors
def test_mirrors():
    L = _lib.lib()
    assert L.kv_sizeof_config() == C.sizeof(_lib.Config) and L.kv_sizeof_stats() == C.sizeof(_lib.Stats)
    names = [n for n, _ in _lib.Config._fields_]
    assert names[names.index("leaves") + 1] == "arena"
    assert names[-4:] == ["arena", "sample_plies", "sim_groups", "reuse_tree"]
    assert _lib.Config().leaves == 0
    stats = [n for n, _ in _lib.Stats._fields_]
    assert stats[-5:] == ["sim_steps", "leaf_rows_pending", "sims_kept", "roots_carried", "leaf_batch_rows"]


# ---- 2. kv_sim_groups_for
def test_sim_groups_for():
    assert sim_groups_for(2048, 800, leaves=4) == 1
    assert sim_groups_for(2048, 800, 0, True, leaves=4) == 1
    assert sim_groups_for(2048, 800, 1, leaves=4) == 1
    for arena in (False, True):
        with pytest.raises(_lib.KVError, match="leaves 4 with sim_groups 2"):
            sim_groups_for(2048, 800, 2, arena, leaves=4)
    with pytest.raises(_lib.KVError, match="leaves 65 out of range"):
        sim_groups_for(2048, 800, leaves=65)
    for leaves in (0, 1):  # every answer of before
        for slots, sims, groups, arena in [(2048, 800, 0, False), (2047, 800, 0, False), (2048, 0, 0, False),
                                           (256, 800, 0, True), (255, 800, 0, True), (64, 16, 2, False),
                                           (64, 16, 1, True), (34, 16, 2, True)]:
            assert sim_groups_for(slots, sims, groups, arena, leaves=leaves) == sim_groups_for(slots, sims, groups,
                                                                                               arena)
    assert sim_groups_for(2048, 800, leaves=1) == 2 and sim_groups_for(256, 800, 0, True, leaves=1) == 2
    assert sim_groups_for(2047, 800, leaves=0) == 1
    with pytest.raises(_lib.KVError, match="sim_groups 2"):
        sim_groups_for(32, 16, 2, leaves=1)


# ---- 3. the restatement against the existing ones
def test_one_leaf_is_the_selfplay_restatement():
    """Seed 3 at 16 sims: the game whose searches reach terminal leaves at plies 50 and 57."""
    mine = SL.play(3, 0, 16, 60, 1)
    theirs = RU.play(3, 16, 60, False)
    assert len(mine) == len(theirs) == 60
    for p, (x, y) in enumerate(zip(mine, theirs)):
        shared = sorted(set(x) & set(y))
        assert shared == ["move", "visits", "words"]
        assert {k: x[k] for k in shared} == {k: y[k] for k in shared}, p
        assert x["accepted"] == [1] * 16 and [f for step in x["leaf_pending"] for f in step] == y["pending"], p
    assert [p for p, x in enumerate(mine) if not all(f for step in x["leaf_pending"] for f in step)] == [50, 57]


@pytest.mark.parametrize("gid", [2, 3])
def test_one_leaf_is_the_arena_restatement(gid):
    kw = dict(sample_plies=2, eps=0.25)
    mine = SL.play(SL.SEED + gid, gid, 16, 8, 1, arena=True, **kw)
    theirs = AR.play(SL.SEED + gid, gid, 16, 8, **kw)
    assert len(mine) == len(theirs) == 8
    for p, (x, y) in enumerate(zip(mine, theirs)):
        assert sorted(set(x) & set(y)) == ["move", "player", "sampled", "visits", "words"]
        assert {k: x[k] for k in y} == y, p
    assert {x["player"] for x in mine} == {0, 1}


def test_four_leaves_is_the_position_search_on_the_root():
    for seed in (7, 58):
        ply0 = SL.play(seed, 0, 22, 1, 4, eps=0.25, alpha=0.3)[0]
        r = S.search(O.initial_state(), 22, leaves=4, eps=0.25, alpha=0.3, seed=seed)
        assert ply0["visits"] == r["visits"] and ply0["accepted"] == r["accepted"] and ply0["words"] == r["moves"]
        assert sum(len(step) for step in ply0["leaf_pending"]) + 1 == r["nn_rows"]


def test_play_many_is_play_and_counts_the_batch():
    """Four games of 3, 2, 3 and 2 plies on two slots: each game is play()'s own, a ply-step runs as many
    sim-steps as its slowest game, and every pending leaf is counted once."""
    plies, seeds = (3, 2, 3, 2), [SL.SEED + g for g in range(4)]
    starts = SL.starts_of(plies, 2)
    assert starts == [0, 0, 2, 3]
    many, info = SL.play_many(seeds, range(4), 22, plies, 4, lambda sts: [SL.hash_eval(st) for st in sts],
                              starts=starts)
    single = [SL.play(s, g, 22, n, 4) for s, g, n in zip(seeds, range(4), plies)]
    assert many == single
    at = [[g for g in range(4) if starts[g] <= t < starts[g] + plies[g]] for t in range(5)]
    assert at == [[0, 1], [0, 1], [0, 2], [2, 3], [2, 3]]
    assert info["steps"] == sum(max(len(single[g][t - starts[g]]["accepted"]) for g in gs) for t, gs in enumerate(at))
    assert info["pending"] == [sum(f for g in single for x in g for step in x["leaf_pending"] for f in step), 0]
    assert len(info["batches"]) == info["steps"] and sum(a for a, _ in info["batches"]) == info["pending"][0]


# ---- 4. the fixed inputs of the GPU tests are not vacuous
@functools.lru_cache(maxsize=None)
def _restated_run(name):
    cfg = SL.HASH_RUNS[name]
    return {g: SL.play(SL.SEED + g, g, cfg["sims"], n, cfg["leaves"])
            for g, n in zip(range(cfg["base"], cfg["base"] + cfg["n_games"]), cfg["plies"])}


def test_the_gpu_runs_hold_a_collision_a_short_last_step_and_a_terminal_leaf():
    collisions, short, terminal = [], [], []
    for name, cfg in SL.HASH_RUNS.items():
        sims, leaves = cfg["sims"], cfg["leaves"]
        for g, plies in _restated_run(name).items():
            for p, x in enumerate(plies):
                assert sum(x["accepted"]) == sims == sum(x["visits"])
                done = 0
                for k, acc in enumerate(x["accepted"]):
                    budget = min(leaves, sims - done)
                    if acc < budget:
                        collisions.append((name, g, p, k))
                    if k == len(x["accepted"]) - 1 and budget < leaves:
                        short.append((name, g, p))
                    done += acc
                if not all(f for step in x["leaf_pending"] for f in step):
                    terminal.append((name, g, p))
    print(f"collisions {len(collisions)} (first {collisions[:3]}), short last steps {len(short)}, terminal leaves "
          f"{terminal}")
    assert {n for n, *_ in collisions} >= {"tail", "wide"}
    assert ("tail", 19, 7) in {c[:3] for c in collisions}
    assert {n for n, *_ in short} == set(SL.HASH_RUNS)
    assert ("small_class", 15, 5) in terminal
