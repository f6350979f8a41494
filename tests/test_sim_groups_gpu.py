"""Slot groups of the MCTS sim loop (kv_config.sim_groups): a move's sim-steps as two groups of slots, each chain
(leaf forward, backup + select) on a stream of its own with its own network workspaces, against one group.

Every board's network row is independent of its batch inside the > 16-board class, every slot's tree and RNG are
its own, and records are allocated by the all-slot kernels on the engine stream, so two groups must reproduce one
group byte for byte: records, root visit counts, the game table and the stats counters."""
import numpy as np
import pytest

from knightvision_amd.engine import EVAL_FAITHFUL, EVAL_HASH, SelfPlayEngine, sim_groups_for
from knightvision_amd.weights import synthetic_state_dict

COUNTERS = ("steps", "plies", "games_done", "nn_rows", "sims", "records", "tree_overflows", "nn_rows_lazy",
            "sims_kept", "roots_carried", "leaf_batch_rows")


@pytest.fixture(scope="module")
def weights():
    return synthetic_state_dict(42, "init")


def _run(weights, groups, moves, **kw):
    with SelfPlayEngine(weights, seed=42, c_puct=1.5, keep_root_visits=True, sim_groups=groups, **kw) as eng:
        eng.run(moves)
        st = eng.stats()
        return eng.records(), eng.root_visits(), eng.games(), {k: st[k] for k in COUNTERS}


def _same(weights, moves, **kw):
    assert sim_groups_for(kw["slots"], kw["sims"], 2) == 2
    one, two = _run(weights, 1, moves, **kw), _run(weights, 2, moves, **kw)
    assert one[3]["sims"] > 0 and len(one[0]) > 0
    for a, b, what in zip(one[:3], two[:3], ("records", "root visits", "games")):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differ between one and two groups"
    assert one[3] == two[3]
    return one


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [64, 96])  # groups of 32 (the smallest above the 16-board class) and of 48
def test_two_groups_equal_one(weights, slots):
    rec, visits, _, st = _same(weights, 3, slots=slots, n_games=slots, sims=16, max_moves=None)
    assert len(rec) == 3 * slots and st["sims"] == 3 * slots * 16 and st["leaf_batch_rows"] == 3 * slots * 16
    assert np.all(visits.clip(min=0).sum(axis=1) == 16)


@pytest.mark.gpu
def test_two_groups_with_recycling(weights):
    # 2-ply games: slots finish and start the next game id inside the run, and the last plies run with fewer
    # active slots than slots (the compact leaf batch, which runs as one group)
    _, _, games, st = _same(weights, 6, slots=64, n_games=160, sims=16, max_moves=2)
    assert st["games_done"] == 160 and len(games) == 160


@pytest.mark.gpu
def test_two_groups_hash_evaluator(weights):
    _same(weights, 3, slots=64, n_games=64, sims=16, max_moves=None, eval_mode=EVAL_HASH)


@pytest.mark.gpu
def test_two_groups_reuse_tree(weights):
    _, _, _, st = _same(weights, 3, slots=64, n_games=64, sims=16, max_moves=None, reuse_tree=True,
                        eval_mode=EVAL_FAITHFUL)
    assert st["roots_carried"] > 0


def test_auto_rule():
    """auto: two groups only from 2,048 slots in MCTS mode (each group keeps the fused stem's 1,024-board floor)"""
    assert sim_groups_for(2048, 800) == 2 and sim_groups_for(4096, 1) == 2
    assert sim_groups_for(2047, 800) == 1 and sim_groups_for(1024, 800) == 1 and sim_groups_for(64, 16) == 1
    assert sim_groups_for(2048, 0) == 1 and sim_groups_for(1 << 20, 0) == 1
    assert sim_groups_for(2048, 800, 1) == 1 and sim_groups_for(64, 16, 2) == 2
    for bad in ((32, 16, 2), (2048, 0, 2), (64, 16, 3)):  # a group in the <= 16-board class, no search, no such mode
        with pytest.raises(Exception):
            sim_groups_for(*bad)
