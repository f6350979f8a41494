"""MCTS self-play with carried subtrees (kv_config.reuse_tree; k_mcts_root / k_mcts_carry in kv_mcts.hip, the
live-slot leaf batches of kv_run) against its plain-Python restatement (tests/_mcts_selfplay_reuse.py),
through the C ABI.

* Hash evaluator: every PUCT score is bit-reproducible on both sides, so moves, root visit vectors and root
  move words must be identical.
* The real ChessNet: the restatement's evaluator returns the HIP network's own rows, evaluated in the
  > 16-board class the engine's batches are in (batch-invariant bit for bit inside it), so the same holds.
* The schedule: a game does not depend on its neighbours or on when the leaf batch was compacted, and the
  rows the network ran are those of the live slots, padded to the class.

The engine runs and the restated games are computed once per configuration and shared by the tests."""
import functools

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import EVAL_HASH, SelfPlayEngine, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_selfplay_reuse as R

pytestmark = pytest.mark.gpu

SEED = 49  # tests/test_mcts_reuse_cpu.py: these games carry on most plies
CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class


@functools.lru_cache(maxsize=None)
def _run(variant, slots, n_games, sims, steps, max_moves=None, reuse=True, hash_eval=False):
    """One engine run -> (records, root visits, root move words, games, stats)."""
    with SelfPlayEngine(synthetic_state_dict(42, variant), slots=slots, n_games=n_games, seed=SEED,
                        max_moves=max_moves, sims=sims, c_puct=1.5, keep_root_moves=True, reuse_tree=reuse,
                        eval_mode=EVAL_HASH if hash_eval else 0) as eng:
        eng.run(steps)
        return eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()


_NETS = {}


def _net(variant):
    from knightvision_amd.model import KVNet
    if variant not in _NETS:
        _NETS[variant] = KVNet(0, packed_from(synthetic_state_dict(42, variant)))
    return _NETS[variant]


@pytest.fixture(scope="module", autouse=True)
def _close_nets():
    yield
    while _NETS:
        _NETS.popitem()[1].close()


def _hip_eval_many(variant):
    """The restatement's evaluator: the HIP network's rows of a list of positions, computed as one batch of
    the engine's class (test_mcts_gpu.py's _hip_eval: fewer than 17 positions are padded with copies of the
    first; the board codes are the state vector's)."""
    net = _net(variant)

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


@functools.lru_cache(maxsize=None)
def _restated(variant, games, sims, plies, hash_eval=False):
    """The restated games `games` (ids), game g over plies[g] plies -> {g: per-ply dicts}."""
    seeds = [SEED + g for g in games]
    if hash_eval:
        return {g: R.play(s, sims, n, True) for g, s, n in zip(games, seeds, plies)}
    return dict(zip(games, R.play_many(seeds, sims, plies, True, _hip_eval_many(variant))))


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
                print(f"game {g} ply {p}: GPU visits {visits[sel][p][:n]} restated {ply['visits']} "
                      f"(kept {ply['kept']})")
                break  # the games part here
    return bad


def _plies_of(run, games):
    return tuple(int((run[0]["game_id"] == g).sum()) for g in games)


@pytest.mark.parametrize("sims", [16, 64, 200])
def test_reuse_hash_games_identical_to_restatement(sims):
    run = _run("init", 6, 6, sims, 12, hash_eval=True)
    games = tuple(range(6))
    plies = _plies_of(run, games)
    assert sum(plies) == run[4]["plies"] and min(plies) >= 1
    rest = _restated("init", games, sims, plies, hash_eval=True)
    assert _divergences(run, rest, sims) == []
    st = run[4]
    kept = sum(ply["kept"] for g in rest.values() for ply in g)
    carried = sum(ply["carried"] for g in rest.values() for ply in g)
    print(f"hash, {sims} sims: {st['plies']} plies, {st['roots_carried']} carried roots, {st['sims_kept']} of "
          f"{st['plies'] * sims} root visits kept")
    assert st["sims"] + st["sims_kept"] == st["plies"] * sims
    assert st["roots_carried"] > 0
    assert (st["sims_kept"], st["roots_carried"]) == (kept, carried)


@pytest.mark.parametrize("variant", ["init", "peaked"])
def test_reuse_network_games_identical_to_restatement(variant):
    """The > 16-board class: 17 slots x 32 sims x 6 plies, the first 4 games against the restatement."""
    run = _run(variant, 17, 17, 32, 6)
    games = tuple(range(4))
    rest = _restated(variant, games, 32, _plies_of(run, games))
    bad = _divergences(run, rest, 32)
    print(f"reuse network parity ({variant}): {sum(len(g) for g in rest.values())} root vectors compared, "
          f"kept per ply {[[ply['kept'] for ply in g] for g in rest.values()]}, divergences {len(bad)}")
    assert bad == []
    st = run[4]
    assert st["sims"] + st["sims_kept"] == st["plies"] * 32 and st["roots_carried"] > 0


def test_reuse_games_independent_of_neighbours_and_compaction():
    """The same seeds on 17 and on 40 slots: other rem values around a game change when its slot leaves the
    leaf batch and when the batch is compacted, never the game."""
    a, b = _run("peaked", 17, 17, 32, 6), _run("peaked", 40, 40, 32, 6)
    for g in range(17):
        sa, sb = a[0]["game_id"] == g, b[0]["game_id"] == g
        assert sa.sum() == 6 and sb.sum() == 6
        assert a[0][sa].tobytes() == b[0][sb].tobytes(), g
        assert a[1][sa].tobytes() == b[1][sb].tobytes(), g
        assert a[2][sa].tobytes() == b[2][sb].tobytes(), g


def test_reuse_recycled_slots_and_tails_identical_to_restatement():
    """20 games on 17 slots, 10 plies each: recycled slots start from a fresh root (the restatement starts
    every game fresh, and the engine's kept / carried totals are its own), and the tail runs with fewer
    active slots than slots."""
    sims = 16
    run = _run("peaked", 17, 20, sims, -1, max_moves=10)
    games = tuple(range(20))
    assert len(run[3]) == 20
    plies = _plies_of(run, games)
    assert plies == tuple(int(p) for p in run[3]["plies"][np.argsort(run[3]["game_id"])])
    rest = _restated("peaked", games, sims, plies)
    assert _divergences(run, rest, sims) == []
    assert all(g[0]["kept"] == 0 and not g[0]["carried"] for g in rest.values())
    st = run[4]
    assert st["sims_kept"] == sum(ply["kept"] for g in rest.values() for ply in g)
    assert st["roots_carried"] == sum(ply["carried"] for g in rest.values() for ply in g)
    assert st["sims"] + st["sims_kept"] == st["plies"] * sims


def test_reuse_leaf_batch_rows_are_the_live_slots():
    """40 slots x 32 sims x 6 plies: per sim-step the network ran the live slots' rows, padded to the class,
    at most KV_REUSE_COMPACT_STEP - 1 stale ones with them -- and fewer than without reuse."""
    slots, sims, n_plies, step = 40, 32, 6, _lib.REUSE_COMPACT_STEP
    run = _run("peaked", slots, slots, sims, n_plies)
    games = tuple(range(slots))
    plies = _plies_of(run, games)
    assert plies == (n_plies,) * slots
    rest = _restated("peaked", games, sims, plies)
    assert _divergences(run, rest, sims) == []
    lo = hi = 0
    for p in range(n_plies):
        rem = np.array([rest[g][p]["rem"] for g in games])
        for k in range(int(rem.max())):
            live = int((rem > k).sum())
            lo += max(live, CLASS_ROWS)
            hi += max(live + step - 1, CLASS_ROWS)
    rows = run[4]["leaf_batch_rows"]
    off = _run("peaked", slots, slots, sims, n_plies, reuse=False)[4]
    print(f"leaf batch rows: {rows} with reuse (bounds {lo}..{hi}), {off['leaf_batch_rows']} without")
    assert lo <= rows <= hi
    assert off["leaf_batch_rows"] == slots * sims * n_plies and off["sims_kept"] == 0 and off["roots_carried"] == 0
    assert rows < off["leaf_batch_rows"]


def test_reuse_visit_targets_build():
    """policy_target="visits" works unchanged: every root still holds sims visits."""
    from knightvision_amd.policy_targets import PolicyTargets
    run = _run("peaked", 17, 17, 32, 6)
    pt = PolicyTargets.from_engine(run[1].astype("uint16"), run[2], "cuda")
    off = pt.off.cpu().numpy()
    cnt = pt.cnt.cpu().numpy().view(np.uint16).astype(np.int64)
    assert len(off) == len(run[0]) + 1
    assert (np.add.reduceat(cnt, off[:-1]) == 32).all()
    assert run[4]["roots_carried"] > 0
