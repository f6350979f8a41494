"""Forced playouts and policy target pruning in MCTS self-play (kv_config.forced_k; forced_edge in kv_engine.h,
mcts_select_slot / pruned_count / k_mcts_choose in kv_mcts.hip, search_select_tree in kv_search.hip) against its
plain-Python restatement (tests/_mcts_selfplay_forced.py), through the C ABI / SelfPlayEngine.

* Hash evaluator: every PUCT score is bit-reproducible on both sides, so records (moves, boards, the fast flag), the
  raw root visits, the root move words, the pruned targets and the two counters must be identical -- one leaf
  (trees built from nothing or carried, with and without fast_sims) and four leaves (with and without the
  evaluation cache) alike. tests/test_mcts_forced_cpu.py asserts that these very games fire the rule against PUCT's
  own choice, prune to 0, prune partly, keep an edge whole and move the draw.
* Two slot groups give the one-group run's bytes.
* The real ChessNet: the restatement's evaluator returns the HIP network's own rows (tests/_mcts_network.py, the
  > 16-board class), so the same holds, with tests/test_mcts_pcr_gpu.py's rule for network runs: no divergence.
* forced_k = 0 is the engine built without the argument, byte for byte, and kv_root_targets refuses.
* learn.selfplay_shard hands the pruned counts to the policy targets.

The engine runs and the restated games are computed once per configuration and shared by the tests."""
import functools

import numpy as np
import pytest

from knightvision_amd.engine import EVAL_HASH, SelfPlayEngine
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_selfplay_forced as FP
from tests import _mcts_selfplay_reuse as R

pytestmark = pytest.mark.gpu

SEED, NET_SEED, K, Q16, GAMES = FP.SEED, FP.NET_SEED, FP.K, FP.Q16, FP.GAMES


@functools.lru_cache(maxsize=None)
def _run(slots, n_games, sims, steps, forced_k=K, fast=0, reuse=False, leaves=0, hash_eval=True, seed=SEED,
         eval_cache=0, sim_groups=0, sample_plies=0, named=True, variant="init"):
    """One engine run -> (records, root visits, root move words, games, stats, root targets or None). named False:
    the engine is built without naming forced_k."""
    kw = dict(forced_k=forced_k) if named else {}
    if fast:
        kw.update(fast_sims=fast, full_prob=Q16 / 65536.0)
    with SelfPlayEngine(synthetic_state_dict(42, variant), slots=slots, n_games=n_games, seed=seed, max_moves=None,
                        sims=sims, c_puct=1.5, keep_root_moves=True, reuse_tree=reuse, leaves=leaves,
                        eval_cache=eval_cache, sim_groups=sim_groups, sample_plies=sample_plies,
                        eval_mode=EVAL_HASH if hash_eval else 0, **kw) as eng:
        assert eng.cfg.forced_k == (forced_k if named else 0.0)
        eng.run(steps)
        on = named and forced_k > 0
        if not on:
            with pytest.raises(Exception, match="kv_root_targets: engine was created without forced_k"):
                eng.root_targets()
        return (eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats(),
                eng.root_targets() if on else None)


@functools.lru_cache(maxsize=None)
def _restated(name, sample_plies=0):
    r = FP.HASH_RUNS[name]
    q16 = Q16 if r["fast"] else 0
    kw = dict(sample_plies=sample_plies)
    if r["leaves"] > 1:
        return {g: FP.play_leaves(SEED + g, r["sims"], r["plies"], r["leaves"], r["fast"], q16, K, **kw)
                for g in range(GAMES)}
    return {g: FP.play(SEED + g, r["sims"], r["plies"], r["reuse"], r["fast"], q16, K, **kw) for g in range(GAMES)}


def _hash_run(name, **kw):
    r = FP.HASH_RUNS[name]
    return _run(GAMES, GAMES, r["sims"], r["plies"], fast=r["fast"], reuse=r["reuse"], leaves=r["leaves"], **kw)


def _divergences(run, restated):
    """Plies at which a game's record (move, board, fast flag), raw root visits, root move words or pruned targets
    differ from the restatement's."""
    recs, visits, words, targets = run[0], run[1], run[2], run[5]
    bad = []
    for g, plies in restated.items():
        sel = recs["game_id"] == g
        assert (np.diff(recs["ply"][sel]) == 1).all() and sel.sum() == len(plies), g
        for p, ply in enumerate(plies):
            n = len(ply["visits"])
            ok = (recs["move"][sel][p] == ply["move"] and np.array_equal(visits[sel][p][:n], ply["visits"])
                  and (visits[sel][p][n:] == -1).all() and np.array_equal(words[sel][p][:n], ply["words"])
                  and (words[sel][p][n:] == 0xffff).all()
                  and np.array_equal(targets[sel][p][:n], ply["targets"]) and (targets[sel][p][n:] == -1).all()
                  and recs["pad"][sel][p] == (0 if ply["full"] else 1)
                  and recs["board"][sel][p].tobytes() == plies.extra[p]["board"])
            if not ok:
                bad.append((g, p))
                print(f"game {g} ply {p}: GPU visits {visits[sel][p][:n]} targets {targets[sel][p][:n]} move "
                      f"{recs['move'][sel][p]} restated {ply['visits']} / {ply['targets']} move {ply['move']} "
                      f"(full {ply['full']}, kept {ply['kept']})")
                break  # the games part here
    return bad


def _all(rest):
    return [ply for g in rest.values() for ply in g]


def _check_counters(st, rest):
    plies = _all(rest)
    assert st["plies"] == len(plies)
    assert st["sims"] == sum(ply["rem"] for ply in plies)
    assert st["forced_descents"] == sum(ply["forced"] for ply in plies) > 0
    assert st["visits_pruned"] == sum(ply["pruned"] for ply in plies) > 0
    assert st["plies_fast"] == sum(not ply["full"] for ply in plies)
    return plies


def _check_raw_invariants(run):
    """The raw counts keep every invariant they had: each row sums to what sims and sims_kept count."""
    st = run[4]
    vis = np.where(run[1] < 0, 0, run[1]).sum(1)
    assert vis.sum() == st["sims"] + st["sims_kept"]
    tg = np.where(run[5] < 0, 0, run[5])
    assert (tg <= np.where(run[1] < 0, 0, run[1])).all() and (tg.sum(1) > 0).all()
    assert vis.sum() - tg.sum() == st["visits_pruned"]


# ---- 1. hash evaluator, one leaf: every tree built from nothing, carried trees, with fast_sims
@pytest.mark.parametrize("name", ["fresh", "carried", "pcr"])
def test_forced_hash_games_identical_to_restatement(name):
    run, rest = _hash_run(name), _restated(name)
    assert _divergences(run, rest) == []
    plies = _check_counters(run[4], rest)
    _check_raw_invariants(run)
    st = run[4]
    if name == "carried":
        assert st["sims_kept"] == sum(ply["kept"] for ply in plies) > 0
        assert st["roots_carried"] == sum(ply["carried"] for ply in plies) > 0
    else:
        assert st["sims_kept"] == 0
        assert st["sims"] == st["plies_full"] * 48 + st["plies_fast"] * 4
    if name == "pcr":
        assert st["plies_fast"] > 0 and st["plies_full"] > 0
        fast = run[0]["pad"] == 1
        assert fast.sum() == st["plies_fast"] and np.array_equal(run[5][fast], run[1][fast])  # T = N on a fast ply
    assert any(ply["pick"] != ply["raw_pick"] for ply in plies)


# ---- 2. hash evaluator, four leaves, with and without the evaluation cache
def test_forced_leaves_hash_games_identical_to_restatement():
    run, rest = _hash_run("leaves"), _restated("leaves")
    assert _divergences(run, rest) == []
    plies = _check_counters(run[4], rest)
    _check_raw_invariants(run)
    st = run[4]
    assert sum(ply["v_decides"] for ply in plies) > 0
    assert st["leaf_rows_pending"] == sum(sum(step) for ply in plies for step in ply["leaf_pending"])
    cached = _hash_run("leaves", eval_cache=1024)
    for k in (0, 1, 2, 3, 5):
        assert cached[k].tobytes() == run[k].tobytes(), k
    for key in ("plies", "sims", "sim_steps", "leaf_rows_pending", "forced_descents", "visits_pruned"):
        assert cached[4][key] == st[key], key
    assert cached[4]["cache_probes"] == st["leaf_rows_pending"]


# ---- 3. the first maximum of the pruned counts
def test_forced_sample_plies_takes_the_first_maximum_of_the_targets():
    run, rest = _hash_run("fresh", sample_plies=3), _restated("fresh", sample_plies=3)
    assert _divergences(run, rest) == []
    _check_counters(run[4], rest)
    # T_b = N_b and T_j <= N_j: the first maximum of T is the first maximum of N, so from ply 3 on the rule shows
    # in the search (the raw counts, compared above) and in the targets, never in the move
    late = [ply for g in rest.values() for ply in g[3:]]
    assert all(ply["pick"] == ply["raw_pick"] for ply in late) and sum(ply["pruned"] for ply in late) > 0
    assert any(ply["pick"] != ply["raw_pick"] for g in rest.values() for ply in g[:3])  # the drawn plies differ


# ---- 4. two slot groups against one
def test_forced_two_slot_groups_give_the_one_group_run():
    g1 = _run(64, 64, 16, 4, sim_groups=1)
    g2 = _run(64, 64, 16, 4, sim_groups=2)
    for k in (0, 1, 2, 3, 5):
        assert g1[k].tobytes() == g2[k].tobytes(), k
    for key in ("plies", "sims", "forced_descents", "visits_pruned"):
        assert g1[4][key] == g2[4][key], key
    assert g1[4]["forced_descents"] > 0 and g1[4]["visits_pruned"] > 0 and g1[4]["plies"] == 64 * 4


# ---- 5. the real network
def test_forced_network_games_identical_to_restatement():
    """17 slots (the > 16-board class) x 32 sims x 6 ply-steps on the `init` weights: games 0-3 against the
    restatement fed the HIP network's own rows, tests/test_mcts_pcr_gpu.py's rule for network runs (no divergence
    allowed: the evaluator's rows are the engine's bit for bit)."""
    from tests._mcts_network import hip_eval
    slots, sims, n_plies = 17, 32, 6
    run = _run(slots, slots, sims, n_plies, hash_eval=False, seed=NET_SEED)
    games = tuple(range(4))
    ev, net = hip_eval(synthetic_state_dict(42, "init"))
    try:
        rest = dict(zip(games, FP.play_many([NET_SEED + g for g in games], sims, [n_plies] * 4, False, 0, 0, K,
                                            R.net_eval(ev))))
    finally:
        net.close()
    bad = _divergences(run, rest)
    plies = _all(rest)
    print(f"forced network parity: {len(plies)} root vectors compared, forced {sum(p['forced'] for p in plies)}, "
          f"pruned {sum(p['pruned'] for p in plies)}, divergences {len(bad)}")
    assert bad == []
    assert sum(p["forced"] for p in plies) > 0 and sum(p["pruned"] for p in plies) > 0
    _check_raw_invariants(run)
    assert run[4]["sims"] == slots * sims * n_plies


# ---- 6. off is off
@pytest.mark.parametrize("reuse, leaves", [(False, 0), (True, 0), (False, 4)])
def test_forced_k_zero_is_the_engine_without_it(reuse, leaves):
    kw = dict(reuse=reuse, leaves=leaves)
    off = _run(GAMES, GAMES, 16, 8, forced_k=0.0, **kw)
    unnamed = _run(GAMES, GAMES, 16, 8, named=False, **kw)
    on = _run(GAMES, GAMES, 16, 8, **kw)
    for k in range(4):  # records, root visits, root moves, the game table
        assert off[k].tobytes() == unnamed[k].tobytes(), k
    for key in ("plies", "sims", "sims_kept", "roots_carried", "nn_rows", "leaf_rows_pending", "sim_steps"):
        assert off[4][key] == unnamed[4][key], key
    for st in (off[4], unnamed[4]):
        assert st["forced_descents"] == 0 and st["visits_pruned"] == 0
    assert off[5] is None and unnamed[5] is None  # (_run saw kv_root_targets refuse on both)
    assert on[4]["forced_descents"] > 0 and on[1].tobytes() != off[1].tobytes()  # and on is not off


# ---- 7. the learn seam
def test_selfplay_shard_hands_the_pruned_counts_to_the_policy_targets(monkeypatch):
    import torch

    from knightvision_amd import learn
    from knightvision_amd.model import ChessNet
    from knightvision_amd.policy_targets import PolicyTargets
    seen = {}

    class Spy(SelfPlayEngine):
        def root_targets(self):
            seen["targets"] = super().root_targets()
            seen["visits"] = super().root_visits()
            seen["stats"] = self.stats()
            return seen["targets"]

    monkeypatch.setattr(learn, "SelfPlayEngine", Spy)
    torch.manual_seed(0)
    model = ChessNet().to("cuda:0").eval()
    recs, games, counts, moves = learn.selfplay_shard(model, 4, 0, "cuda:0", sims=32, max_moves=6, slots=4,
                                                      policy_targets=True, forced_k=2.0)
    assert len(recs) == 24 and counts.dtype == np.uint16
    assert np.array_equal(counts, seen["targets"].astype(np.uint16))
    assert not np.array_equal(seen["targets"], seen["visits"]) and seen["stats"]["visits_pruned"] > 0
    t = PolicyTargets.from_engine(counts, moves, "cpu")
    rows = torch.repeat_interleave(torch.arange(len(t)), t.lengths())
    sums = torch.zeros(len(t), dtype=torch.int64).index_add_(0, rows, t.cnt.to(torch.int64) & 0xffff)
    want = np.where(seen["targets"] < 0, 0, seen["targets"]).sum(1)
    assert np.array_equal(sums.numpy(), want) and (want > 0).all()
    assert want.sum() == 24 * 32 - seen["stats"]["visits_pruned"]
    # without forced_k the third array is the raw visits, as ever
    raw = learn.selfplay_shard(model, 4, 0, "cuda:0", sims=32, max_moves=6, slots=4, policy_targets=True)
    assert "targets" in seen and np.where(raw[2] == 0xffff, 0, raw[2]).sum(1).tolist() == [32] * 24
