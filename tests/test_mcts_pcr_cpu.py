"""Playout cap randomization (kv_config.fast_sims / full_q16, DESIGN.md "Playout cap randomization"), the parts
that need no GPU: the config validation and the ctypes mirrors, the plain-Python restatement
(tests/_mcts_selfplay_pcr.py) pinned to the restatements it is built from with every ply full, the kind
function on the seeds and plies the GPU tests use, and the per-sample weights of the policy loss."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _mcts_selfplay_leaves as LV
from tests import _mcts_selfplay_pcr as P
from tests import _mcts_selfplay_reuse as R

SEED, NET_SEED, Q16 = P.SEED, P.NET_SEED, P.Q16
GAMES, PLY_STEPS = 6, 12  # tests/test_mcts_pcr_gpu.py's hash-evaluator runs
ADDED = ("full", "target", "kept", "rem")


def _cfg(**kw):
    from knightvision_amd import _lib
    base = dict(device=0, slots=4, n_games=4, game_id_base=0, game_id_stride=1, seed=42, seed_mode=0, max_moves=0,
                batch=16, eps=0.25, alpha=0.3, sims=16, c_puct=1.5, eval_mode=0, record_cap=0, recycle=1,
                precision=0, algo=0, tree_edge_cap=0, keep_root_visits=0)
    base.update(kw)
    return _lib.Config(**base)


@pytest.mark.parametrize("kw, msg", [
    (dict(fast_sims=-1, full_q16=16384), "fast_sims -1 out of range"),
    (dict(fast_sims=16, full_q16=16384), "fast_sims 16 out of range"),
    (dict(fast_sims=17, full_q16=16384), "fast_sims 17 out of range"),
    (dict(fast_sims=4, full_q16=0), "full_q16 0 out of range [1, 65536]"),
    (dict(fast_sims=4, full_q16=65537), "full_q16 65537 out of range [1, 65536]"),
    (dict(fast_sims=4, full_q16=-5), "full_q16 -5 out of range [1, 65536]"),
    (dict(fast_sims=0, full_q16=16384), "full_q16 16384 with fast_sims 0"),
    (dict(fast_sims=4, full_q16=16384, sims=0), "fast_sims 4 with sims 0"),
    (dict(fast_sims=4, full_q16=16384, arena=1), "fast_sims 4 with arena 1"),
])
def test_kv_create_rejects_bad_pcr_configs(kw, msg):
    """Validated before the device is touched: KV_EINVAL, the reason in kv_last_error(), a NULL handle."""
    from knightvision_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _cfg(**kw)
    assert L.kv_create(C.byref(cfg), C.byref(h)) == -1  # KV_EINVAL
    assert msg in L.kv_last_error().decode()
    assert not h.value


def test_config_and_stats_mirrors():
    from knightvision_amd import _lib
    L = _lib.lib()
    assert L.kv_sizeof_config() == C.sizeof(_lib.Config)
    assert L.kv_sizeof_stats() == C.sizeof(_lib.Stats)
    names = [n for n, _ in _lib.Config._fields_]
    k = names.index("keep_root_visits")
    assert names[k:k + 4] == ["keep_root_visits", "fast_sims", "full_q16", "eval_cache"]
    assert dict(_lib.Config._fields_)["fast_sims"] is C.c_int and dict(_lib.Config._fields_)["full_q16"] is C.c_int
    stats = [n for n, _ in _lib.Stats._fields_]
    a = stats.index("arena_rows")
    assert stats[a - 2:a + 1] == ["plies_full", "plies_fast", "arena_rows"]
    assert dict(_lib.Stats._fields_)["plies_full"] is C.c_int64 and dict(_lib.Stats._fields_)["plies_fast"] is C.c_int64
    zero = _lib.Config()
    assert zero.fast_sims == 0 and zero.full_q16 == 0  # a zeroed config: the feature is off


def test_engine_options_default_to_off():
    import inspect

    from knightvision_amd import learn
    from knightvision_amd.engine import SelfPlayEngine
    for fn in (SelfPlayEngine.__init__, learn.selfplay_shard, learn.reinforcement_loop):
        sig = inspect.signature(fn).parameters
        assert sig["fast_sims"].default == 0 and sig["full_prob"].default == 0.25


def _strip(plies):
    return [{k: v for k, v in d.items() if k not in ADDED} for d in plies]


@pytest.mark.parametrize("reuse", [False, True])
def test_every_ply_full_is_the_reuse_restatement(reuse):
    """3 seeds x 6 plies x 16 sims on the hash evaluator, full_q16 = 65536: ply for ply
    tests/_mcts_selfplay_reuse.play, which tests/test_mcts_reuse_cpu.py pins to the C oracle."""
    for seed in (49, 50, 51):
        a, b = P.play(seed, 16, 6, reuse, 4, 65536), R.play(seed, 16, 6, reuse)
        assert len(a) == len(b) == 6
        for x, y in zip(a, b):
            assert x["full"] and x["target"] == 16 and x["rem"] == 16 - x["kept"]
            assert {k: v for k, v in x.items() if k not in ("full", "target")} == y
        assert a.extra == b.extra


def test_every_ply_full_is_the_leaves_restatement():
    """The same at L = 4 against tests/_mcts_selfplay_leaves.play (pinned by tests/test_mcts_leaves_cpu.py)."""
    for seed in (49, 50, 51):
        a, b = P.play_leaves(seed, 16, 6, 4, 4, 65536), LV.play(seed, 0, 16, 6, 4)
        assert len(a) == len(b) == 6
        assert all(x["full"] and x["target"] == 16 and x["kept"] == 0 and x["rem"] == 16 for x in a)
        assert _strip(a) == list(b)
        assert a.extra == b.extra


def test_feature_off_is_every_ply_full():
    a, b = P.play(49, 16, 6, True, 0, 0), P.play(49, 16, 6, True, 4, 65536)
    assert list(a) == list(b)


def test_kind_function():
    """The hash, restated once more from its definition, and its rate: about full_q16 / 65536 of the plies."""
    def ref(key, ply, q16):
        m = (1 << 64) - 1
        x = (key * 0x9E3779B97F4A7C15 + (ply + 1) * 0xD1B54A32D192ED03) & m
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & m
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & m
        x ^= x >> 31
        return (x >> 48) < q16
    for key in (0, 1, 49, 2 ** 63 + 5):
        for ply in (0, 1, 7, 500):
            assert P.kind(key, ply, Q16) == ref(key, ply, Q16)
            assert P.kind(key, ply, 65536) and P.target(key, ply, 64, 4, 65536) == (True, 64)
    full = sum(P.kind(SEED + g, p, Q16) for g in range(200) for p in range(100))
    assert 0.22 < full / 20000 < 0.28  # 20,000 draws at 1/4: sigma 0.003
    assert P.target(5, 3, 64, 0, 0) == (True, 64)  # the feature off


def test_gpu_test_games_hold_both_kinds_and_a_rem_zero_ply():
    """The seeds and plies of tests/test_mcts_pcr_gpu.py: at full_q16 = 16384 the 6 games x 12 plies hold both
    kinds; with reuse on, fast_sims 2 and sims 64 they hold plies with rem = 0, and every root's visits sum to
    max(target, kept)."""
    kinds = [P.kind(SEED + g, p, Q16) for g in range(GAMES) for p in range(PLY_STEPS)]
    assert any(kinds) and not all(kinds)
    zero = 0
    for g in range(GAMES):
        plies = P.play(SEED + g, 64, PLY_STEPS, True, 2, Q16)
        for d in plies:
            assert d["target"] == (64 if d["full"] else 2)
            assert d["rem"] == max(d["target"] - d["kept"], 0) and len(d["pending"]) == d["rem"]
            assert sum(d["visits"]) == max(d["target"], d["kept"])
            zero += d["rem"] == 0
    assert zero >= 1
    # the network runs (17 games x 6 plies): both kinds in the compared games 0-3, and a ply-step at which every
    # game is fast, so that the ply-step runs fewer sim-steps than any ply-step of the feature-off engine
    kinds = [P.kind(NET_SEED + g, p, Q16) for g in range(4) for p in range(6)]
    assert any(kinds) and not all(kinds)
    assert any(not any(P.kind(NET_SEED + g, p, Q16) for g in range(17)) for p in range(6))


def test_every_root_draws_the_noise_and_a_fast_one_drops_it(monkeypatch):
    """One root_priors call -- one Dirichlet draw from the game's numpy stream -- per ply whatever its kind, with
    eps 0 on a fast ply and the configured eps on a full one."""
    calls = []
    real = P.root_priors

    def spy(logits, words, np_mt, eps, alpha):
        calls.append(eps)
        return real(logits, words, np_mt, eps, alpha)

    monkeypatch.setattr(P, "root_priors", spy)
    for play in (lambda: P.play(SEED + 5, 16, 8, True, 4, Q16), lambda: P.play_leaves(SEED + 5, 16, 8, 4, 4, Q16)):
        calls.clear()
        plies = play()
        assert len(calls) == len(plies) == 8
        assert calls == [0.25 if d["full"] else 0.0 for d in plies]
        assert 0.0 in calls and 0.25 in calls


# ---- the per-sample weights of the policy targets and the loss
def _targets():
    from knightvision_amd.policy_targets import PolicyTargets
    vis = np.full((5, 320), 0xffff, dtype=np.uint16)
    mov = np.full((5, 320), 0xffff, dtype=np.uint16)
    rng = np.random.RandomState(3)
    for r, n in enumerate((3, 20, 1, 7, 30)):
        vis[r, :n] = rng.randint(0, 40, n)
        vis[r, 0] = 5
        mov[r, :n] = rng.choice(4096, n, replace=False)
    w = np.array([1, 0, 1, 0, 1], dtype=np.float32)
    return PolicyTargets.from_engine(vis, mov, "cpu", weights=w), PolicyTargets.from_engine(vis, mov, "cpu"), w


def test_policy_target_weights_survive_row_operations():
    from knightvision_amd.policy_targets import PolicyTargets
    t, plain, w = _targets()
    assert plain.w is None and torch.equal(plain.weights(), torch.ones(5))
    assert t.w.dtype == torch.float32 and torch.equal(t.w, torch.from_numpy(w))
    assert torch.equal(t.off, plain.off) and torch.equal(t.idx, plain.idx) and torch.equal(t.cnt, plain.cnt)
    mask = torch.tensor([True, True, False, False, True])
    assert torch.equal(t[mask].w, torch.tensor([1.0, 0.0, 1.0])) and len(t[mask]) == 3
    rows = torch.tensor([4, 1, 1, 0])
    assert torch.equal(t[rows].w, torch.tensor([1.0, 0.0, 0.0, 1.0]))
    assert torch.equal(t[rows].dense(), plain[rows].dense())
    assert plain[rows].w is None  # targets without weights stay without
    both = PolicyTargets.cat([plain, t, PolicyTargets.one_hot(torch.tensor([7, 9]))])
    assert torch.equal(both.w, torch.tensor([1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1], dtype=torch.float32))
    assert PolicyTargets.cat([plain, plain]).w is None
    assert torch.equal(t.to("cpu").w, t.w)
    with pytest.raises(ValueError, match="weights"):
        PolicyTargets.from_engine(np.zeros((2, 320), np.uint16), np.zeros((2, 320), np.uint16), "cpu",
                                  weights=np.ones(3))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Linear(768, 4096)
        self.v = torch.nn.Linear(768, 1)

    def forward(self, x):
        x = x.reshape(x.shape[0], -1)
        return self.p(x), torch.tanh(self.v(x))


def test_batch_loss_weighted_policy_term_matches_fp64():
    """batch_loss on CPU tensors against the fp64 restatement of (ce * w).sum() / w.sum(); the entropy and value
    terms run over all rows. Tolerance: tests/test_policy_targets_cpu.py's own (1e-5 absolute)."""
    from knightvision_amd import train as T
    t, plain, w = _targets()
    torch.manual_seed(0)
    net = _Net()
    g = torch.Generator().manual_seed(1)
    boards = (torch.rand(4, 12, 8, 8, generator=g) > 0.9).float()
    rows = torch.tensor([3, 0, 1, 4])
    b = T.Batch(boards, torch.zeros(4, dtype=torch.int64), torch.tensor([1.0, -1.0, 0.2, 1.0]), t, rows)
    loss, lp, lv, ent, pol = T.batch_loss(net, b, amp=False)
    z = pol.detach().double()
    logp = F.log_softmax(z, 1)
    ce = -(plain.dense(rows, dtype=torch.float64) * logp).sum(1)
    wr = torch.from_numpy(w).double()[rows]
    assert wr.sum() == 2
    want = float((ce * wr).sum() / wr.sum())
    assert lp.item() == pytest.approx(want, abs=1e-5)
    assert abs(want - float(ce.mean())) > 1e-3  # the weights matter on this batch
    assert ent.item() == pytest.approx(float(-(logp.exp() * logp).sum(1).mean()), abs=1e-5)
    ev = T.evaluate(net, [b])
    assert ev == pytest.approx(want + lv.item(), abs=1e-5)
    # targets without weights: the unweighted mean, as ever
    lp0 = T.batch_loss(net, T.Batch(boards, b.moves, b.outcomes, plain, rows), amp=False)[1]
    assert lp0.item() == pytest.approx(float(ce.mean()), abs=1e-5)
    # a batch of fast plies only: the policy term is 0 (w.sum() = 0 -> the divisor is 1), not NaN
    b0 = T.Batch(boards[:2], b.moves[:2], b.outcomes[:2], t, torch.tensor([1, 3]))
    assert T.batch_loss(net, b0, amp=False)[1].item() == 0.0


def test_fast_mask():
    from knightvision_amd.engine import RECORD_DTYPE, fast_mask
    recs = np.zeros(4, dtype=RECORD_DTYPE)
    recs["pad"] = [0, 1, 0, 3]
    assert fast_mask(recs).tolist() == [False, True, False, True]
