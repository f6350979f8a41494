"""The learn loop's policy_target="visits" on one GPU: self-play keeps the root
move words beside the visit counts, the dataset carries the sparse targets,
the update step trains on them through the fused policy loss -- and the
default ("move", the reference's loss) is bit for bit what it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def fresh_model():
    from knightvision_amd.model import ChessNet
    from knightvision_amd.weights import synthetic_state_dict
    torch.manual_seed(0)
    m = ChessNet()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(42, "bn").items()})
    return m


@pytest.fixture(scope="module")
def shard():
    from knightvision_amd.learn import selfplay_shard
    m = fresh_model().to(DEV).eval()
    return selfplay_shard(m, 8, 0, DEV, sims=16, max_moves=12, slots=8, policy_targets=True)


def test_shard_returns_four_aligned_arrays(shard):
    from knightvision_amd import _lib
    recs, games, visits, moves = shard
    n = len(recs)
    assert n > 0 and len(games) == 8
    assert visits.dtype == np.uint16 and moves.dtype == np.uint16
    assert visits.shape == (n, _lib.MAXM) == moves.shape
    assert np.array_equal(visits == 0xffff, moves == 0xffff)  # the same legal-move prefix, row for row
    counts = np.where(visits == 0xffff, 0, visits).sum(1)
    assert (counts == 16).all()
    idx = (moves.astype(np.int64) & 63) * 64 + ((moves.astype(np.int64) >> 6) & 63)
    played = (idx == recs["move"][:, None].astype(np.int64)) & (visits != 0xffff) & (visits > 0)
    assert played.any(1).all()  # the move played was visited


def test_loop_trains_on_visits():
    from knightvision_amd.learn import reinforcement_loop
    m = fresh_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    stats = reinforcement_loop(m, iterations=2, games_per_iter=8, device=DEV, epochs=1, batch_size=64, max_moves=12,
                               slots=8, sims=16, policy_target="visits", log=None)
    assert stats[0]["records"] > 0
    assert stats[1]["optimizer_steps"] > 0
    assert np.isfinite(stats[1]["train_loss"]) and np.isfinite(stats[1]["val_loss"])
    assert all(s["policy_target"] == "visits" for s in stats)
    after = m.state_dict()
    assert any(not torch.equal(before[k].cpu(), after[k].cpu()) for k in before if "weight" in k)


def test_batch_loss_equals_the_dense_restatement(shard):
    """batch_loss with targets (amp on: fp16 logits, the HIP kernel) against the dense torch restatement on the
    same logits: each loss within 4 x the fp32 restatement's own error against fp64 + 1e-6 max(1, |ref|)."""
    from knightvision_amd import train as T
    from knightvision_amd.learn import extend_dataset
    from knightvision_amd.train_ops import policy_loss_dense
    recs, games, visits, moves = shard
    data = extend_dataset(None, recs, games, torch.device(DEV), pi=(visits, moves), policy_targets=True)
    assert len(data) == 4 and len(data[3]) == data[0].shape[0] >= 64
    b = next(iter(T.batches(*data[:3], 64, True, torch.Generator().manual_seed(1), targets=data[3])))
    assert b.rows.numel() == 64
    m = fresh_model().to(DEV).train()
    loss, lp, lv, ent, pol = T.batch_loss(m, b, entropy_coef=0.01, amp=True)
    assert pol.dtype == torch.float16 and pol.shape == (64, 4096)  # the fused path ran
    z = pol.detach()
    ce64, ent64 = policy_loss_dense(z, b.targets, b.rows, dtype=torch.float64)
    ce32, ent32 = policy_loss_dense(z, b.targets, b.rows)
    ref = {"policy": ce64.mean(), "entropy": ent64.mean()}
    f32 = {"policy": ce32.mean().double(), "entropy": ent32.mean().double()}
    ref["loss"] = ref["policy"] + lv.detach().double() - 0.01 * ref["entropy"]
    f32["loss"] = (ce32.mean() + lv.detach() - 0.01 * ent32.mean()).double()
    got = {"policy": lp, "entropy": ent, "loss": loss}
    for k in ref:
        err = abs(float(got[k].detach().double() - ref[k]))
        tol = 4 * abs(float(f32[k] - ref[k])) + 1e-6 * max(1.0, abs(float(ref[k])))
        print(f"{k}: fused {float(got[k].detach()):.9f} ref64 {float(ref[k]):.9f} err {err:.3e} tol {tol:.3e}")
        assert err <= tol, k
    loss.backward()  # the gradient reaches the network through the kernel's backward
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)


def test_default_target_is_unchanged():
    """policy_target="move" is the loop without the argument, bit for bit."""
    from knightvision_amd.learn import reinforcement_loop
    kw = dict(iterations=2, games_per_iter=8, device=DEV, epochs=1, batch_size=64, max_moves=12, slots=8, log=None)
    a = reinforcement_loop(fresh_model(), **kw)
    b = reinforcement_loop(fresh_model(), policy_target="move", **kw)
    assert a[1]["optimizer_steps"] > 0 and a[1]["train_loss"] == b[1]["train_loss"]
    assert a[1]["val_loss"] == b[1]["val_loss"] and a[1]["records"] == b[1]["records"]
    assert b[0]["policy_target"] == "move" == a[0]["policy_target"]
