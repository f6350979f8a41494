"""The fused soft-target policy loss (train_ops.policy_loss: kv_tr_policy_loss_f16 + its backward) against
the dense torch restatement (logits.float(), scatter of the sparse targets to [B, 4096], log_softmax, softmax,
autograd backward), forward + backward from fp16 logits [B, 4096], at 23 (an average position) and 320 (a full
move list) entries per row. HIP-event timed, the two sides alternating inside one process, median of REPS; then
one update step of the same batch size in "visits" mode for the share.

    python tools/policy_loss_bench.py [B] [REPS]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
from knightvision_amd import train as T  # noqa: E402
from knightvision_amd.policy_targets import PolicyTargets  # noqa: E402
from knightvision_amd.train_ops import policy_loss, policy_loss_dense  # noqa: E402

DEV = "cuda:0"


def make_targets(n, entries, gen):
    idx = torch.argsort(torch.rand(n, 4096, generator=gen), dim=1)[:, :entries].reshape(-1)  # distinct per row
    cnt = torch.randint(0, 800 // entries + 40, (n * entries,), generator=gen)
    off = torch.arange(n + 1, dtype=torch.int64) * entries
    return PolicyTargets(off, idx.to(torch.int16), cnt.to(torch.int16)).to(DEV)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench(B, entries, reps):
    gen = torch.Generator().manual_seed(entries)
    targets = make_targets(B, entries, gen)
    rows = torch.randperm(B, generator=gen).to(DEV)
    logits = (torch.randn(B, 4096, generator=gen) * 3).to(torch.float16).to(DEV).requires_grad_(True)
    scale = 1024.0

    def step(op):
        ce, ent = op(logits, targets, rows)
        ((ce.mean() - 0.01 * ent.mean()) * scale).backward()
        logits.grad = None

    sides = {"fused": lambda: step(policy_loss), "dense": lambda: step(policy_loss_dense)}
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for r in range(reps):
        for k in (("fused", "dense") if r % 2 == 0 else ("dense", "fused")):
            ms[k].append(timed(sides[k]))
    return {k: statistics.median(v) for k, v in ms.items()}


def update_step_ms(B, entries, iters=5):
    from knightvision_amd.model import ChessNet
    from knightvision_amd.weights import synthetic_state_dict
    gen = torch.Generator().manual_seed(1)
    m = ChessNet().to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(42, "init").items()})
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    scaler = T.make_scaler(DEV)
    x = torch.randint(0, 2, (B, 12, 8, 8), generator=gen).float().to(DEV)
    b = T.Batch(x, torch.randint(0, 4096, (B,), generator=gen).to(DEV), (torch.rand(B, generator=gen) * 2 - 1).to(DEV),
                make_targets(B, entries, gen), torch.randperm(B, generator=gen).to(DEV))

    def one():
        loss = T.batch_loss(m, b)[0]
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()

    one()
    one()
    torch.cuda.synchronize()
    return statistics.median(timed(one) for _ in range(iters))


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    out = {"B": B, "reps": reps}
    for entries in (23, 320):
        r = bench(B, entries, reps)
        out[f"entries_{entries}"] = r
        print(f"B={B} entries/row={entries:3d}: fused {r['fused']:.3f} ms  dense torch {r['dense']:.3f} ms  "
              f"(dense / fused = {r['dense'] / r['fused']:.2f})", flush=True)
    step = update_step_ms(B, 23)
    out["update_step_ms"] = step
    for k in ("fused", "dense"):
        print(f"update step B={B} (visits mode, 23 entries/row): {step:.1f} ms; the {k} loss is "
              f"{100 * out['entries_23'][k] / step:.2f} % of it", flush=True)
    print(json.dumps(out))
