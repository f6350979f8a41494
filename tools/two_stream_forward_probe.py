"""Probe: two half-batch forwards on two streams against one whole-batch forward (HIP events).

    python tools/two_stream_forward_probe.py [B=2048] [iters=10] [rounds=3] [only]

Two kv_net objects with the same weights stand in for per-group workspaces. Each round times, alternating:
  single  one B-board forward per iteration on one stream
  serial  two B/2-board forwards per iteration, back to back on one stream
  pair    two B/2-board forwards per iteration, one on each of two streams, the streams joined after every
          iteration (they start each forward together)
  free    the same two chains without a join between iterations (as an engine's sim loop would run them)
  stag    free, with the second stream's chain started about half a layer late (one ~130 us memory pass), so
          that one stream's GEMM meets the other's output kernel
  free2   free, each net's GEMM grid sized for half the CUs (kv_dev_net_pair cu_share 2)
  lead1   free, the second net's GEMM of every conv waiting for the first net's (kv_dev_net_pair follow 1)
  lead2   free2 and lead1 together
with kv_net_forward_boards_legal (the MCTS leaf forward, 32 listed moves per board). Times are ms per iteration,
i.e. per B boards. lead2's outputs are compared with the single forward's bit for bit. `only` (a variant's
name) runs that variant alone, for a kernel trace of it.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knightvision_amd import _lib  # noqa: E402
from knightvision_amd.model import KVNet  # noqa: E402
from knightvision_amd.weights import pack_weights, synthetic_state_dict  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ONLY = sys.argv[4] if len(sys.argv) > 4 else None
H = B // 2
MAXM = 320

packed = pack_weights(synthetic_state_dict(42, "bn"))[0]
nets = [KVNet(0, packed), KVNet(0, packed)]
print("path_large", [n.calibration()["path_large"] for n in nets], flush=True)

g = torch.Generator().manual_seed(B)
boards = torch.randint(0, 13, (B, 64), dtype=torch.int8, generator=g).cuda()
moves = torch.randint(0, 4096, (B, MAXM), dtype=torch.int16, generator=g).cuda()
n_moves = torch.full((B,), 32, dtype=torch.int32).cuda()
halves = [(boards[:H].contiguous(), moves[:H].contiguous(), n_moves[:H].contiguous()),
          (boards[H:].contiguous(), moves[H:].contiguous(), n_moves[H:].contiguous())]
streams = [torch.cuda.Stream(), torch.cuda.Stream()]
main = torch.cuda.current_stream()
delay_buf = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")  # one read + write pass: ~130 us


def set_pair(cu_share, follow):
    _lib.check(_lib.lib().kv_dev_net_pair(nets[0].h, nets[1].h, cu_share, follow), "kv_dev_net_pair")


def single(n):
    for _ in range(n):
        out = nets[0].forward_boards_legal(boards, moves, n_moves)
    return out


def serial(n):
    for _ in range(n):
        out = [nets[0].forward_boards_legal(*h) for h in halves]
    return out


def pair(n):
    for _ in range(n):
        out = []
        for s, net, h in zip(streams, nets, halves):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                out.append(net.forward_boards_legal(*h))
        for s in streams:
            main.wait_stream(s)
    return out


def free(n, stagger=False, cu_share=1, follow=0):
    set_pair(cu_share, follow)
    for s in streams:
        s.wait_stream(main)
    if stagger:
        with torch.cuda.stream(streams[1]):
            delay_buf.add_(1.0)
    for _ in range(n):
        out = []
        for s, net, h in zip(streams, nets, halves):
            with torch.cuda.stream(s):
                out.append(net.forward_boards_legal(*h))
    for s in streams:
        main.wait_stream(s)
    set_pair(1, 0)
    return out


def stag(n):
    return free(n, True)


def free2(n):
    return free(n, cu_share=2)


def lead1(n):
    return free(n, follow=1)


def lead2(n):
    return free(n, cu_share=2, follow=1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn(ITERS)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


VARIANTS = [(f.__name__, f) for f in (single, serial, pair, free, stag, free2, lead1, lead2) if ONLY in (None, f.__name__)]
for _, fn in VARIANTS:  # warm-up: workspaces, code objects
    fn(3)
torch.cuda.synchronize()

if not ONLY:
    ref_l, ref_v = single(1)
    out = lead2(1)
    torch.cuda.synchronize()
    same = all(torch.equal(ref_l[i * H:(i + 1) * H], out[i][0]) and torch.equal(ref_v[i * H:(i + 1) * H], out[i][1])
               for i in range(2))
    print(f"lead2 == single bit for bit: {same}", flush=True)

res = {n: [] for n, _ in VARIANTS}
for r in range(ROUNDS):
    for name, fn in VARIANTS:
        res[name].append(timed(fn))
    print(f"round {r} B={B} ms/iter " + " ".join(f"{k} {v[-1]:.3f}" for k, v in res.items()), flush=True)
for k, v in res.items():
    print(f"{k:7s} median {np.median(v):.3f} ms  spread {max(v) - min(v):.3f} ms  ({' '.join(f'{x:.3f}' for x in v)})")
if not ONLY:
    for k in ("pair", "free", "stag", "free2", "lead1", "lead2"):
        gain = np.median(res["single"]) / np.median(res[k]) - 1
        print(f"{k} vs single: {100 * gain:+.2f} % boards/s; {k}'s spread "
              f"{100 * (max(res[k]) - min(res[k])) / np.median(res[k]):.2f} %")
