"""What several leaves per game buy (DESIGN.md "Several leaves per game in self-play"): self-play and an arena A
against A at kv_config.leaves in {1, 2, 4, 8, 16}, every engine shape's variants in one process on one GPU.
Random-init weights, the AUTO path, sample_plies = -1. tools/arena_bench.py's timed-ply scheme: `--warmup` plies
from the initial position, then `--steps` timed plies between device synchronises; the variants of a shape are
timed in turn, `--repeats` rounds of them, so that a drift of the box shows as spread inside every variant. Per
shape one JSON line: per L the median ms/ply and sims/s, the sim-steps per ply, the rows per sim-step and the
share of the leaf-batch rows that carried a pending leaf, each also as a ratio to L = 1 of the same shape. With
--match N a last line has the score of an N-game match of the weights against themselves at --match-leaves for both
sides (no hash evaluator; the first 8 plies drawn). The last line is the chip's clock under the headline GEMM.

    python tools/leaves_bench.py [--selfplay 32x800,64x800,256x800,256x400] [--arena 64x800] [--leaves 1,2,4,8,16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--selfplay", default="32x800,64x800,256x800,256x400", help="slots x sims, comma separated")
    ap.add_argument("--arena", default="64x800", help="slots x sims of the arena A against A, comma separated")
    ap.add_argument("--leaves", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--match", type=int, default=0, help="games of the match at --match-leaves (0: none)")
    ap.add_argument("--match-leaves", type=int, default=8)
    ap.add_argument("--match-sims", type=int, default=200)
    ap.add_argument("--match-max-moves", type=int, default=120)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--clock-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from knightvision_amd.engine import SelfPlayEngine
    from knightvision_amd.weights import synthetic_state_dict
    assert torch.cuda.is_available(), "leaves_bench needs a GPU"
    w = synthetic_state_dict(42, "init")
    ls = [int(x) for x in args.leaves.split(",")]
    assert ls[0] == 1, "the ratios are to L = 1, which comes first"
    shapes = [(s, False) for s in args.selfplay.split(",") if s] + [(s, True) for s in args.arena.split(",") if s]
    for shape, arena in shapes:
        slots, sims = (int(x) for x in shape.split("x"))
        engines, runs = {}, {L: [] for L in ls}
        cap = max(1 << 16, slots * (args.warmup + args.repeats * args.steps + 8))
        for L in ls:  # every engine is set up and warmed before any is timed
            eng = SelfPlayEngine(w, opponent=w if arena else None, slots=slots, n_games=1 << 40, seed=42, sims=sims,
                                 leaves=L, sample_plies=-1, record_cap=cap, device=args.device)
            eng.run(args.warmup)
            engines[L] = eng
        for _ in range(args.repeats):
            for L in ls:
                eng = engines[L]
                s0 = eng.stats()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(args.steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                s1 = eng.stats()
                d = {k: s1[k] - s0[k] for k in ("sims", "sim_steps", "leaf_batch_rows", "leaf_rows_pending")}
                runs[L].append({"sims_per_s": d["sims"] / dt, "ply_ms": dt * 1e3 / args.steps,
                                "steps_per_ply": d["sim_steps"] / args.steps,
                                "rows_per_step": d["leaf_batch_rows"] / max(d["sim_steps"], 1),
                                "pending_share": d["leaf_rows_pending"] / max(d["leaf_batch_rows"], 1)})
                print(f"leaves_bench: {'arena' if arena else 'selfplay'} {slots}x{sims} L={L} "
                      f"{dt * 1e3 / args.steps:.1f} ms/ply", file=sys.stderr, flush=True)
        out = {"engine": "arena" if arena else "selfplay", "slots": slots, "sims": sims, "steps": args.steps,
               "warmup": args.warmup, "repeats": args.repeats, "nn_path": engines[1].calibration()["path_large"],
               "leaves": {}}
        for L in ls:
            r = runs[L]
            out["leaves"][L] = {k: statistics.median(x[k] for x in r) for k in r[0]}
            out["leaves"][L]["ply_ms_all"] = [round(x["ply_ms"], 2) for x in r]
            engines[L].close()
        base = out["leaves"][1]
        out["ratio_to_L1"] = {L: {k: out["leaves"][L][k] / base[k] for k in ("ply_ms", "sims_per_s", "steps_per_ply",
                                                                             "rows_per_step", "pending_share")}
                              for L in ls}
        print(json.dumps(out), flush=True)
    if args.match > 0:
        from knightvision_amd import arena as AR
        r = AR.play_match(w, w, args.match, sims=args.match_sims, slots=min(256, args.match), seed=42,
                          max_moves=args.match_max_moves, leaves=args.match_leaves, device=args.device)
        half = 1.96 * (max(r["score"] * (1 - r["score"]), 1e-9) / r["games"]) ** 0.5  # (draws make it narrower)
        print(json.dumps({"match": {"games": r["games"], "leaves": args.match_leaves, "sims": args.match_sims,
                                    "max_moves": args.match_max_moves, "wins": r["wins"], "draws": r["draws"],
                                    "losses": r["losses"], "score": r["score"], "score_ci95_halfwidth_upper": half,
                                    "reasons": r["reasons"], "sim_steps": r["stats"]["sim_steps"],
                                    "plies": r["stats"]["plies"]}}), flush=True)
    from bench import gemm_clock
    print(json.dumps({"gemm_clock": gemm_clock(args.device, 2048, args.clock_seconds, 3)}), flush=True)


if __name__ == "__main__":
    main()
