"""What an arena sim-step costs (DESIGN.md "Arena"): arena(A, A) as one stream (sim_groups 1) and as two chains
(sim_groups 2) against self-play of A on the same engine with arena = 0, at sim_groups 1 and auto, in one process
on one GPU. bench.py's timed-ply scheme: `--warmup` plies from the initial position, then `--steps` timed plies
between device synchronises (kv_run ends in one); sims/s = the timed plies' backups / their wall time. The four
variants are timed in turn, `--repeats` rounds of them, so that a drift of the box shows as spread inside every
variant, not as a difference between them. Prints one JSON line per shape and a last line with the chip's clock
under the headline GEMM (bench.py's gemm_clock).

    python tools/arena_bench.py [--shapes 2048x800,256x400] [--steps 2] [--warmup 1] [--repeats 3]
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

VARIANTS = (("selfplay_g1", False, 1), ("selfplay_auto", False, 0), ("arena_g1", True, 1), ("arena_g2", True, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x800,256x400", help="slots x sims, comma separated")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--clock-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from knightvision_amd.engine import SelfPlayEngine, sim_groups_for
    from knightvision_amd.weights import synthetic_state_dict
    assert torch.cuda.is_available(), "arena_bench needs a GPU"
    w = synthetic_state_dict(42, "init")
    for shape in args.shapes.split(","):
        slots, sims = (int(x) for x in shape.split("x"))
        engines, runs = {}, {name: [] for name, _, _ in VARIANTS}
        cap = max(1 << 16, slots * (args.warmup + args.repeats * args.steps + 8))
        for name, arena, groups in VARIANTS:  # every engine is set up and warmed before any is timed
            eng = SelfPlayEngine(w, opponent=w if arena else None, slots=slots, n_games=1 << 40, seed=42, sims=sims,
                                 sim_groups=groups, record_cap=cap, device=args.device)
            eng.run(args.warmup)
            engines[name] = eng
        for _ in range(args.repeats):
            for name, _, _ in VARIANTS:
                eng = engines[name]
                s0 = eng.stats()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(args.steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                s1 = eng.stats()
                runs[name].append({"sims_per_s": (s1["sims"] - s0["sims"]) / dt,
                                   "ply_ms": dt * 1e3 / args.steps,
                                   "leaf_batch_rows": s1["leaf_batch_rows"] - s0["leaf_batch_rows"],
                                   "arena_rows": [a - b for a, b in zip(s1["arena_rows"], s0["arena_rows"])]})
                print(f"arena_bench: {slots}x{sims} {name} {dt * 1e3 / args.steps:.1f} ms/ply", file=sys.stderr,
                      flush=True)
        out = {"slots": slots, "sims": sims, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
               "nn_path": engines["arena_g1"].calibration()["path_large"], "variants": {}}
        for name, arena, groups in VARIANTS:
            r = runs[name]
            rate = [x["sims_per_s"] for x in r]
            out["variants"][name] = {
                "sim_groups": sim_groups_for(slots, sims, groups, arena=arena),
                "sims_per_s_median": statistics.median(rate), "sims_per_s_min": min(rate), "sims_per_s_max": max(rate),
                "ply_ms_median": statistics.median(x["ply_ms"] for x in r),
                "ply_ms_all": [round(x["ply_ms"], 2) for x in r],
                "leaf_batch_rows": r[-1]["leaf_batch_rows"], "arena_rows": r[-1]["arena_rows"]}
            engines[name].close()
        v = out["variants"]
        base = v["selfplay_g1"]["sims_per_s_median"]
        out["ratio_to_selfplay_g1"] = {k: v[k]["sims_per_s_median"] / base for k in v}
        out["arena_g2_over_g1"] = v["arena_g2"]["sims_per_s_median"] / v["arena_g1"]["sims_per_s_median"]
        print(json.dumps(out), flush=True)
    from bench import gemm_clock
    print(json.dumps({"gemm_clock": gemm_clock(args.device, 2048, args.clock_seconds, 3)}), flush=True)


if __name__ == "__main__":
    main()
