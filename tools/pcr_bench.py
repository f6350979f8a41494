"""MCTS self-play with and without playout cap randomization (kv_config.fast_sims, DESIGN.md "Playout cap
randomization"): the same games (same seeds, same weights) played by an engine with the feature off and by one
with it on, the two alternating inside one process so that both see the same clocks.

Legs, each a child process of its own under its own time limit (a leg that fails or runs out of time ends
the run: nothing more is started on the GPU after it): c2-init, c2-peaked (256 games x 400 sims, 9 ply-steps),
c3-init, c3-peaked (2,048 games x 800 sims, 5 ply-steps), at fast_sims = sims / 8 and full_prob 0.25. Per leg
`--reps` repeats of (off, on); the first ply-step of every run is warm-up and is not timed. Prints one JSON line
per run -- ms per ply-step, plies per second, full plies per second (the policy targets), leaf batch rows per
ply-step, the full share of the plies -- and one summary line per leg with the medians and the off runs' own
max - min spread, the margin a difference has to exceed to be stated as one.

    python tools/pcr_bench.py [--legs c2-init,c2-peaked,c3-init,c3-peaked] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LIMIT = 420  # seconds per leg
SHAPES = {"c2": (256, 400, 9), "c3": (2048, 800, 5)}  # games (= slots), sims, ply-steps
FULL_PROB = 0.25


def run_once(sd, slots, sims, plies, fast):
    from knightvision_amd.engine import SelfPlayEngine
    with SelfPlayEngine(sd, slots=slots, n_games=slots, seed=42, sims=sims, c_puct=1.5, fast_sims=fast,
                        full_prob=FULL_PROB) as eng:
        eng.run(1)
        a = eng.stats()
        t0 = time.perf_counter()
        eng.run(plies - 1)
        s = time.perf_counter() - t0
        b = eng.stats()
    d = {k: b[k] - a[k] for k in ("plies", "plies_full", "sims", "leaf_batch_rows", "steps", "sim_steps")}
    return {"fast_sims": fast, "steps": d["steps"], "ms_per_ply_step": round(s * 1e3 / d["steps"], 3),
            "plies_per_s": round(d["plies"] / s, 1), "full_plies_per_s": round(d["plies_full"] / s, 1),
            "backups_per_s": round(d["sims"] / s, 1),
            "leaf_batch_rows_per_ply_step": round(d["leaf_batch_rows"] / d["steps"], 1),
            "sim_steps_per_ply_step": round(d["sim_steps"] / d["steps"], 1),
            "full_share": round(d["plies_full"] / max(d["plies"], 1), 4), "nn_path": b["dom_kernel"]}


def leg(name, reps):
    from knightvision_amd.weights import synthetic_state_dict
    shape, variant = name.split("-")
    slots, sims, plies = SHAPES[shape]
    sd = synthetic_state_dict(42, variant)
    runs = {0: [], 1: []}
    for rep in range(reps):
        for on in (0, 1):
            r = run_once(sd, slots, sims, plies, sims // 8 if on else 0)
            runs[on].append(r)
            print(json.dumps(dict(r, leg=name, rep=rep)), flush=True)
    med = lambda k, key: statistics.median(r[key] for r in runs[k])  # noqa: E731
    off = [r["ms_per_ply_step"] for r in runs[0]]
    off_full = [r["full_plies_per_s"] for r in runs[0]]
    print(json.dumps({"leg": name, "summary": True, "games": slots, "sims": sims, "fast_sims": sims // 8,
                      "full_prob": FULL_PROB, "timed_ply_steps": plies - 1, "reps": reps,
                      "ms_per_ply_step_off": med(0, "ms_per_ply_step"), "ms_per_ply_step_on": med(1, "ms_per_ply_step"),
                      "off_spread_ms": round(max(off) - min(off), 3),
                      "ply_step_speedup": round(med(0, "ms_per_ply_step") / med(1, "ms_per_ply_step"), 4),
                      "plies_per_s_off": med(0, "plies_per_s"), "plies_per_s_on": med(1, "plies_per_s"),
                      "full_plies_per_s_off": med(0, "full_plies_per_s"),
                      "full_plies_per_s_on": med(1, "full_plies_per_s"),
                      "off_spread_full_plies_per_s": round(max(off_full) - min(off_full), 1),
                      "rows_per_ply_step_off": med(0, "leaf_batch_rows_per_ply_step"),
                      "rows_per_ply_step_on": med(1, "leaf_batch_rows_per_ply_step"),
                      "sim_steps_per_ply_step_on": med(1, "sim_steps_per_ply_step"),
                      "full_share_on": med(1, "full_share")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c2-init,c2-peaked,c3-init,c3-peaked")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", help="run this leg in this process (what the driver starts)")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.reps)
        return 0
    for name in a.legs.split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(a.reps)],
                                timeout=LIMIT).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": name, "error": f"time limit of {LIMIT} s"}), flush=True)
            return 1
        if rc != 0:
            print(json.dumps({"leg": name, "error": f"exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
