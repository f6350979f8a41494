"""MCTS self-play with and without forced playouts and policy target pruning (kv_config.forced_k, DESIGN.md "Forced
playouts and policy target pruning"): the same games (same seeds, same weights) played by an engine with forced_k = 0
and by one with forced_k = 2, the two alternating inside one process so that both see the same clocks.

Legs, each a child process of its own under its own time limit (a leg that fails or runs out of time ends the run:
nothing more is started on the GPU after it): c2-init, c2-peaked (256 games x 400 sims, 9 ply-steps), c3-init,
c3-peaked (2,048 games x 800 sims, 5 ply-steps). Per leg `--reps` repeats of (off, on); the first ply-step of every
run is warm-up and is not timed, as in tools/pcr_bench.py, whose feature-off runs on another build are therefore this
tool's off runs on that build. Prints one JSON line per run -- ms per ply-step, backups (sims) per second, the share
of the root visits the pruning took out of the targets, the share of plies whose move is not the first maximum of the
raw counts (with forced_k = 0: what the tau = 1 draw alone does), forced descents per ply -- and one summary line per
leg with the medians and the off runs' own max - min spread, the margin a difference has to exceed to be stated as
one.

    python tools/forced_bench.py [--legs c2-init,c2-peaked,c3-init,c3-peaked] [--reps 3] [--k 2]
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


def pick_share(recs, visits, words):
    """The share of plies whose move is not the first maximum of the raw root counts."""
    import numpy as np
    top = np.argmax(visits, axis=1)  # (-1 padding never wins)
    w = words[np.arange(len(recs)), top].astype(np.int64)
    return float(((w & 63) * 64 + ((w >> 6) & 63) != recs["move"]).mean()) if len(recs) else 0.0


def run_once(sd, slots, sims, plies, k):
    from knightvision_amd.engine import SelfPlayEngine
    with SelfPlayEngine(sd, slots=slots, n_games=slots, seed=42, sims=sims, c_puct=1.5, forced_k=k,
                        keep_root_moves=True) as eng:
        eng.run(1)
        a = eng.stats()
        t0 = time.perf_counter()
        eng.run(plies - 1)
        s = time.perf_counter() - t0
        b = eng.stats()
        share = pick_share(eng.records(), eng.root_visits(), eng.root_moves())
    d = {key: b[key] - a[key] for key in ("plies", "sims", "steps", "forced_descents", "visits_pruned")}
    return {"forced_k": k, "steps": d["steps"], "ms_per_ply_step": round(s * 1e3 / d["steps"], 3),
            "sims_per_s": round(d["sims"] / s, 1), "plies_per_s": round(d["plies"] / s, 1),
            "pruned_share": round(b["visits_pruned"] / max(b["sims"], 1), 4),
            "pick_not_raw_top_share": round(share, 4),
            "forced_descents_per_ply": round(d["forced_descents"] / max(d["plies"], 1), 2), "nn_path": b["dom_kernel"]}


def leg(name, reps, k):
    from knightvision_amd.weights import synthetic_state_dict
    shape, variant = name.split("-")
    slots, sims, plies = SHAPES[shape]
    sd = synthetic_state_dict(42, variant)
    runs = {0: [], 1: []}
    for rep in range(reps):
        for on in (0, 1):
            r = run_once(sd, slots, sims, plies, k if on else 0.0)
            runs[on].append(r)
            print(json.dumps(dict(r, leg=name, rep=rep)), flush=True)
    med = lambda x, key: statistics.median(r[key] for r in runs[x])  # noqa: E731
    off = [r["ms_per_ply_step"] for r in runs[0]]
    on = [r["ms_per_ply_step"] for r in runs[1]]
    print(json.dumps({"leg": name, "summary": True, "games": slots, "sims": sims, "forced_k": k,
                      "timed_ply_steps": plies - 1, "reps": reps,
                      "ms_per_ply_step_off": med(0, "ms_per_ply_step"), "ms_per_ply_step_on": med(1, "ms_per_ply_step"),
                      "off_spread_ms": round(max(off) - min(off), 3), "on_spread_ms": round(max(on) - min(on), 3),
                      "on_over_off": round(med(1, "ms_per_ply_step") / med(0, "ms_per_ply_step"), 4),
                      "sims_per_s_off": med(0, "sims_per_s"), "sims_per_s_on": med(1, "sims_per_s"),
                      "pruned_share_on": med(1, "pruned_share"),
                      "pick_not_raw_top_share_off": med(0, "pick_not_raw_top_share"),
                      "pick_not_raw_top_share_on": med(1, "pick_not_raw_top_share"),
                      "forced_descents_per_ply_on": med(1, "forced_descents_per_ply")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c2-init,c2-peaked,c3-init,c3-peaked")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--leg", help="run this leg in this process (what the driver starts)")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.reps, a.k)
        return 0
    for name in a.legs.split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(a.reps),
                                 "--k", str(a.k)], timeout=LIMIT).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": name, "error": f"time limit of {LIMIT} s"}), flush=True)
            return 1
        if rc != 0:
            print(json.dumps({"leg": name, "error": f"exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
