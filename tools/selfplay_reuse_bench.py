"""MCTS self-play with and without carried subtrees (kv_config.reuse_tree, DESIGN.md "Carried subtrees in
self-play"): the same games (same seeds, same weights) played by an engine of either kind, the two alternating
inside one process so that both see the same clocks.

Legs, each a child process of its own under its own time limit (a leg that fails or runs out of time ends
the run: nothing more is started on the GPU after it): c2-init, c2-peaked (256 games x 400 sims, 12 plies),
c3-init, c3-peaked (2,048 games x 800 sims, 6 plies). Per leg `--reps` repeats of (reuse off, reuse on); the
first ply of every run is warm-up (it carries nothing: both kinds search a fresh root) and is not timed.
Prints one JSON line per run -- ms per ply, new backups per second, root visits per second (plies x sims / s),
leaf batch rows per ply, the kept share of the root visits -- and one summary line per leg with the medians
and the off runs' own spread.

    python tools/selfplay_reuse_bench.py [--legs c2-init,c2-peaked,c3-init,c3-peaked] [--reps 3]
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
SHAPES = {"c2": (256, 400, 12), "c3": (2048, 800, 6)}  # games (= slots), sims, plies


def run_once(sd, slots, sims, plies, reuse):
    from knightvision_amd.engine import SelfPlayEngine
    with SelfPlayEngine(sd, slots=slots, n_games=slots, seed=42, sims=sims, c_puct=1.5, reuse_tree=reuse) as eng:
        eng.run(1)
        a = eng.stats()
        t0 = time.perf_counter()
        eng.run(plies - 1)
        s = time.perf_counter() - t0
        b = eng.stats()
    d = {k: b[k] - a[k] for k in ("plies", "sims", "sims_kept", "leaf_batch_rows", "steps")}
    return {"reuse": int(reuse), "steps": d["steps"], "ms_per_ply": round(s * 1e3 / d["steps"], 3),
            "backups_per_s": round(d["sims"] / s, 1), "root_visits_per_s": round(d["plies"] * sims / s, 1),
            "leaf_batch_rows_per_ply": round(d["leaf_batch_rows"] / d["steps"], 1),
            "kept_share": round(d["sims_kept"] / max(d["plies"] * sims, 1), 4), "nn_path": b["dom_kernel"]}


def leg(name, reps):
    from knightvision_amd.weights import synthetic_state_dict
    shape, variant = name.split("-")
    slots, sims, plies = SHAPES[shape]
    sd = synthetic_state_dict(42, variant)
    runs = {0: [], 1: []}
    for rep in range(reps):
        for reuse in (False, True):
            r = run_once(sd, slots, sims, plies, reuse)
            runs[r["reuse"]].append(r)
            print(json.dumps(dict(r, leg=name, rep=rep)), flush=True)
    med = lambda k, key: statistics.median(r[key] for r in runs[k])  # noqa: E731
    off = [r["ms_per_ply"] for r in runs[0]]
    print(json.dumps({"leg": name, "summary": True, "games": slots, "sims": sims, "timed_plies": plies - 1,
                      "reps": reps, "ms_per_ply_off": med(0, "ms_per_ply"), "ms_per_ply_on": med(1, "ms_per_ply"),
                      "off_spread_ms": round(max(off) - min(off), 3),
                      "speedup": round(med(0, "ms_per_ply") / med(1, "ms_per_ply"), 4),
                      "root_visits_per_s_off": med(0, "root_visits_per_s"),
                      "root_visits_per_s_on": med(1, "root_visits_per_s"),
                      "backups_per_s_off": med(0, "backups_per_s"), "backups_per_s_on": med(1, "backups_per_s"),
                      "rows_per_ply_off": med(0, "leaf_batch_rows_per_ply"),
                      "rows_per_ply_on": med(1, "leaf_batch_rows_per_ply"),
                      "rows_saved_share": round(1.0 - med(1, "leaf_batch_rows_per_ply") /
                                                med(0, "leaf_batch_rows_per_ply"), 4),
                      "kept_share": med(1, "kept_share")}), flush=True)


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
