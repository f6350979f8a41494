"""Wall time of kv_search (engine.PositionSearch) with the real network on random-init weights.

Legs, each a child process of its own under its own time limit (a leg that fails or runs out of time ends
the run: nothing more is started on the GPU after it):
  one    one position x 800 sims at L = 1, 8, 32, 64 in one process on one engine (the L = 32 / L = 1 ratio)
  many   256 positions x 400 sims at L = 1 (self-play's C2 shape without the move choice)
  mid    17 positions x 800 sims at L = 8
  agree  how often `best` at L = 8 and L = 32 equals L = 1's: 18 positions of oracle hash games, 800 sims,
         peaked weights (reported, not a pass/fail figure)
Prints one JSON line per measurement.

    python tools/search_bench.py [--legs one,many,mid,agree] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LIMITS = {"one": 240, "many": 240, "mid": 180, "agree": 300}  # seconds per leg


def _game_states(n):
    """n distinct positions: the start position and the ones after its first legal moves."""
    import numpy as np
    from knightvision_amd import _lib
    import ctypes as C
    from knightvision_amd.chess_engine import GameState
    st0 = GameState()._state()
    L = _lib.lib()
    out = [st0]
    k = 0
    while len(out) < n:
        base = out[k // 20].copy()[None]
        idx = np.array([k % 20], dtype=np.int32)
        _lib.check(L.kv_dev_make_move(0, base.ctypes.data_as(C.POINTER(C.c_int8)),
                                      idx.ctypes.data_as(C.POINTER(C.c_int)), 1), "kv_dev_make_move")
        out.append(base[0])
        k += 1
    return np.stack(out[:n])


def _time(ps, states, sims, leaves, reps):
    ps.search(states, sims, leaves=leaves)  # warm-up: workspaces, code objects
    best, rows = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        rows = ps.search(states, sims, leaves=leaves)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    n = len(states)
    return {"positions": n, "sims": sims, "leaves": leaves, "ms_per_search": round(best * 1e3, 3),
            "sims_per_s": round(n * sims / best, 1), "steps": int(rows["steps"].max()),
            "nn_rows_per_position": round(float(rows["nn_rows"].mean()), 1), "reps": reps}


def leg(name, reps):
    import numpy as np
    from knightvision_amd.engine import PositionSearch
    from knightvision_amd.weights import synthetic_state_dict
    if name == "one":
        with PositionSearch(synthetic_state_dict(42, "init"), max_positions=1, max_sims=800) as ps:
            st = _game_states(1)
            res = {L: _time(ps, st, 800, L, reps) for L in (1, 8, 32, 64)}
            for L, r in res.items():
                r["leg"] = "one"
                r["speedup_vs_l1"] = round(res[1]["ms_per_search"] / r["ms_per_search"], 2)
                print(json.dumps(r), flush=True)
    elif name == "many":
        with PositionSearch(synthetic_state_dict(42, "init"), max_positions=256, max_sims=400) as ps:
            print(json.dumps(dict(_time(ps, _game_states(256), 400, 1, reps), leg="many")), flush=True)
    elif name == "mid":
        with PositionSearch(synthetic_state_dict(42, "init"), max_positions=17, max_sims=800) as ps:
            print(json.dumps(dict(_time(ps, _game_states(17), 800, 8, reps), leg="mid")), flush=True)
    elif name == "agree":
        from tests import _mcts_search as S  # the tests' 18 positions
        states = np.stack([s for s, _ in S.hash_positions()])
        with PositionSearch(synthetic_state_dict(42, "peaked"), max_positions=len(states), max_sims=800) as ps:
            base = ps.search(states, 800, leaves=1)
            for L in (8, 32):
                r = ps.search(states, 800, leaves=L)
                print(json.dumps({"leg": "agree", "positions": len(states), "sims": 800, "leaves": L,
                                  "best_equals_l1": int((r["best"] == base["best"]).sum())}), flush=True)
    else:
        raise SystemExit(f"unknown leg {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="one,many,mid,agree")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", help="run this leg in this process (what the driver starts)")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.reps)
        return 0
    for name in a.legs.split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(a.reps)],
                                timeout=LIMITS[name]).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": name, "error": f"time limit of {LIMITS[name]} s"}), flush=True)
            return 1
        if rc != 0:
            print(json.dumps({"leg": name, "error": f"exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
