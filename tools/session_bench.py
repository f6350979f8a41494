"""One game from the start position, searched ply by ply (800 visits, L = 32, real network): a fresh
PositionSearch.search per ply against a search session that carries the played move's subtree
(advance + resume, DESIGN.md "Search sessions").

Legs, each a child process of its own under its own time limit (a leg that fails or runs out of time ends
the run: nothing more is started on the GPU after it):
  pair-init, pair-peaked    both searches on the same line (the session's best move is played), each on an
                            engine of its own: per ply the wall time and network rows of either, the kept
                            share of the visits, the advance call's own time and the tree's nodes after it
  fresh-init, fresh-peaked  the fresh search alone, playing its own best move (needs kv_search only, so it
                            also runs on a tree without sessions: the yardstick for kv_search itself)
Prints one JSON line per ply and one summary line per leg.

    python tools/session_bench.py [--legs pair-init,pair-peaked,fresh-init,fresh-peaked] [--plies 40]
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

LIMIT = 240  # seconds per leg
SIMS, LEAVES = 800, 32


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def leg(name, plies):
    from knightvision_amd.chess_engine import GameState
    from knightvision_amd.engine import PositionSearch
    from knightvision_amd.weights import synthetic_state_dict
    mode, variant = name.split("-")
    sd = synthetic_state_dict(42, variant)
    gs = GameState()
    fresh = PositionSearch(sd, max_positions=1, max_sims=SIMS)
    fresh.search(gs._state()[None], SIMS, leaves=LEAVES)  # warm-up: workspaces, code objects
    ses = None
    if mode == "pair":
        ses = PositionSearch(sd, max_positions=1, max_sims=SIMS)
        ses.search(gs._state()[None], SIMS, leaves=LEAVES)
    tot = dict(ms_fresh=0.0, rows_fresh=0, steps_fresh=0, ms_session=0.0, rows_session=0, ms_advance=0.0, kept=0)
    played = 0
    for ply in range(plies):
        valid = gs.getValidMoves()
        st = gs._state()[None]
        f, ms_f = _ms(lambda: fresh.search(st, SIMS, leaves=LEAVES)[0])
        if f["status"] != 0:
            break
        out = {"leg": name, "ply": ply, "ms_fresh": round(ms_f, 3), "rows_fresh": int(f["nn_rows"]),
               "steps_fresh": int(f["steps"])}
        tot["ms_fresh"] += ms_f
        tot["rows_fresh"] += int(f["nn_rows"])
        tot["steps_fresh"] += int(f["steps"])
        best = int(f["best"])
        if ses is not None:
            if ply == 0:
                s, ms_s = _ms(lambda: ses.search(st, SIMS, leaves=LEAVES)[0])
                kept = 0
            else:
                (rows, kp), ms_s = _ms(lambda: ses.resume(SIMS, leaves=LEAVES))
                s, kept = rows[0], int(kp[0])
            assert int(s["visits"][:s["n_moves"]].sum()) == SIMS
            assert int(s["nn_rows"]) <= SIMS - kept + (1 if kept == 0 else 0)
            best = int(s["best"])
            _, ms_a = _ms(lambda: ses.advance([best]))
            out.update(ms_session=round(ms_s, 3), rows_session=int(s["nn_rows"]), steps_session=int(s["steps"]),
                       kept=kept, kept_share=round(kept / SIMS, 3), ms_advance=round(ms_a, 3),
                       nodes_after_advance=ses.tree_size(0)[0])
            tot["ms_session"] += ms_s
            tot["rows_session"] += int(s["nn_rows"])
            tot["ms_advance"] += ms_a
            tot["kept"] += kept
        print(json.dumps(out), flush=True)
        gs.makeMove(valid[best])
        played += 1
    summary = {"leg": name, "summary": True, "plies": played, "sims": SIMS, "leaves": LEAVES,
               "ms_per_ply_fresh": round(tot["ms_fresh"] / played, 3),
               "rows_per_ply_fresh": round(tot["rows_fresh"] / played, 1),
               "ms_per_sim_step": round(tot["ms_fresh"] / tot["steps_fresh"], 3)}
    if ses is not None:
        summary.update(ms_per_ply_session=round(tot["ms_session"] / played, 3),
                       rows_per_ply_session=round(tot["rows_session"] / played, 1),
                       rows_saved_share=round(1.0 - tot["rows_session"] / tot["rows_fresh"], 3),
                       kept_share=round(tot["kept"] / (played * SIMS), 3),
                       ms_per_advance=round(tot["ms_advance"] / played, 3))
        ses.close()
    fresh.close()
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="pair-init,pair-peaked,fresh-init,fresh-peaked")
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--leg", help="run this leg in this process (what the driver starts)")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.plies)
        return 0
    for name in a.legs.split(","):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--plies", str(a.plies)],
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
