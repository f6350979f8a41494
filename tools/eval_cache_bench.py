"""What the evaluation cache buys (DESIGN.md "Evaluation cache"): kv_config.eval_cache off against on, the two
engines of a shape alternating in one process on one GPU, after tools/leaves_bench.py. The engines play the same
games byte for byte (checked on the records at the end), so both time the same search.

Two timed phases per engine: plies 1 .. --plies from the initial position -- all games share their opening, which
flatters a cache -- and, after --skip untimed plies, plies skip + 1 .. skip + plies. A phase is timed in chunks of
--chunk plies, off and on in turn, so that a drift of the box shows as spread inside both. Self-play draws every
move (sample_plies 0, root noise on); the arena is A against A with arena.play_match's defaults (no noise, the first
8 plies drawn). Per shape and weight set one JSON line: per phase and variant the median ms/ply with every chunk's,
sims/s, sim-steps per ply, network rows per sim-step, and for the cache the hit rate, the stores and the table's
bytes.

    python tools/eval_cache_bench.py [--selfplay 256x800,64x800] [--arena 64x800] [--leaves 8] [--entries 1048576]
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
    ap.add_argument("--selfplay", default="256x800,64x800", help="slots x sims, comma separated")
    ap.add_argument("--arena", default="64x800", help="slots x sims of the arena A against A, comma separated")
    ap.add_argument("--weights", default="init,peaked")
    ap.add_argument("--leaves", type=int, default=8)
    ap.add_argument("--entries", type=int, default=1 << 20, help="kv_config.eval_cache of the cached engine")
    ap.add_argument("--plies", type=int, default=6, help="timed plies per phase")
    ap.add_argument("--skip", type=int, default=20, help="plies played before the second phase")
    ap.add_argument("--chunk", type=int, default=2, help="plies per timed chunk")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch
    from knightvision_amd import _lib
    from knightvision_amd.engine import SelfPlayEngine
    from knightvision_amd.weights import synthetic_state_dict
    assert torch.cuda.is_available(), "eval_cache_bench needs a GPU"
    assert args.plies % args.chunk == 0 and args.skip >= args.plies
    shapes = [(s, False) for s in args.selfplay.split(",") if s] + [(s, True) for s in args.arena.split(",") if s]
    keys = ("sims", "sim_steps", "leaf_batch_rows", "leaf_rows_pending", "cache_probes", "cache_hits", "cache_stores")
    for variant in args.weights.split(","):
        w = synthetic_state_dict(42, variant)
        for shape, arena in shapes:
            slots, sims = (int(x) for x in shape.split("x"))
            kw = dict(eps=0.0, sample_plies=8) if arena else {}
            engines = {name: SelfPlayEngine(w, opponent=w if arena else None, slots=slots, n_games=1 << 40, seed=42,
                                            sims=sims, leaves=args.leaves, eval_cache=entries, device=args.device,
                                            record_cap=max(1 << 16, slots * (args.skip + args.plies + 8)), **kw)
                       for name, entries in (("off", 0), ("on", args.entries))}
            phases = {}
            for phase, before in (("opening", 0), ("midgame", args.skip - args.plies)):
                for eng in engines.values():
                    if before:
                        eng.run(before)
                runs = {name: [] for name in engines}
                for _ in range(args.plies // args.chunk):
                    for name, eng in engines.items():
                        s0 = eng.stats()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        eng.run(args.chunk)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        s1 = eng.stats()
                        runs[name].append(dict({k: s1[k] - s0[k] for k in keys}, s=dt))
                        print(f"eval_cache_bench: {variant} {'arena' if arena else 'selfplay'} {shape} {phase} {name} "
                              f"{dt * 1e3 / args.chunk:.1f} ms/ply", file=sys.stderr, flush=True)
                out = {}
                for name, r in runs.items():
                    tot = {k: sum(x[k] for x in r) for k in keys + ("s",)}
                    ms = [x["s"] * 1e3 / args.chunk for x in r]
                    out[name] = {"ply_ms": statistics.median(ms), "ply_ms_all": [round(x, 2) for x in ms],
                                 "sims_per_s": tot["sims"] / tot["s"], "steps_per_ply": tot["sim_steps"] / args.plies,
                                 "rows_per_step": tot["leaf_batch_rows"] / max(tot["sim_steps"], 1),
                                 "pending_per_step": tot["leaf_rows_pending"] / max(tot["sim_steps"], 1)}
                    if name == "on":
                        out[name].update(hit_rate=tot["cache_hits"] / max(tot["cache_probes"], 1),
                                         stores=tot["cache_stores"])
                off_ms = out["off"]["ply_ms_all"]
                out["on_over_off_ply_ms"] = out["on"]["ply_ms"] / out["off"]["ply_ms"]
                out["off_spread_ms"] = max(off_ms) - min(off_ms)
                phases[phase] = out
            same = engines["off"].records().tobytes() == engines["on"].records().tobytes()
            nets = 2 if arena else 1
            line = {"engine": "arena" if arena else "selfplay", "weights": variant, "slots": slots, "sims": sims,
                    "leaves": args.leaves, "eval_cache": args.entries, "tables": nets,
                    "table_bytes": nets * args.entries * (_lib.CACHE_ENTRY_BYTES + 4),
                    "nn_path": engines["off"].calibration()["path_large"], "same_records": same, "phases": phases}
            for eng in engines.values():
                eng.close()
            print(json.dumps(line), flush=True)
            assert same, "the cached engine played other games"


if __name__ == "__main__":
    main()
