"""The reinforcement loop of scripts/learn.py (reinforcement_loop :152-209) on
one process per GPU (BASELINE configs[4]):

    for each iteration:
        train_with_validation on a 90/10 random split of the data so far (train.py:293-420: epochs of
            the update step, DDP over RCCL, validation loss, ReduceLROnPlateau, early stopping)
        self-play with the new weights (generate_self_play_data -> libkv.so engine, games sharded by rank)
        dataset.extend(new records)    (decisive-record filter of generate_self_play_data :304-310)

The dataset is optionally seeded with the reference's JSONL training data
(ChessPGNDataset, learn.py:162). Every rank holds the whole dataset on its GPU
(int8 board codes, move index, reward: 76 B per sample instead of a 3 KB plane
tensor, expanded per batch on the device), draws the same split and trains on
its round-robin shard of the train subset; DistributedDataParallel averages
the gradients with bucketed RCCL all-reduces overlapped with the backward
pass. The one data exchange is the end-of-iteration all-gather of the new
records (distributed.gather_rows, dst=None), filtered as one dataset (the
reference's global decisive filter).
The global batch is the reference's: nn.DataParallel splits one batch of
BATCH_SIZE over the GPUs (utils/model_utils.py:26-28), so each of the W ranks
trains on batch_size // W rows per micro-batch with the same accumulation
count -- W x (batch_size // W) rows per micro-batch, one optimizer step per
accumulate_steps micro-batches, as on one process. Self-play game g of iteration i has the global id
i * games_per_iter + g and the seeds SEED + id (per-game seeding).

policy_target="visits" (no reference counterpart; MCTS self-play only) trains
the policy on each record's root visit distribution instead of the move
played: the engine keeps the root move words beside the visit counts, the
dataset tuple carries them as sparse PolicyTargets (policy_targets.py) and
the update step scores them with the fused HIP loss (train_ops.policy_loss).
The default, "move", is the reference's loss.

fast_sims > 0 (no reference counterpart; MCTS self-play only) turns on playout
cap randomization (kv_config.fast_sims, DESIGN.md "Playout cap randomization"):
a ply is searched to `sims` visits with probability full_prob, else to
fast_sims. Every record gives a value target; in "visits" mode only the full
plies give a policy target (PolicyTargets.w is 0 on the fast ones). "move"
mode trains on every record as before.

forced_k > 0 (no reference counterpart; MCTS self-play only) turns on forced
playouts and policy target pruning (kv_config.forced_k, DESIGN.md "Forced
playouts and policy target pruning"): in "visits" mode the policy targets are
the pruned root counts (engine.root_targets) instead of the raw visit counts.

arena_games > 0 (no reference counterpart; the reference evaluates against
Stockfish here, learn.py:204-206): after an iteration's update the new weights
play a match against the weights the iteration started from (arena.py,
kv_config.arena) and the iteration's statistics carry the summary. Reporting
only: nothing is gated or reverted.

Not reproduced (out of the self-play path): the Stockfish
evaluation, checkpoints, Telegram and TensorBoard logging.
"""
from __future__ import annotations

import math
import os
import time

import numpy as np
import torch

from . import train as T
from .distributed import gather_rows
from .engine import SelfPlayEngine, fast_mask, packed_from
from .policy_targets import PolicyTargets
from .self_play import ALPHA, BATCH_SIZE as SELFPLAY_BATCH, EPSILON, SEED

# learn.py's configuration (:105-112) and train.py's scheduler constants (:21, :463-464)
TRAIN_EPOCHS = int(os.getenv("TRAIN_EPOCHS", "2"))
LEARN_BATCH_SIZE = int(os.getenv("BATCH_SIZE", "2048"))
LEARN_LR = float(os.getenv("LR", "1e-3"))
PATIENCE = int(os.getenv("PATIENCE", "5"))
LR_GAMMA = float(os.getenv("LR_GAMMA", "0.1"))
LR_STEP_SIZE = int(os.getenv("LR_STEP_SIZE", "10"))  # train.py:463
COSINE_T0 = int(os.getenv("COSINE_T0", "10"))        # train.py:295
VAL_FRAC = 0.1


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def selfplay_shard(model, n_games: int, iteration: int, device, *, sims=0, max_moves=None, slots=256,
                   precision="fp32", policy_targets=False, reuse_tree=False, leaves=0, eval_cache=0, fast_sims=0,
                   full_prob=0.25, forced_k=0.0):
    """This rank's share of one iteration's games, played by the HIP engine with
    the model's current weights. Returns (records, games) numpy arrays; with
    policy_targets (MCTS runs) also the root visit counts and root move words of
    every record, (records, games, visits uint16 [n, MAXM], moves uint16
    [n, MAXM]) row for row, 0xffff past each position's move list. reuse_tree (sims > 0): the engine carries
    the subtree under each move played into the next ply (kv_config.reuse_tree); every root still holds sims
    visits, so the visit targets are built as without it. leaves > 1 (sims > 0): that many descents in flight
    per game and sim-step (kv_config.leaves); eval_cache (leaves >= 2): entries of the engine's exact leaf-row cache
    (kv_config.eval_cache; 0: off), which changes no record. fast_sims > 0 (0 < fast_sims < sims): playout cap
    randomization (kv_config.fast_sims) -- a ply is searched to sims visits with probability full_prob and to
    fast_sims otherwise; the records of fast plies carry pad bit 0 (engine.fast_mask). forced_k > 0: forced playouts
    and policy target pruning (kv_config.forced_k); with policy_targets the third array is then the pruned counts
    (engine.root_targets) in place of the raw visit counts, the same layout."""
    dist, rank, world = _dist()
    dev = torch.device(device)
    ids = list(range(rank, n_games, world))
    if policy_targets and sims <= 0:
        raise ValueError("selfplay_shard: policy_targets needs the search's visit counts (sims > 0)")
    if not ids:
        return (None, None, None, None) if policy_targets else (None, None)
    base = iteration * n_games + rank
    from .self_play import batched_eval_mode
    with SelfPlayEngine(packed_from(model), slots=min(slots, len(ids)), n_games=len(ids), seed=SEED,
                        max_moves=max_moves, batch=SELFPLAY_BATCH, eps=EPSILON, alpha=ALPHA, sims=sims,
                        game_id_base=base, game_id_stride=world, device=dev.index or 0,
                        precision=precision, eval_mode=batched_eval_mode() if sims == 0 else 0,
                        keep_root_moves=bool(policy_targets), reuse_tree=bool(reuse_tree), leaves=int(leaves),
                        eval_cache=int(eval_cache), fast_sims=int(fast_sims), full_prob=float(full_prob),
                        forced_k=float(forced_k)) as eng:
        eng.run()
        selfplay_shard.last_calibration = eng.calibration()  # the conv paths these weights ran on
        selfplay_shard.last_stats = eng.stats()
        if policy_targets:
            counts = eng.root_targets() if forced_k > 0 else eng.root_visits()
            return eng.records(), eng.games(), counts.astype("uint16"), eng.root_moves()
        return eng.records(), eng.games()


def arena_shard(new_weights, old_weights, n_games: int, iteration: int, device, *, sims: int, max_moves=None,
                slots=256, precision="fp32", leaves=0, eval_cache=0) -> dict:
    """A match of `n_games` games between the new weights (player A) and the old ones (player B), the games
    sharded over the ranks by global id as selfplay_shard shards them (game g of iteration i has the id
    i * n_games + g; A plays white in the even ids). Every rank returns the same arena.summarize of all the
    ranks' games (W / D / L summed over ranks), with this rank's engine stats under "stats"."""
    from . import arena
    from .engine import GAME_DTYPE
    dist, rank, world = _dist()
    dev = torch.device(device)
    ids = list(range(rank, n_games, world))
    table, stats = np.zeros(0, dtype=GAME_DTYPE), None
    if ids:
        r = arena.play_match(new_weights, old_weights, len(ids), sims=sims, slots=min(slots, len(ids)), seed=SEED,
                             max_moves=max_moves, device=dev.index or 0, game_id_base=iteration * n_games + rank,
                             game_id_stride=world, precision=precision, leaves=leaves, eval_cache=eval_cache)
        table, stats = r["game_table"], r["stats"]
    if dist is not None and world > 1:
        rows = torch.from_numpy(table.view(np.uint8).reshape(-1, GAME_DTYPE.itemsize).copy()).to(dev)
        rows = gather_rows(rows, dst=None).cpu().numpy()
        table = np.ascontiguousarray(rows).view(GAME_DTYPE).reshape(-1)
    out = arena.summarize(table)
    out["stats"] = stats
    return out


def _max_over_ranks(n: int, dev) -> int:
    dist, _, world = _dist()
    if dist is None or world == 1:
        return n
    t = torch.tensor([n], dtype=torch.int64, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return int(t.item())


def rank_batch_size(batch_size: int, world: int) -> int:
    """Per-rank micro-batch that keeps the reference's global batch (DataParallel
    scatters one batch of `batch_size` rows over the devices)."""
    return max(1, batch_size // world)


def decisive_filter(codes, moves, rewards, targets=None):
    """generate_self_play_data (self_play.py:304-310): keep only records whose
    reward is +-1 when there are at least 10 of them (`targets`: the samples'
    PolicyTargets rows, filtered with them)."""
    dec = rewards.abs() == 1.0
    if int(dec.sum()) >= 10:
        out = codes[dec], moves[dec], rewards[dec]
        return out if targets is None else out + (targets[dec],)
    return (codes, moves, rewards) if targets is None else (codes, moves, rewards, targets)


def _gather_targets(recs, games, pi, dev, weighted=False) -> PolicyTargets:
    """This iteration's visit targets of every rank, in gather_rows' rank order (the order the samples'
    tensors take): each row's legal-move prefix (distributed.pack_pi) of the visit counts and of the move
    words crosses ranks, and the CSR is built from that compact form directly. weighted (fast_sims > 0, the
    same on every rank): the targets carry per-sample weights, 0 on the records of fast plies and 1 on the
    others, which cross ranks beside the rows' lengths."""
    if recs is not None and len(recs):
        if pi is None:
            raise ValueError("extend_dataset: policy_targets needs the records' (visits, moves) of selfplay_shard")
        keep = np.isin(recs["game_id"], games["game_id"])  # records_to_tensors' rows: the finished games'
        local = PolicyTargets.from_engine(pi[0][keep], pi[1][keep], dev,
                                          weights=1.0 - fast_mask(recs[keep]) if weighted else None)
    else:
        local = PolicyTargets.empty(dev)
    counts = local.lengths().to(torch.int16)
    if weighted:  # (length, weight) pairs: one exchange for both
        pairs = torch.stack([counts, local.weights().to(torch.int16)], 1).contiguous()
        pairs = gather_rows(pairs.view(torch.uint8).reshape(-1, 4), dst=None).to(dev).contiguous()
        pairs = pairs.view(torch.int16).reshape(-1, 2)

    def all_ranks(t):  # int16 travels as byte pairs (gloo has no int16 collectives)
        return gather_rows(t.view(torch.uint8).reshape(-1, 2), dst=None).to(dev).contiguous().view(torch.int16).reshape(-1)

    w = None
    if weighted:
        counts, w = pairs[:, 0].contiguous(), pairs[:, 1].to(torch.float32)
    else:
        counts = all_ranks(counts)
    idx, cnt = all_ranks(local.idx), all_ranks(local.cnt)
    off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(counts.to(torch.int64) & 0xffff, 0)
    return PolicyTargets(off, idx, cnt, w)


def extend_dataset(data, recs, games, dev, pi=None, policy_targets=False, weighted=False):
    """dataset.extend(generate_self_play_data(...)) for one iteration
    (learn.py:194-199): the ranks' new records are all-gathered (the one
    end-of-iteration exchange) and filtered as one dataset (the reference's
    global decisive filter); every rank appends the same union, so every rank
    holds the whole dataset (64 + 12 B per sample) and the 90/10 split below is
    the same on all of them.
    policy_targets ("visits" mode): `pi` is this rank's (visits, moves) of
    selfplay_shard, row for row with `recs` (None on a rank without games); the
    visit targets are gathered and filtered with the samples and the dataset
    tuple carries them as a fourth element, samples that came without a search
    holding their one-hot row. weighted (fast_sims > 0): the targets carry the
    per-sample policy weights (_gather_targets)."""
    if recs is not None and len(recs):
        local = T.records_to_tensors(recs, games, dev)
    else:
        local = (torch.zeros((0, 64), dtype=torch.int8, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                 torch.zeros(0, dtype=torch.float32, device=dev))
    if not policy_targets:
        union = decisive_filter(*(gather_rows(x, dst=None).to(dev) for x in local))
        return union if data is None else tuple(torch.cat([a, b]) for a, b in zip(data, union))
    union = tuple(gather_rows(x, dst=None).to(dev) for x in local)
    union = decisive_filter(*union, _gather_targets(recs, games, pi, dev, weighted))
    if data is None:
        return union
    old = data[3] if len(data) > 3 else PolicyTargets.one_hot(data[1])
    return tuple(torch.cat([a, b]) for a, b in zip(data[:3], union[:3])) + (PolicyTargets.cat([old, union[3]]),)


def split_train_val(n: int, gen: torch.Generator):
    """random_split(dataset, [int(0.9 n), n - int(0.9 n)]) (learn.py:162-165, :196-199): index tensors of the
    train and validation subsets (the generator is seeded alike on every rank)."""
    perm = torch.randperm(n, generator=gen)
    n_train = int((1.0 - VAL_FRAC) * n)
    return perm[:n_train], perm[n_train:]


def evaluate_sharded(model, data, idx, batch_size: int, dev) -> float:
    """train.evaluate (train.py:109-124) over a validation subset split round-robin over the ranks:
    sum of per-sample (CE + MSE) and the sample count all-reduced, then their ratio."""
    dist, rank, world = _dist()
    mine = idx[rank::world].to(dev)
    tot = torch.zeros(2, dtype=torch.float64, device=dev)
    if mine.numel():
        batches = list(T.batches(*(x[mine] for x in data[:3]), batch_size, False,
                                 targets=data[3][mine] if len(data) > 3 else None))
        n = sum(b.boards.shape[0] for b in batches)
        tot[0] = T.evaluate(model, batches) * n
        tot[1] = n
    if dist is not None and world > 1:
        t = tot.to(dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t)
        tot = t
    return float(tot[0] / tot[1]) if float(tot[1]) > 0 else math.inf


def train_with_validation(ddp, model, optimizer, data, epochs: int, batch_size: int, accumulate_steps: int,
                          gen: torch.Generator, split_gen: torch.Generator, dev) -> dict:
    """train.py train_with_validation (:293-420) as the learn loop calls it (TRAIN_EPOCHS = 2 <
    NUM_PGN_EPOCHS, so no self-play inside it). Per call, as the reference: a fresh GradScaler and the
    three LR schedulers in its order -- CosineAnnealingWarmRestarts(T_0=COSINE_T0, T_mult=1) (:293-297;
    constructing it resets the LR to the optimizer's initial LR, so the cosine schedule restarts every
    iteration), ReduceLROnPlateau(mode='min', factor=LR_GAMMA, patience=PATIENCE) (:298-304) and
    StepLR(LR_STEP_SIZE, LR_GAMMA) (:306-307). Per epoch one pass of _train_one_epoch over the train
    split, evaluate() on the validation split and the plateau step on its loss (_run_validation
    :198-218), early stopping after PATIENCE epochs without improvement (before the other two
    schedulers step), then cos.step(epoch + 1) and step.step() (:421-423). Checkpoints, TensorBoard
    and Telegram are not reproduced."""
    import warnings
    dist, rank, world = _dist()
    tr, va = split_train_val(int(data[0].shape[0]), split_gen)
    mine = tr[rank::world].to(dev)
    n_max = _max_over_ranks(int(mine.numel()), dev)
    scaler = T.make_scaler(dev)
    cos, plateau, step = make_lr_schedulers(optimizer)
    best, no_improve, ep, val_loss, done = math.inf, 0, None, math.inf, 0
    shard = tuple(x[mine] for x in data[:3])
    shard_targets = data[3][mine] if len(data) > 3 else None  # "visits" mode: this rank's rows of the CSR
    lrs = []
    for epoch in range(epochs):
        ep = T.train_one_epoch(ddp, T.batches(*shard, rank_batch_size(batch_size, world), True, gen, total=n_max,
                                              targets=shard_targets),
                               optimizer, scaler, accumulate_steps=accumulate_steps)
        val_loss = evaluate_sharded(model, data, va, batch_size, dev)
        plateau.step(val_loss)
        done += 1
        if val_loss < best:
            best, no_improve = val_loss, 0
        else:
            no_improve += 1
            if no_improve >= PATIENCE:
                break
        with warnings.catch_warnings():  # the reference passes the epoch to step() (deprecated form)
            warnings.simplefilter("ignore")
            cos.step(epoch + 1)
        step.step()
        lrs.append(optimizer.param_groups[0]["lr"])
    return {"ep": ep, "val_loss": val_loss, "epochs_run": done, "train_split": int(tr.numel()),
            "val_split": int(va.numel()), "lr": optimizer.param_groups[0]["lr"], "lr_per_epoch": lrs}


def make_lr_schedulers(optimizer):
    """The three schedulers train_with_validation builds per call (train.py:293-307), in its order."""
    cos = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, T_0=COSINE_T0, T_mult=1)
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=LR_GAMMA, patience=PATIENCE)
    step = torch.optim.lr_scheduler.StepLR(optimizer, step_size=LR_STEP_SIZE, gamma=LR_GAMMA)
    return cos, plateau, step


def reinforcement_loop(model, iterations: int, games_per_iter: int, device, *, epochs: int = TRAIN_EPOCHS,
                       batch_size: int = LEARN_BATCH_SIZE, lr: float = LEARN_LR,
                       accumulate_steps: int = T.ACCUM_STEPS, sims: int = 0, max_moves=None, slots: int = 256,
                       seed: int = 0, games_path: str | None = None, max_samples: int = 10000, log=print,
                       policy_target: str = "move", reuse_tree: bool = False, arena_games: int = 0,
                       arena_sims: int | None = None, leaves: int = 0, arena_leaves: int | None = None,
                       eval_cache: int = 0, arena_eval_cache: int | None = None, fast_sims: int = 0,
                       full_prob: float = 0.25, forced_k: float = 0.0):
    """Run the loop (learn.py reinforcement_loop :152-209); returns per-iteration statistics.
    `model` is a knightvision_amd.model.ChessNet (same parameters as ai/model.py) on `device`.
    `games_path`: the reference's JSONL dataset (ChessPGNDataset, :162) the self-play records extend --
    each sample keeps its own source's plane order and move indexing, as in the reference; None:
    self-play records only (iteration 1 then has nothing to train on).
    `policy_target`: "move" (the reference's loss: cross-entropy against the move played) or "visits"
    (no reference counterpart): the policy trains on each self-play record's MCTS root visit distribution
    (soft cross-entropy, PolicyTargets + train_ops.policy_loss), which needs sims > 0; the samples of
    `games_path` then carry their one-hot rows.
    `reuse_tree` (sims > 0): self-play carries the searched subtree from ply to ply (kv_config.reuse_tree); the
    per-iteration statistics then show the carried root visits (sims_kept) beside the new backups (sims).
    `arena_games` > 0 (no reference counterpart): after the iteration's update the new weights (player A) play
    `arena_games` games against the weights the iteration started from (player B) at `arena_sims` simulations a
    move (None: `sims`, which must then be > 0), sharded over the ranks by game id; st["arena"] gets
    arena.summarize of all ranks' games and "updated" (False: the iteration had nothing to train on, the match
    is the weights against themselves). Reporting only: no gating, no revert. 0: the loop as without it.
    `leaves` (sims > 0): descents in flight per game and sim-step in self-play (kv_config.leaves; 0 or 1: one);
    `arena_leaves`: the same for the matches (None: `leaves`).
    `eval_cache` (leaves >= 2): entries of the self-play engine's exact leaf-row cache (kv_config.eval_cache; 0: off);
    `arena_eval_cache`: the same per net for the matches (None: `eval_cache`). Neither changes a game.
    `fast_sims` > 0 (0 < fast_sims < sims; no reference counterpart): playout cap randomization in self-play
    (kv_config.fast_sims) -- each ply is searched to `sims` visits with probability `full_prob`, else to
    `fast_sims`. The statistics gain plies_full / plies_fast. With policy_target="visits" only the full plies'
    visit distributions train the policy (PolicyTargets.w, train.batch_loss); every record trains the value
    head. policy_target="move" trains on every record, fast plies included, as before. The matches
    (`arena_games`) always search every ply to `arena_sims`.
    `forced_k` > 0 (no reference counterpart): forced playouts and policy target pruning in self-play
    (kv_config.forced_k; KataGo: 2). With policy_target="visits" the policy trains on the pruned root counts; the
    statistics gain forced_descents / visits_pruned. The matches always run the plain search."""
    if policy_target not in ("move", "visits"):
        raise ValueError(f"reinforcement_loop: policy_target {policy_target!r}: 'move' or 'visits'")
    if arena_games > 0 and (arena_sims if arena_sims is not None else sims) <= 0:
        raise ValueError("reinforcement_loop: arena_games plays MCTS matches: arena_sims (or sims) must be > 0")
    visits = policy_target == "visits"
    if visits and sims <= 0:
        raise ValueError("reinforcement_loop: policy_target='visits' trains on the search's root visit counts: "
                         "sims must be > 0")
    _, rank, world = _dist()
    dev = torch.device(device)
    model.to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    ddp = T.wrap_ddp(model, dev)
    gen = torch.Generator().manual_seed(seed + rank)      # batch order (DataLoader shuffle), per rank
    split_gen = torch.Generator().manual_seed(seed)       # random_split: the same on every rank
    data = None  # (codes, moves, rewards) on the device: the whole dataset, on every rank
    if games_path is not None:
        data = T.ChessPGNDataset(games_path, max_samples=max_samples).materialize(dev)
        if visits:
            data = data + (PolicyTargets.one_hot(data[1]),)
    stats = []
    for it in range(iterations):
        st = {"iteration": it + 1, "policy_target": policy_target}
        n = int(data[0].shape[0]) if data is not None else 0
        incumbent = packed_from(model).copy() if arena_games > 0 else None  # the weights the iteration starts from
        if n >= 2 * world:  # every rank holds train data (fewer samples: no update this iteration)
            t0 = time.perf_counter()
            tv = train_with_validation(ddp, model, optimizer, data, epochs, batch_size, accumulate_steps, gen,
                                       split_gen, dev)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            ep = tv["ep"]
            st.update(train_s=time.perf_counter() - t0, train_loss=ep["loss"], train_samples=ep["samples"],
                      optimizer_steps=ep["optimizer_steps"], val_loss=tv["val_loss"], epochs_run=tv["epochs_run"],
                      train_split=tv["train_split"], val_split=tv["val_split"], lr=tv["lr"])
        model.eval()
        if arena_games > 0:
            t0 = time.perf_counter()
            ar = arena_shard(packed_from(model), incumbent, arena_games, it, dev, max_moves=max_moves, slots=slots,
                             sims=arena_sims if arena_sims is not None else sims,
                             leaves=arena_leaves if arena_leaves is not None else leaves,
                             eval_cache=arena_eval_cache if arena_eval_cache is not None else eval_cache)
            ar.pop("stats", None)
            ar["updated"] = n >= 2 * world
            st["arena"] = ar
            st["arena_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        pi = None
        if visits:
            recs, games, *pi = selfplay_shard(model, games_per_iter, it, dev, sims=sims, max_moves=max_moves,
                                              slots=slots, policy_targets=True, reuse_tree=reuse_tree,
                                              leaves=leaves, eval_cache=eval_cache, fast_sims=fast_sims,
                                              full_prob=full_prob, forced_k=forced_k)
            pi = None if recs is None else tuple(pi)
        else:
            recs, games = selfplay_shard(model, games_per_iter, it, dev, sims=sims, max_moves=max_moves, slots=slots,
                                         reuse_tree=reuse_tree, leaves=leaves, eval_cache=eval_cache,
                                         fast_sims=fast_sims, full_prob=full_prob, forced_k=forced_k)
        st["selfplay_s"] = time.perf_counter() - t0
        cal = getattr(selfplay_shard, "last_calibration", None)
        if cal is not None:  # fp32 AUTO: the self-play network's conv path for this iteration's weights
            st["nn_path"] = cal["path_large"]
            if cal.get("calibrated"):  # the load-time calibration (inside selfplay_s) and its candidates' errors
                st["calib_ms"] = cal["ms"]
                st["calib_err"] = {k: (cal["err_logit"][k], cal["err_value"][k]) for k in cal["err_logit"]}
        es = getattr(selfplay_shard, "last_stats", None)
        if es is not None:  # this rank's engine: plies and MCTS simulations (the throughput a path flip moves)
            st.update(plies=int(es["plies"]), sims=int(es["sims"]), sims_kept=int(es["sims_kept"]),
                      leaf_batch_rows=int(es["leaf_batch_rows"]), sim_steps=int(es["sim_steps"]),
                      plies_full=int(es["plies_full"]), plies_fast=int(es["plies_fast"]),
                      forced_descents=int(es["forced_descents"]), visits_pruned=int(es["visits_pruned"]))
        model.train()
        data = extend_dataset(data, recs, games, dev, pi=pi, policy_targets=True, weighted=fast_sims > 0) if visits \
            else extend_dataset(data, recs, games, dev)
        st.update(records=int(data[0].shape[0]) if data is not None else 0,
                  games=int(len(games)) if games is not None else 0)
        if rank == 0 and log:
            log(f"iteration {it + 1}/{iterations}: {st}")
        stats.append(st)
    return stats
