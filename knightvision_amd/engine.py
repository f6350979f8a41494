"""Python owner of one kv_engine (include/kv.h): the batched self-play engine
on one GPU. self_play.py builds the reference's API on top of this class."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .weights import pack_weights, state_dict_to_numpy

SEED_PER_GAME, SEED_SEQUENTIAL = 0, 1
EVAL_FAITHFUL, EVAL_LAZY, EVAL_HASH = 0, 1, 2

RECORD_DTYPE = np.dtype([("game_id", "<i8"), ("ply", "<i4"), ("move", "<u2"), ("pad", "<u2"),
                         ("board", "i1", (64,))])
GAME_DTYPE = np.dtype([("game_id", "<i8"), ("plies", "<i4"), ("outcome", "<i4"), ("reward", "<f4"),
                       ("reason", "<i4"), ("n_evals", "<i4"), ("pad", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_lib.Record) and GAME_DTYPE.itemsize == C.sizeof(_lib.Game)

REASONS = {0: "max_moves", 1: "Resignation", 2: "Checkmate", 3: "Stalemate", 4: "Draw", 5: "Material"}


def packed_from(weights) -> np.ndarray:
    """ChessNet module / state_dict / checkpoint dict / packed array -> packed fp32 blob."""
    if isinstance(weights, np.ndarray) and weights.ndim == 1:
        return np.ascontiguousarray(weights, dtype=np.float32)
    if hasattr(weights, "state_dict") and callable(weights.state_dict):
        m = weights.module if hasattr(weights, "module") else weights  # nn.DataParallel
        weights = m.state_dict()
    return pack_weights(state_dict_to_numpy(weights))[0]


from .model import ALGOS, PRECISIONS  # noqa: E402


def sim_groups_for(slots: int, sims: int, sim_groups: int = 0, arena: bool = False, *, leaves: int = 0) -> int:
    """The slot groups an engine with these settings runs its sim loop as (kv_sim_groups_for; no GPU needed);
    arena: a match engine (kv_config.arena), whose groups are its two players' chains; leaves > 1
    (kv_config.leaves): always one group, and sim_groups=2 is refused."""
    cfg = _lib.Config(slots=slots, sims=sims, sim_groups=sim_groups, arena=1 if arena else 0, leaves=int(leaves))
    rc = _lib.lib().kv_sim_groups_for(C.byref(cfg))
    _lib.check(min(rc, 0), "kv_sim_groups_for")
    return rc


class SelfPlayEngine:
    def __init__(self, weights, *, slots=256, n_games=256, seed=42, seed_mode=SEED_PER_GAME, max_moves=None,
                 batch=16, eps=0.25, alpha=0.3, sims=0, c_puct=1.5, eval_mode=EVAL_FAITHFUL, record_cap=None,
                 recycle=True, device=0, game_id_base=0, game_id_stride=1, precision="fp32",
                 algo="auto", tree_edge_cap=0, keep_root_visits=False, keep_root_moves=False, reuse_tree=False,
                 sim_groups=0, opponent=None, sample_plies=0, leaves=0, eval_cache=0, fast_sims=0, full_prob=0.25,
                 forced_k=0.0):
        """opponent (MCTS, sims >= 1): a second weight set makes the engine an arena (kv_config.arena): `weights`
        is player A, `opponent` player B, A plays white in the games with an even global id, and every ply is
        searched on the net of the side to move; games()["outcome"] stays white-perspective (arena.summarize
        attributes it). calibration_b() reports B's conv paths, stats()["arena_rows"] the leaf rows each net ran.
        sample_plies (MCTS): 0 every ply draws the move from the root visit counts, k > 0 only plies 0..k-1 do and
        the later ones take the first maximum, -1 every ply takes it (kv_config.sample_plies).
        reuse_tree (MCTS, sims >= 1): carry the subtree under the move just played into the next ply
        (kv_config.reuse_tree); stats() then reports sims_kept / roots_carried.
        sim_groups (MCTS): the slot groups a move's sim loop runs as, each on its own stream (kv_config.sim_groups):
        0 auto (sim_groups_for), 1 one group, 2 two groups; the results are the same bit for bit.
        leaves (MCTS, self-play and arena; kv_config.leaves): 0 or 1 one descent per game and sim-step; 2..64 that
        many in flight under virtual loss, a step's network batch being the pending leaves of all games, so a ply
        takes fewer, larger steps (another search than one leaf's: the visit counts differ). Not with reuse_tree,
        sim_groups=2 or sims=0. stats() reports sim_steps and leaf_rows_pending.
        eval_cache (leaves >= 2; kv_config.eval_cache): entries per network of an exact cache of the leaf rows in HBM,
        a power of two in [64, 2^24], 0 off: a leaf whose board and move list were evaluated before takes the stored
        logits and value and leaves the step's network batch. Play is byte for byte the play without it; stats()
        reports cache_probes / cache_hits / cache_stores, and nn_rows - cache_hits rows ran on the network.
        load_weights / load_opponent empty the table of the net they replace.
        fast_sims (MCTS self-play; kv_config.fast_sims): 0 off; 1 <= fast_sims < sims turns on playout cap
        randomization -- each ply is searched to `sims` root visits with probability full_prob and to fast_sims
        otherwise (a pure function of seed, game id and ply; full_q16 = round(full_prob * 65536) clipped to
        [1, 65536]). A fast ply's record has pad bit 0 set (fast_mask): it gives a value target and no policy
        target. stats() reports plies_full / plies_fast. Not with an opponent.
        forced_k (MCTS self-play; kv_config.forced_k): 0 off; 0 < forced_k <= 16 (KataGo: 2) turns on forced playouts
        and policy target pruning -- on a full ply a visited root move is searched at least sqrt(forced_k * P * visits)
        times, and at the move choice the forced visits PUCT would not have made are taken out again: the move is drawn
        from the pruned counts, which root_targets() returns (with keep_root_visits), while root_visits() keeps the
        raw ones. stats() reports forced_descents / visits_pruned. Not with an opponent."""
        L = _lib.lib()
        keep = 2 if keep_root_moves else (1 if keep_root_visits else 0)  # the move words imply the visits
        if record_cap is None:
            # one record per committed ply: a capped game holds at most max_moves; an uncapped one
            # (the reference default) is given 1,024 plies (its random-init games run 116-660). A
            # run that still fills the buffer fails with KV_EOVERFLOW ("record buffer full").
            per_game = int(max_moves) if max_moves else 1024
            # (the side buffers are 640 B per record each: 2^22 records with the visits, 2^21 with the moves too)
            record_cap = max(1 << 16, min(1 << {0: 27, 1: 22, 2: 21}[keep], int(n_games) * per_game))
        full_q16 = min(max(int(round(float(full_prob) * 65536)), 1), 65536) if int(fast_sims) else 0
        cfg = _lib.Config(device=device, slots=slots, n_games=n_games, game_id_base=game_id_base,
                          game_id_stride=game_id_stride, seed=seed, seed_mode=seed_mode,
                          max_moves=max_moves if max_moves else 0, batch=batch, eps=eps, alpha=alpha, sims=sims,
                          c_puct=c_puct, eval_mode=eval_mode, record_cap=record_cap, recycle=1 if recycle else 0,
                          precision=PRECISIONS[precision], algo=ALGOS[algo],
                          tree_edge_cap=int(tree_edge_cap), keep_root_visits=keep, reuse_tree=int(reuse_tree),
                          sim_groups=int(sim_groups), arena=0 if opponent is None else 1,
                          sample_plies=int(sample_plies), leaves=int(leaves), eval_cache=int(eval_cache),
                          fast_sims=int(fast_sims), full_q16=full_q16, forced_k=float(forced_k))
        h = C.c_void_p()
        _lib.check(L.kv_create(C.byref(cfg), C.byref(h)), "kv_create")
        self.h = h
        self.cfg = cfg
        self.load_weights(weights)
        if opponent is not None:
            self.load_opponent(opponent)

    def load_weights(self, weights):
        """(Re)load the network's weights -- player A's in an arena (kv_load_weights); empties its eval_cache."""
        packed = packed_from(weights)
        _lib.check(_lib.lib().kv_load_weights(self.h, packed.ctypes.data_as(C.POINTER(C.c_float)), packed.size),
                   "kv_load_weights")

    def load_opponent(self, weights):
        """(Re)load player B's weights of an arena engine (kv_load_weights_b); empties B's eval_cache."""
        packed = packed_from(weights)
        _lib.check(_lib.lib().kv_load_weights_b(self.h, packed.ctypes.data_as(C.POINTER(C.c_float)), packed.size),
                   "kv_load_weights_b")

    def run(self, max_steps: int = -1, stop_after_games: int = -1):
        _lib.check(_lib.lib().kv_run(self.h, int(max_steps), int(stop_after_games)), "kv_run")

    def set_max_moves(self, max_moves):
        _lib.check(_lib.lib().kv_set_max_moves(self.h, max_moves if max_moves else 0), "kv_set_max_moves")

    def _set_starts(self, states):
        """Test-only (kv_dev_set_starts): game g starts from states[g % n] ([n, 80] int8 state vectors); None
        restores the initial position. Only before the first run()."""
        if states is None:
            _lib.check(_lib.lib().kv_dev_set_starts(self.h, None, 0), "kv_dev_set_starts")
            return
        st = np.ascontiguousarray(states, dtype=np.int8).reshape(-1, 80)
        _lib.check(_lib.lib().kv_dev_set_starts(self.h, st.ctypes.data_as(C.POINTER(C.c_int8)), len(st)),
                   "kv_dev_set_starts")

    def reset_records(self):
        _lib.check(_lib.lib().kv_reset_records(self.h), "kv_reset_records")

    def sync(self):
        _lib.check(_lib.lib().kv_sync(self.h), "kv_sync")

    def records(self) -> np.ndarray:
        """All records so far, ordered by (game_id, ply)."""
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_records(self.h, None, 0, C.byref(n)), "kv_records")
        out = np.zeros(n.value, dtype=RECORD_DTYPE)
        if n.value:
            _lib.check(L.kv_records(self.h, out.ctypes.data_as(C.POINTER(_lib.Record)), n.value, C.byref(n)),
                       "kv_records")
        return out

    def records_device(self):
        """The records as a uint8 CUDA tensor [n, 80] on the engine's GPU, in allocation order
        (kv_records_device: no host round trip; sort after gathering)."""
        import torch
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_records_device(self.h, None, 0, C.byref(n), None), "kv_records_device")
        dev = torch.device("cuda", self.cfg.device)
        out = torch.empty((n.value, RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if n.value:
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.kv_records_device(self.h, C.c_void_p(out.data_ptr()), n.value, C.byref(n), C.c_void_p(st)),
                       "kv_records_device")
        return out

    def root_visits_device(self):
        """The MCTS root visit counts (pi) as a uint8 CUDA tensor [n, MAXM * 2] (uint16 counts, 0xffff padded),
        row k belonging to row k of records_device() (needs keep_root_visits=True)."""
        import torch
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_root_visits_device(self.h, None, 0, C.byref(n), None), "kv_root_visits_device")
        dev = torch.device("cuda", self.cfg.device)
        out = torch.empty((n.value, _lib.MAXM * 2), dtype=torch.uint8, device=dev)
        if n.value:
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.kv_root_visits_device(self.h, C.c_void_p(out.data_ptr()), n.value, C.byref(n),
                                               C.c_void_p(st)), "kv_root_visits_device")
        return out

    def root_visits(self) -> np.ndarray:
        """MCTS root visit counts [records, MAXM] (-1 padded), rows in records() order
        (needs keep_root_visits=True)."""
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_root_visits(self.h, None, 0, C.byref(n)), "kv_root_visits")
        out = np.zeros((n.value, _lib.MAXM), dtype=np.int32)
        if n.value:
            _lib.check(L.kv_root_visits(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)),
                       "kv_root_visits")
        return out

    def root_targets(self) -> np.ndarray:
        """The pruned root counts T (the policy targets of forced_k > 0) [records, MAXM] (-1 padded), rows in
        records() order, root_visits()'s layout (needs forced_k > 0 and keep_root_visits=True)."""
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_root_targets(self.h, None, 0, C.byref(n)), "kv_root_targets")
        out = np.zeros((n.value, _lib.MAXM), dtype=np.int32)
        if n.value:
            _lib.check(L.kv_root_targets(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)),
                       "kv_root_targets")
        return out

    def root_targets_device(self):
        """The same counts as a uint8 CUDA tensor [n, MAXM * 2] (uint16, 0xffff padded), row k belonging to row k
        of records_device() and of root_visits_device()."""
        import torch
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_root_targets_device(self.h, None, 0, C.byref(n), None), "kv_root_targets_device")
        dev = torch.device("cuda", self.cfg.device)
        out = torch.empty((n.value, _lib.MAXM * 2), dtype=torch.uint8, device=dev)
        if n.value:
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.kv_root_targets_device(self.h, C.c_void_p(out.data_ptr()), n.value, C.byref(n),
                                                C.c_void_p(st)), "kv_root_targets_device")
        return out

    def root_moves(self) -> np.ndarray:
        """The root move words [records, MAXM] uint16 (from | to << 6 | flags << 12, 0xffff padded) the counts of
        root_visits() are indexed by, rows in records() order (needs keep_root_moves=True). The policy logit
        of a word w is (w & 63) * 64 + ((w >> 6) & 63)."""
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_root_moves(self.h, None, 0, C.byref(n)), "kv_root_moves")
        out = np.zeros((n.value, _lib.MAXM), dtype=np.uint16)
        if n.value:
            _lib.check(L.kv_root_moves(self.h, out.ctypes.data_as(C.POINTER(C.c_uint16)), n.value, C.byref(n)),
                       "kv_root_moves")
        return out

    def root_moves_device(self):
        """The same move words as a uint8 CUDA tensor [n, MAXM * 2], row k belonging to row k of
        records_device() and of root_visits_device() (needs keep_root_moves=True)."""
        import torch
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_root_moves_device(self.h, None, 0, C.byref(n), None), "kv_root_moves_device")
        dev = torch.device("cuda", self.cfg.device)
        out = torch.empty((n.value, _lib.MAXM * 2), dtype=torch.uint8, device=dev)
        if n.value:
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.kv_root_moves_device(self.h, C.c_void_p(out.data_ptr()), n.value, C.byref(n),
                                              C.c_void_p(st)), "kv_root_moves_device")
        return out

    def games(self) -> np.ndarray:
        L = _lib.lib()
        n = C.c_size_t()
        _lib.check(L.kv_games(self.h, None, 0, C.byref(n)), "kv_games")
        out = np.zeros(n.value, dtype=GAME_DTYPE)
        if n.value:
            _lib.check(L.kv_games(self.h, out.ctypes.data_as(C.POINTER(_lib.Game)), n.value, C.byref(n)),
                       "kv_games")
        return out

    def calibration(self) -> dict:
        """The network's conv paths and load-time calibration (kv_engine_calibration)."""
        c = _lib.Calib()
        _lib.check(_lib.lib().kv_engine_calibration(self.h, C.byref(c)), "kv_engine_calibration")
        return _lib.calib_dict(c)

    def calibration_b(self) -> dict:
        """Player B's conv paths and load-time calibration (an arena engine, kv_engine_calibration_b)."""
        c = _lib.Calib()
        _lib.check(_lib.lib().kv_engine_calibration_b(self.h, C.byref(c)), "kv_engine_calibration_b")
        return _lib.calib_dict(c)

    def stats(self) -> dict:
        st = _lib.Stats()
        _lib.check(_lib.lib().kv_stats_get(self.h, C.byref(st)), "kv_stats_get")
        out = {k: getattr(st, k) for k, _ in _lib.Stats._fields_}
        out["dom_kernel"] = out["dom_kernel"].decode()
        out["arena_rows"] = (int(st.arena_rows[0]), int(st.arena_rows[1]))
        return out

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().kv_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SEARCH_DTYPE = np.dtype([("status", "<i4"), ("n_moves", "<i4"), ("sims", "<i4"), ("best", "<i4"), ("pv_len", "<i4"),
                         ("steps", "<i4"), ("nn_rows", "<i4"), ("pad", "<i4"), ("root_value", "<f4"),
                         ("best_q", "<f4"), ("pv", "<u2", (16,)), ("moves", "<u2", (_lib.MAXM,)),
                         ("visits", "<i4", (_lib.MAXM,)), ("q", "<f4", (_lib.MAXM,)),
                         ("prior", "<f4", (_lib.MAXM,))])
assert SEARCH_DTYPE.itemsize == C.sizeof(_lib.SearchResult)

SEARCH_STATUS = {0: "searched", 1: "checkmated", 2: "stalemate", 3: "draw"}


class PositionSearch:
    """PUCT search of given positions on one GPU (kv_search, include/kv.h): up to max_positions roots per
    call, up to max_sims simulations each. The weights are loaded (and the conv path calibrated) once."""

    def __init__(self, weights, *, max_positions, max_sims, c_puct=1.5, eval_mode=EVAL_FAITHFUL, precision="fp32",
                 algo="auto", tree_edge_cap=0, device=0):
        L = _lib.lib()
        cfg = _lib.Config(device=device, slots=int(max_positions), n_games=0, game_id_base=0, game_id_stride=1,
                          seed=0, seed_mode=SEED_PER_GAME, max_moves=0, batch=1, eps=0.0, alpha=0.3,
                          sims=int(max_sims), c_puct=c_puct, eval_mode=eval_mode, record_cap=1, recycle=0,
                          precision=PRECISIONS[precision], algo=ALGOS[algo], tree_edge_cap=int(tree_edge_cap),
                          keep_root_visits=0)
        h = C.c_void_p()
        _lib.check(L.kv_create(C.byref(cfg), C.byref(h)), "kv_create")
        self.h = h
        self.cfg = cfg
        packed = packed_from(weights)
        _lib.check(L.kv_load_weights(self.h, packed.ctypes.data_as(C.POINTER(C.c_float)), packed.size),
                   "kv_load_weights")

    def search(self, states, sims, leaves=1, eps=0.0, alpha=0.3, seed=0) -> np.ndarray:
        """states: [n, 80] int8 state vectors (GameState._state(), the oracle's) -> SEARCH_DTYPE[n]: root visit
        counts, q, priors and move words in root list order, best move index, principal variation."""
        st = np.ascontiguousarray(states, dtype=np.int8).reshape(-1, 80)
        out = np.zeros(len(st), dtype=SEARCH_DTYPE)
        p = _lib.SearchParams(sims=int(sims), leaves=int(leaves), eps=float(eps), alpha=float(alpha), seed=int(seed))
        _lib.check(_lib.lib().kv_search(self.h, st.ctypes.data_as(C.POINTER(C.c_int8)), len(st), C.byref(p),
                                        out.ctypes.data_as(C.POINTER(_lib.SearchResult))), "kv_search")
        self._n = len(st)
        return out

    # -- search sessions (include/kv.h): the trees of the last search() follow a game
    def advance(self, edges) -> np.ndarray:
        """Play root move edges[i] (root list index, -1: none) in every tree of the last search: the child's
        subtree becomes the tree; an edge the search never expanded drops it -> the [n, 80] states after the
        moves."""
        ed = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
        out = np.zeros((len(ed), 80), dtype=np.int8)
        _lib.check(_lib.lib().kv_search_advance(self.h, len(ed), ed.ctypes.data_as(C.POINTER(C.c_int32)),
                                                out.ctypes.data_as(C.POINTER(C.c_int8))), "kv_search_advance")
        return out

    def resume(self, sims, leaves=1, alpha=0.3, seed=0):
        """Search the session's current roots up to `sims` root visits, the carried visits counting ->
        (SEARCH_DTYPE[n] with steps / nn_rows of this call only, kept[n]: the visits each root already held)."""
        n = getattr(self, "_n", 0)
        out = np.zeros(n, dtype=SEARCH_DTYPE)
        kept = np.zeros(n, dtype=np.int32)
        p = _lib.SearchParams(sims=int(sims), leaves=int(leaves), eps=0.0, alpha=float(alpha), seed=int(seed))
        _lib.check(_lib.lib().kv_search_continue(self.h, n, C.byref(p),
                                                 out.ctypes.data_as(C.POINTER(_lib.SearchResult)),
                                                 kept.ctypes.data_as(C.POINTER(C.c_int32))), "kv_search_continue")
        return out, kept

    def tree_size(self, i):
        """(nodes, edges of the pool in use) of the session's tree i."""
        nodes, edges = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().kv_search_tree_size(self.h, int(i), C.byref(nodes), C.byref(edges)),
                   "kv_search_tree_size")
        return nodes.value, edges.value

    def calibration(self) -> dict:
        c = _lib.Calib()
        _lib.check(_lib.lib().kv_engine_calibration(self.h, C.byref(c)), "kv_engine_calibration")
        return _lib.calib_dict(c)

    def stats(self) -> dict:
        st = _lib.Stats()
        _lib.check(_lib.lib().kv_stats_get(self.h, C.byref(st)), "kv_stats_get")
        out = {k: getattr(st, k) for k, _ in _lib.Stats._fields_}
        out["dom_kernel"] = out["dom_kernel"].decode()
        out["arena_rows"] = (0, 0)  # (a position search has one network)
        return out

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().kv_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fast_mask(recs: np.ndarray) -> np.ndarray:
    """bool[n]: the records of fast plies (kv_record.pad bit 0, kv_config.fast_sims): value targets only."""
    return (np.asarray(recs["pad"]) & 1).astype(bool)


def records_by_game(recs: np.ndarray, games: np.ndarray):
    """-> {game_id: (moves uint16[plies], boards int8[plies,64], reward)}."""
    out = {}
    if len(recs) == 0:
        return out
    ids = recs["game_id"]
    cuts = np.flatnonzero(np.diff(ids)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(recs)]])
    reward = {int(g["game_id"]): float(g["reward"]) for g in games}
    for s, e in zip(starts, ends):
        gid = int(ids[s])
        out[gid] = (recs["move"][s:e].copy(), recs["board"][s:e].copy(), reward.get(gid))
    return out
