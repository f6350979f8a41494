"""The evaluation cache (kv_config.eval_cache; knightvision_amd/csrc/kv_cache.hip, eng_leaves_ply in kv_engine.hip)
through the C ABI. Every comparison is exact:

* kv_dev_eval_cache -- the product's probe and store kernels on given rows -- against the restatement
  (tests/_eval_cache.py): hit flags, and payloads as bit patterns.
* Play with the cache on is the play with it off byte for byte: hash evaluator runs (self-play and arena), whose
  hit, store and batch-row counts are the restatement's, and the real network in both batch classes.
* A weight reload empties the table; kv_create's refusals; the Python surface.

The engine runs and the restated games are computed once per configuration and shared by the tests."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import EVAL_HASH, SelfPlayEngine
from knightvision_amd.weights import synthetic_state_dict

from tests import _eval_cache as EC
from tests import _mcts_selfplay_leaves as SL

pytestmark = pytest.mark.gpu

SEED = SL.SEED
MAXM, CM = _lib.MAXM, _lib.CACHE_MAXM
PARTS = ("records", "root visits", "root moves", "game table")


# ---- 1. the kernels against the restatement
def _dev_eval_cache(entries, rows, step_len, buffers):
    """rows: (board[64], words, payload logits uint32 [MAXM], payload value uint32) -> hit [n], logits [n][MAXM],
    values [n], counters [3] of kv_dev_eval_cache; the move words past a row's count are random, as a reused
    workspace row holds them -- but for a key in buffers ((board, words) as tuples -> MAXM words), whose rows all
    carry that whole buffer."""
    n = len(rows)
    rng = np.random.default_rng(11)
    boards = np.array([r[0] for r in rows], dtype=np.int8)
    moves = rng.integers(0, 1 << 16, size=(n, MAXM), dtype=np.uint16)
    counts = np.array([len(r[1]) for r in rows], dtype=np.int32)
    for k, r in enumerate(rows):
        moves[k, :len(r[1])] = r[1]
        whole = buffers.get((tuple(r[0]), tuple(r[1])))
        if whole is not None:
            assert list(whole[:len(r[1])]) == list(r[1])
            moves[k] = whole
    logits = np.array([r[2] for r in rows], dtype=np.uint32)
    values = np.array([r[3] for r in rows], dtype=np.uint32)
    steps = np.array(step_len, dtype=np.int32)
    hit = np.full(n, -1, dtype=np.int32)
    out_l, out_v = np.zeros((n, MAXM), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    ctr = np.zeros(3, dtype=np.int64)
    P = C.POINTER
    _lib.check(_lib.lib().kv_dev_eval_cache(
        0, entries, boards.ctypes.data_as(P(C.c_int8)), moves.ctypes.data_as(P(C.c_uint16)),
        counts.ctypes.data_as(P(C.c_int)), logits.ctypes.data_as(P(C.c_uint32)), values.ctypes.data_as(P(C.c_uint32)),
        n, steps.ctypes.data_as(P(C.c_int)), len(steps), hit.ctypes.data_as(P(C.c_int32)),
        out_l.ctypes.data_as(P(C.c_uint32)), out_v.ctypes.data_as(P(C.c_uint32)), ctr.ctypes.data_as(P(C.c_int64))),
        "kv_dev_eval_cache")
    return hit, out_l, out_v, ctr


def _kernel_case():
    """Keys of every move count at which the kernels take another path; pairs of keys that differ in one place only
    and -- found with the restated hash -- share an entry, so that only the whole-key compare tells them apart; two
    unrelated keys on one entry; steps of 1, 17 and 300 rows that hold equal rows and both keys of an entry."""
    rng = random.Random(3)
    sizes = (0, 1, 63, 64, 65, CM, CM + 1, MAXM)
    board = lambda: [rng.randrange(13) for _ in range(64)]  # noqa: E731
    words = lambda n: [rng.randrange(1 << 16) for _ in range(n)]  # noqa: E731
    table = EC.Table(64)
    index = lambda k: table.index(EC.make_key(*k))  # noqa: E731

    def twin(make):
        """(a, b) from make() -> (a, candidates for b): the first candidate on a's entry."""
        while True:
            a, cands = make()
            for b in cands:
                if b != a and index(b) == index(a):
                    return a, b

    def byte63():
        b, w = board(), words(CM)
        return (b, w), [(b[:63] + [c], w) for c in range(13)]

    def last_word(n):
        def make():
            b, w = board(), words(n)
            return (b, w), [(b, w[:-1] + [x]) for x in range(0, 1 << 16, 97)]
        return make

    def count_only():
        b, w = board(), words(64)
        return (b, w), [(b, w + [x]) for x in range(0, 1 << 16, 97)]

    def no_moves():
        b = board()
        return (b, []), [(b[:63] + [c], []) for c in range(13)]

    # differ only in: board byte 63; the last move word (n = KV_CACHE_MAXM, and n = 64, the end of a whole 16-byte
    # group); n (and the word n adds); board byte 63 with no moves at all
    pairs = [twin(byte63), twin(last_word(CM)), twin(last_word(64)), twin(count_only), twin(no_moves)]
    # the pair that differs only in n, with byte-equal move buffers: both keys' rows carry the longer key's words
    # and the same words after them, so only the count in the entry's header tells the two apart
    whole = pairs[3][1][1] + words(MAXM - 65)
    assert pairs[3][0][1] == whole[:64] and pairs[3][0][0] == pairs[3][1][0]
    buffers = {(tuple(bd), tuple(wd)): whole for bd, wd in pairs[3]}
    by_entry = {}
    while True:  # two unrelated keys on one entry
        k = (board(), words(rng.choice((1, 20, 64))))
        other = by_entry.setdefault(index(k), k)
        if other is not k:
            same_entry = (other, k)
            break
    pool = [(board(), words(n)) for n in sizes for _ in range(3)]
    everything = pool + [k for p in pairs for k in p] + list(same_entry)
    first = pool[0]
    pick = lambda src, n: [rng.choice(src) for _ in range(n)]  # noqa: E731
    steps = [[first],
             [first, same_entry[0], same_entry[1], pool[3], pool[3]] + [a for a, _ in pairs] + [pool[9], pool[9]]
             + pick(pool, 5),
             [b for _, b in pairs] + [same_entry[1], same_entry[0], pool[3]] + pick(pool, 9),
             [a for a, _ in pairs] + pick(everything, 295),
             pick(everything, 300),
             [same_entry[0]]]
    assert [len(s) for s in steps] == [1, 17, 17, 300, 300, 1]
    special = [0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0x00000001, 0]  # -0.0, NaNs, inf, a subnormal, 0
    rows = []
    for s in steps:
        for bd, wd in s:  # every row its own payload: which of two equal rows was stored shows
            lg = [rng.choice(special) if rng.random() < 0.2 else rng.getrandbits(32) for _ in range(MAXM)]
            rows.append((bd, wd, lg, rng.choice(special) if rng.random() < 0.3 else rng.getrandbits(32)))
    return rows, [len(s) for s in steps], pairs, same_entry, buffers


def test_kernels_against_the_restatement():
    rows, step_len, pairs, same_entry, buffers = _kernel_case()
    hit, out_l, out_v, ctr = _dev_eval_cache(64, rows, step_len, buffers)
    table = EC.Table(64)
    assert table.index(EC.make_key(*same_entry[0])) == table.index(EC.make_key(*same_entry[1]))
    want_hit, want_l, want_v = [], [], []
    r0 = 0
    for n in step_len:
        part = rows[r0:r0 + n]
        keys = [EC.make_key(bd, wd) for bd, wd, _, _ in part]
        out, miss = EC.run_step(table, keys, lambda m: [(tuple(part[i][2][:len(part[i][1])]), part[i][3]) for i in m])
        for i in range(n):
            want_hit.append(0 if i in miss else 1)
            want_l.append(out[i][0])
            want_v.append(out[i][1])
        r0 += n
    want_hit = np.array(want_hit, dtype=np.int32)
    print(f"kv_dev_eval_cache: {len(rows)} rows, hits {int(want_hit.sum())}, stores {table.stores}, device counters "
          f"{ctr.tolist()}, move counts hit {sorted({len(rows[k][1]) for k in np.nonzero(want_hit)[0]})}")
    assert np.array_equal(hit, want_hit)
    assert ctr.tolist() == [table.probes, table.hits, table.stores] and table.hits == want_hit.sum()
    for k, (bd, wd, _, _) in enumerate(rows):
        n = len(wd)
        if want_hit[k]:
            assert out_l[k, :n].tolist() == list(want_l[k]), k
            assert int(out_v[k]) == want_v[k], k
        else:
            assert int(out_v[k]) == 0xFFFFFFFF, k
            n = 0
        assert (out_l[k, n:] == 0xFFFFFFFF).all(), k  # nothing past the row's moves, nothing on a miss
    # what the case was built to hold
    hit_counts = {len(rows[k][1]) for k in np.nonzero(want_hit)[0]}
    assert {0, 1, 63, 64, 65, CM} <= hit_counts and not any(len(rows[k][1]) > CM and want_hit[k]
                                                            for k in range(len(rows)))
    second = rows[1:18]
    assert want_hit[1] == 1 and want_hit[2] == want_hit[3] == 0  # step 2: the stored row; both keys of one entry
    assert second[3][:2] == second[4][:2] and want_hit[4] == want_hit[5] == 0  # equal rows of one step both miss
    for a, b in pairs:
        assert table.index(EC.make_key(*a)) == table.index(EC.make_key(*b)) and a != b
    # step 3 probes each pair's other key on the entry the first holds, step 4 the first again: all miss
    assert not want_hit[18:23].any() and not want_hit[35:40].any()
    assert want_hit[23] == 0 and want_hit[24] == 1 and want_hit[25] == 1  # the entry kept its earliest miss


# ---- 2. hash evaluator runs: on == off, the counters are the restatement's
@functools.lru_cache(maxsize=None)
def _run(a, b, slots, n_games, sims, steps, leaves, eval_cache, max_moves=None, hash_eval=False, base=0):
    """One engine run (b None: self-play of a) -> (records, root visits, root move words, games, stats)."""
    opp = None if b is None else synthetic_state_dict(42, b)
    with SelfPlayEngine(synthetic_state_dict(42, a), opponent=opp, slots=slots, n_games=n_games, seed=SEED,
                        max_moves=max_moves, sims=sims, c_puct=1.5, keep_root_moves=True, leaves=leaves,
                        game_id_base=base, eval_mode=EVAL_HASH if hash_eval else 0, eval_cache=eval_cache) as eng:
        eng.run(steps)
        return eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()


@functools.lru_cache(maxsize=None)
def _restated(name, entries):
    return EC.restate(EC.ARENA_RUN if name == "arena" else EC.RUNS[name], entries, arena=name == "arena")


def _same_play(on, off):
    for k, part in enumerate(PARTS):
        assert on[k].tobytes() == off[k].tobytes(), part
    for key in ("steps", "plies", "games_done", "nn_rows", "sims", "records", "sim_steps", "leaf_rows_pending",
                "tree_overflows"):
        assert on[4][key] == off[4][key], key


@pytest.mark.parametrize("entries", [64, 1 << 16])
@pytest.mark.parametrize("name", sorted(EC.RUNS) + ["arena"])
def test_hash_runs_play_the_same_and_count_as_restated(name, entries):
    arena = name == "arena"
    cfg = EC.ARENA_RUN if arena else EC.RUNS[name]
    args = ("init", "init" if arena else None, cfg["slots"], cfg["n_games"], cfg["sims"], -1, cfg["leaves"])
    kw = dict(max_moves=cfg["max_moves"], hash_eval=True, base=cfg["base"])
    off, on = _run(*args, 0, **kw), _run(*args, entries, **kw)
    assert len(off[0]) == sum(cfg["plies"]) and (off[3]["reason"] == 0).all()  # the restated games are these
    _same_play(on, off)
    _, info, caches = _restated(name, entries)
    caches = caches[:2 if arena else 1]
    st, so = on[4], off[4]
    want = {k: sum(getattr(c.table, k) for c in caches) for k in ("probes", "hits", "stores")}
    rows = [c.batch_rows for c in caches]
    print(f"{name} eval_cache {entries}: probes {st['cache_probes']} hits {st['cache_hits']} stores "
          f"{st['cache_stores']} (restated {want}), leaf_batch_rows {st['leaf_batch_rows']} (restated {rows}, off "
          f"{so['leaf_batch_rows']}), arena_rows {st['arena_rows']}")
    assert so["cache_probes"] == so["cache_hits"] == so["cache_stores"] == 0
    assert st["cache_probes"] == st["leaf_rows_pending"] == sum(info["pending"]) == want["probes"]
    assert st["cache_hits"] == want["hits"] > 0
    assert st["cache_stores"] == want["stores"]
    assert st["leaf_batch_rows"] == sum(rows) < so["leaf_batch_rows"]  # (the padding of a short list aside)
    assert st["arena_rows"] == (tuple(rows) if arena else (0, 0))
    assert st["nn_rows"] == so["nn_rows"] == sum(cfg["plies"]) + sum(info["pending"])


# ---- 3. the real network, both batch classes
@pytest.mark.parametrize("variant,slots", [("init", 6), ("stress", 6), ("init", 3), ("stress", 3)])
def test_network_play_is_the_same(variant, slots):
    sims, leaves, steps = 32, 4, 3
    off = _run(variant, None, slots, slots, sims, steps, leaves, 0)
    on = _run(variant, None, slots, slots, sims, steps, leaves, 1 << 12)
    assert len(off[0]) == slots * steps
    _same_play(on, off)
    st = on[4]
    print(f"{variant}, {slots} slots x {leaves}: probes {st['cache_probes']} hits {st['cache_hits']} stores "
          f"{st['cache_stores']}, leaf_batch_rows {st['leaf_batch_rows']} (off {off[4]['leaf_batch_rows']})")
    assert st["cache_probes"] == st["leaf_rows_pending"] and st["cache_hits"] > 0
    assert st["leaf_batch_rows"] <= off[4]["leaf_batch_rows"] - (st["cache_hits"] if slots * leaves <= 16 else 0)


def test_arena_of_a_net_against_itself_is_selfplay_with_the_cache():
    solo = _run("init", None, 6, 6, 32, 3, 4, 1 << 12)
    arena = _run("init", "init", 6, 6, 32, 3, 4, 1 << 12)
    for k, part in enumerate(PARTS):
        assert arena[k].tobytes() == solo[k].tobytes(), part
    st = arena[4]
    assert st["cache_probes"] == st["leaf_rows_pending"] == solo[4]["leaf_rows_pending"] and st["cache_hits"] > 0
    assert st["arena_rows"][0] + st["arena_rows"][1] == st["leaf_batch_rows"]


# ---- 4. a weight reload empties the table
def _reload_run(eval_cache):
    with SelfPlayEngine(synthetic_state_dict(42, "init"), slots=6, n_games=6, seed=SEED, sims=32, c_puct=1.5,
                        keep_root_moves=True, leaves=4, eval_cache=eval_cache) as eng:
        eng.run(2)
        mid = eng.stats()
        eng.load_weights(synthetic_state_dict(42, "stress"))
        eng.run(2)
        return (eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()), mid


def test_weight_reload_empties_the_table():
    (off, _), (on, mid) = _reload_run(0), _reload_run(1 << 12)
    assert len(off[0]) == 6 * 4
    _same_play(on, off)
    print(f"reload: hits {mid['cache_hits']} before, {on[4]['cache_hits'] - mid['cache_hits']} after")
    assert mid["cache_hits"] > 0 and on[4]["cache_hits"] > mid["cache_hits"]
    # the second weight set matters: the run is not the one that keeps the first
    keep = _run("init", None, 6, 6, 32, 4, 4, 1 << 12)
    assert keep[0].tobytes() != on[0].tobytes() or keep[1].tobytes() != on[1].tobytes()


# ---- 5. refusals and the Python surface
def _cfg(**kw):
    base = dict(device=0, slots=4, n_games=4, game_id_base=0, game_id_stride=1, seed=SEED, seed_mode=0, max_moves=0,
                batch=16, eps=0.25, alpha=0.3, sims=8, c_puct=1.5, eval_mode=EVAL_HASH, record_cap=1 << 10,
                recycle=1, precision=0, algo=0, tree_edge_cap=0, keep_root_visits=0, leaves=4)
    base.update(kw)
    return _lib.Config(**base)


@pytest.mark.parametrize("kw,text", [
    (dict(eval_cache=-64), "eval_cache -64 must be 0 (off) or a power of two in [64, 2^24]"),
    (dict(eval_cache=32), "eval_cache 32 must be 0 (off) or a power of two"),
    (dict(eval_cache=96), "eval_cache 96 must be 0 (off) or a power of two"),
    (dict(eval_cache=1 << 25), "must be 0 (off) or a power of two in [64, 2^24]"),
    (dict(eval_cache=64, leaves=0), "eval_cache 64 with leaves 0"),
    (dict(eval_cache=64, leaves=1), "eval_cache 64 with leaves 1"),
    (dict(eval_cache=64, leaves=1, arena=1), "eval_cache 64 with leaves 1"),
])
def test_create_refusals(kw, text):
    h = C.c_void_p()
    rc = _lib.lib().kv_create(C.byref(_cfg(**kw)), C.byref(h))
    assert rc == -1, rc  # KV_EINVAL
    msg = _lib.lib().kv_last_error().decode()
    assert text in msg, msg
    assert not h.value


def test_play_match_and_the_loop_take_eval_cache():
    from knightvision_amd import arena
    from knightvision_amd.learn import reinforcement_loop, selfplay_shard
    from knightvision_amd.model import ChessNet
    a, b = synthetic_state_dict(42, "init"), synthetic_state_dict(42, "peaked")
    kw = dict(sims=16, slots=6, seed=SEED, max_moves=4, sample_plies=2, leaves=4)
    off = arena.play_match(a, b, 6, **kw)
    on = arena.play_match(a, b, 6, eval_cache=1 << 10, **kw)
    assert on["game_table"].tobytes() == off["game_table"].tobytes()
    assert on["stats"]["cache_hits"] > 0 == off["stats"]["cache_hits"]
    assert on["stats"]["leaf_batch_rows"] <= off["stats"]["leaf_batch_rows"]  # (lists this short are padded to 17)
    torch.manual_seed(0)
    m = ChessNet()
    stats = reinforcement_loop(m, iterations=1, games_per_iter=6, device="cuda:0", epochs=1, batch_size=64,
                               max_moves=4, slots=6, log=None, sims=16, leaves=4, arena_games=6, arena_leaves=2,
                               eval_cache=1 << 10, arena_eval_cache=64)
    assert stats[0]["arena"]["games"] == 6
    assert selfplay_shard.last_stats["cache_hits"] > 0
    assert selfplay_shard.last_stats["cache_probes"] == selfplay_shard.last_stats["leaf_rows_pending"]


# ---- recycling: more games than slots while the table is warm (tests/_mcts_starts.RECYCLE)
@functools.lru_cache(maxsize=None)
def _recycling_run(entries):
    from tests import _mcts_starts as ST
    cfg = ST.RECYCLE
    with SelfPlayEngine(synthetic_state_dict(42, "init"), slots=cfg["slots"], n_games=cfg["n_games"], seed=ST.SEED,
                        max_moves=ST.MAX_MOVES, sims=ST.SIMS, c_puct=ST.C_PUCT, eps=ST.EPS, alpha=ST.ALPHA,
                        keep_root_moves=True, leaves=cfg["leaves"], eval_cache=entries, eval_mode=EVAL_HASH) as eng:
        eng._set_starts(ST.start_list())
        eng.run()
        return eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()


@pytest.mark.parametrize("size", ["small", "large"])
def test_recycled_slots_find_the_finished_games_entries(size):
    """22 games from the start set on 2 slots: a game that starts in a recycled slot probes a table that holds the
    finished games' entries, and the slot it sits in decides who wins a contested entry. The games are those of
    the run without the cache byte for byte, the three counters the restatement's with its rows in slot order
    (tests/test_eval_cache_cpu.py: the seating is unambiguous, a later game hits an earlier game's entry in the
    large table, entries are contested in both). The game table is compared with the
    run without the cache only."""
    from tests import _mcts_starts as ST
    entries = ST.RECYCLE[size]
    off, on = _recycling_run(0), _recycling_run(entries)
    for k, part in enumerate(PARTS[:3]):
        assert on[k].tobytes() == off[k].tobytes(), part
    assert np.array_equal(np.sort(on[3], order="game_id"), np.sort(off[3], order="game_id")), PARTS[3]
    assert len(on[3]) == ST.RECYCLE["n_games"]
    for key in ("plies", "sims", "nn_rows", "leaf_rows_pending", "sim_steps", "games_done"):
        assert on[4][key] == off[4][key], key
    games, info, cache = ST.cached_recycling_run(entries)
    recs = on[0]
    for g, p in enumerate(games):
        sel = recs["game_id"] == g
        assert recs["move"][sel].tolist() == [x["move"] for x in p], g
        assert sel.sum() == len(p) and [v[v >= 0].tolist() for v in on[1][sel]] == [x["visits"] for x in p], g
        assert [bytes(b) for b in recs["board"][sel]] == [e["board"] for e in p.extra], g
        assert [w[w != 0xffff].tolist() for w in on[2][sel]] == [x["words"] for x in p], g
    t = cache.table
    st = on[4]
    print(f"eval_cache {entries} on {ST.RECYCLE['slots']} slots: probes / hits / stores {st['cache_probes']} / "
          f"{st['cache_hits']} / {st['cache_stores']} (restated {t.probes} / {t.hits} / {t.stores}), contests "
          f"{cache.contests}, hits on another game's entry {sum(a != b for a, b in cache.hits_from)}")
    assert (st["cache_probes"], st["cache_hits"], st["cache_stores"]) == (t.probes, t.hits, t.stores)
    assert st["sim_steps"] == info["steps"] and st["leaf_rows_pending"] == t.probes
    assert (off[4]["cache_probes"], off[4]["cache_hits"], off[4]["cache_stores"]) == (0, 0, 0)
