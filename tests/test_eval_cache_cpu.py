"""The evaluation cache's restatement (tests/_eval_cache.py) on the CPU: the step rule against brute-force
dictionaries on random keys, the ctypes mirrors against the library's struct sizes, the cached driver against
tests/_mcts_selfplay_leaves.play_many, and the cases the GPU comparison's runs must hold (with the hash as built:
another hash needs the conditions checked again, not loosened)."""
import ctypes as C
import functools
import random

import numpy as np

from knightvision_amd import _lib

from tests import _eval_cache as EC
from tests import _mcts_selfplay_leaves as SL


def _random_pool(rng, count, sizes=(0, 1, 5, 40, EC.CACHE_MAXM, EC.CACHE_MAXM + 1, 200)):
    return [EC.make_key([rng.randrange(13) for _ in range(64)],
                        [rng.randrange(1 << 16) for _ in range(rng.choice(sizes))]) for _ in range(count)]


def _steps(rng, pool, lengths):
    return [[rng.choice(pool) for _ in range(n)] for n in lengths]


def test_hash_is_the_documented_function():
    assert EC.mix64(0) == 0 and EC.mix64(1) == 0x5692161D100B05E5  # splitmix64's finaliser
    key = EC.make_key([0] * 64, [])
    want = 0
    for k in range(33):
        want ^= EC.mix64(((k + 1) * 0x9E3779B97F4A7C15) % (1 << 64))
    assert EC.key_hash(key) == want
    # every word of the key and its place enter the hash
    b = [3] * 64
    base = EC.key_hash(EC.make_key(b, [7, 9]))
    assert base != EC.key_hash(EC.make_key(b, [9, 7])) != EC.key_hash(EC.make_key(b, [7, 9, 0]))
    assert base != EC.key_hash(EC.make_key(b[:63] + [4], [7, 9]))
    assert EC.key_words(EC.make_key([1, 2] + [0] * 62, [5]))[:2] == [1 | (2 << 8), 0]


def test_step_rule_against_an_unbounded_dictionary():
    """Where no two keys share an entry, a row hits iff its key was in an earlier step (and holds at most
    CACHE_MAXM moves), and the payload is that of the key's first row in the last step that missed it."""
    rng = random.Random(5)
    pool = _random_pool(rng, 120)
    table = EC.Table(1 << 24)
    assert len({table.index(k) for k in pool}) == len(pool)
    seen, serial, hits = {}, 0, 0
    for keys in _steps(rng, pool, [1, 17, 300, 40, 300, 3]):
        payloads = list(range(serial, serial + len(keys)))  # the payload of row i of this step, were it to run
        serial += len(keys)
        out, miss = EC.run_step(table, keys, lambda m: [payloads[i] for i in m])
        fresh = {}
        for i, k in enumerate(keys):
            if k in seen:
                assert out[i] == seen[k] and i not in miss
                hits += 1
            else:
                assert out[i] == payloads[i] and i in miss
                if len(k[1]) <= EC.CACHE_MAXM:
                    fresh.setdefault(k, payloads[i])
        seen.update(fresh)
    assert hits > 100 and table.hits == hits and table.stores == len(seen) and table.probes == serial
    assert not any(len(k[1]) > EC.CACHE_MAXM for k in seen)


def test_step_rule_against_an_entry_dictionary():
    """64 entries: the table against a dictionary entry -> (key, payload) written in reverse list order, so that
    the earliest miss of a step on an entry is what stays."""
    rng = random.Random(6)
    pool = _random_pool(rng, 150)
    table = EC.Table(64)
    assert len({table.index(k) for k in pool}) < len(pool)
    model, serial, hits, replaced = {}, 0, 0, 0
    for keys in _steps(rng, pool, [1, 17, 300, 17, 64, 300, 5]):
        payloads = list(range(serial, serial + len(keys)))
        serial += len(keys)
        out, miss = EC.run_step(table, keys, lambda m: [payloads[i] for i in m])
        before = dict(model)
        for i in reversed(range(len(keys))):
            k = keys[i]
            e = before.get(table.index(k))
            if len(k[1]) <= EC.CACHE_MAXM and e is not None and e[0] == k:
                assert out[i] == e[1] and i not in miss
                hits += 1
            else:
                assert out[i] == payloads[i] and i in miss
                if len(k[1]) <= EC.CACHE_MAXM:
                    replaced += table.index(k) in before and before[table.index(k)][0] != k
                    model[table.index(k)] = (k, payloads[i])
        assert {i: e for i, e in enumerate(table.slot) if e is not None} == model
    assert hits > 50 and replaced > 50 and table.evicted_reprobed > 0


def test_mirrors_match_the_library():
    L = _lib.lib()
    assert L.kv_sizeof_config() == C.sizeof(_lib.Config)
    assert L.kv_sizeof_stats() == C.sizeof(_lib.Stats)
    names = [n for n, _ in _lib.Config._fields_]
    assert names[-6:] == ["eval_cache", "leaves", "arena", "sample_plies", "sim_groups", "reuse_tree"]
    stats = [n for n, _ in _lib.Stats._fields_]
    k = stats.index("cache_probes")
    assert stats[k - 1:k + 4] == ["arena_rows", "cache_probes", "cache_hits", "cache_stores", "sim_steps"]
    assert _lib.CACHE_MAXM == EC.CACHE_MAXM and _lib.CACHE_ENTRY_BYTES == EC.ENTRY_BYTES
    assert EC.ENTRY_BYTES % 64 == 0 and EC.ENTRY_BYTES >= 64 + 16 + 6 * EC.CACHE_MAXM
    assert "kv_dev_eval_cache" in _lib.EXPORTED and hasattr(L, "kv_dev_eval_cache")


@functools.lru_cache(maxsize=None)
def _restated(name, entries):
    return EC.restate(EC.ARENA_RUN if name == "arena" else EC.RUNS[name], entries, arena=name == "arena")


def test_cached_driver_plays_play_many_games():
    """Without a table the driver is play_many; with one, the games and the batches' pending rows stay the same."""
    for name in ("class_edge", "arena"):
        cfg = EC.ARENA_RUN if name == "arena" else EC.RUNS[name]
        gids = [cfg["base"] + k for k in range(cfg["n_games"])]
        want, winfo = SL.play_many([SL.SEED + g for g in gids], gids, cfg["sims"], cfg["plies"], cfg["leaves"],
                                   EC._hash_many, EC._hash_many_b, arena=name == "arena")
        off, oinfo, ocaches = EC.restate(cfg, 0, arena=name == "arena")
        assert off == want and oinfo == winfo
        assert all(c.table.hits == 0 and c.table.stores == 0 for c in ocaches)
        assert sum(c.table.probes for c in ocaches) == sum(winfo["pending"])
        for entries in (64, 1 << 16):
            on, info, caches = _restated(name, entries)
            assert on == want and info == winfo
            assert sum(c.table.hits for c in caches) > 0
            for c in caches:
                assert c.table.probes == sum(n for n, _ in c.steps)
                assert c.table.probes - c.table.hits == sum(len(m) for _, m in c.steps)


def test_the_runs_hold_the_cases_the_gpu_comparison_needs():
    tot = {e: dict(hits=0, dup=0, emptied=0, cut=0, reprobed=0) for e in (64, 1 << 16)}
    for entries, t in tot.items():
        for name in sorted(EC.RUNS) + ["arena"]:
            _, info, caches = _restated(name, entries)
            for c in caches[:2 if name == "arena" else 1]:
                print(f"{name} eval_cache {entries}: probes {c.table.probes} hits {c.table.hits} stores "
                      f"{c.table.stores} batch rows {c.batch_rows} duplicate steps {c.dup_steps} emptied lists "
                      f"{c.emptied} lists cut below 17 {c.cut_below_class} evicted keys probed again "
                      f"{c.table.evicted_reprobed}")
                assert c.table.hits > 0, name  # every run and player gives the device something to hit
                t["hits"] += c.table.hits
                t["dup"] += c.dup_steps
                t["emptied"] += c.emptied
                t["cut"] += c.cut_below_class and c.pad_to == EC.CLASS_ROWS
                t["reprobed"] += c.table.evicted_reprobed
    for entries, t in tot.items():
        assert t["hits"] > 0 and t["dup"] > 0, (entries, t)  # a hit; two equal rows in one step
    assert tot[1 << 16]["emptied"] > 0  # a step whose list the hits empty
    assert tot[64]["cut"] > 0 and tot[1 << 16]["cut"] > 0  # a list cut below 17 rows in the larger class
    assert tot[64]["reprobed"] > 0  # 64 entries: an evicted key is probed again later
    assert EC.RUNS["tail"]["n_games"] == EC.RUNS["tail"]["slots"] == 18  # no run recycles a slot
    assert all(cfg["n_games"] == cfg["slots"] for cfg in EC.RUNS.values())


# ---- recycling: more games than slots (tests/_mcts_starts.RECYCLE)
class _Unbounded(EC.Table):
    """A dictionary in the table's place: every key its own entry, nothing ever replaced."""

    def __init__(self):
        super().__init__(0)
        self.entries, self.slot = 1, {}

    def index(self, key):
        return key

    def probe(self, key):
        self.probes += 1
        if len(key[1]) <= EC.CACHE_MAXM and key in self.slot:
            self.hits += 1
            return self.slot[key]
        return None

    def store(self, key, payload):
        self.slot[key] = payload
        self.stores += 1


def _moves_of(games):
    return [[x["move"] for x in g] for g in games], [[x["visits"] for x in g] for g in games]


def test_recycling_the_cached_driver_plays_the_uncached_games():
    from tests import _mcts_starts as ST
    cfg = ST.RECYCLE
    n, slots = cfg["n_games"], cfg["slots"]
    ref = ST.leaves_run(ST.SEED, ST.N_GAMES, ST.SIMS, cfg["leaves"])[:n]
    starts, slot_of, ties = ST.recycling_seating()
    assert ties == 0  # no two slots freed in one ply-step: the seating is the device's, whatever its atomics do
    assert starts == SL.starts_of([r["plies"] for r in ref], slots, [r["holds"] for r in ref])
    assert slot_of[:slots] == list(range(slots)) and set(slot_of) == set(range(slots)) and max(starts) > 100
    # the sim-steps of a ply-step are those of its slowest game
    per_step = {}
    for r, t0 in zip(ref, starts):
        for p, k in enumerate(r["steps"]):
            per_step[t0 + p] = max(per_step.get(t0 + p, 0), k)
    for entries in (cfg["small"], cfg["large"]):
        games, info, cache = ST.cached_recycling_run(entries)
        assert _moves_of(games) == ([r["moves"] for r in ref], [r["visits"] for r in ref]), entries
        assert [g.result for g in games] == [(r["plies"], r["outcome"], r["reason"], r["reward"]) for r in ref]
        t = cache.table
        assert t.probes == sum(info["pending"]) == sum(r["n_evals"] - r["plies"] for r in ref)
        assert 0 < t.hits < t.probes and t.hits + t.stores <= t.probes and info["steps"] == sum(per_step.values())
        print(f"entries {entries}: probes / hits / stores {t.probes} / {t.hits} / {t.stores}, contests "
              f"{cache.contests}, hits on another game's entry {sum(a != b for a, b in cache.hits_from)}")
        assert cache.contests >= 1  # two misses of one step on one entry: the earlier in slot order is stored
    # the large table: a game in a recycled slot hits an entry that an earlier game stored
    late = [(a, b) for a, b in ST.cached_recycling_run(cfg["large"])[2].hits_from if a >= slots and b < a]
    assert late and (19, 0) in late  # game 19 starts where game 0 started
    assert ST.cached_recycling_run(cfg["small"])[0] is not ST.cached_recycling_run(cfg["large"])[0]


def test_recycling_hits_against_an_unbounded_dictionary():
    """A table large enough that no probed key had been replaced counts the dictionary's hits."""
    from tests import _mcts_starts as ST
    games, info, big = ST.recycling_run(1 << 24)
    again, info_d, model = ST.recycling_run(0, table=_Unbounded())
    assert _moves_of(games) == _moves_of(again) and info == info_d
    assert big.table.evicted_reprobed == 0
    assert (big.table.probes, big.table.hits) == (model.table.probes, model.table.hits)
    print(f"probes / hits {model.table.probes} / {model.table.hits}, keys {len(model.table.slot)}")
    assert model.table.hits > 100 and sum(a != b for a, b in model.hits_from) > 0
    assert big.hits_from == model.hits_from
