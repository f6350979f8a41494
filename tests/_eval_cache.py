"""Plain-Python restatement of the evaluation cache (kv_config.eval_cache, DESIGN.md "Evaluation cache";
knightvision_amd/csrc/kv_cache.hip): the hash, the direct-mapped table, the rule of one sim-step, and a driver that
plays tests/_mcts_selfplay_leaves' games with the step batches behind a cache per player -- also with more games
than slots, where a recycled slot's new game finds the entries the finished games stored.

Semantics, as include/kv.h states them:

* The key of a row is its network input and nothing else: the 64 board codes, the move count n and the n move
  words. A hit needs every byte of it equal; the hash only picks the entry.
* h = XOR_k mix64((k + 1) * 0x9E3779B97F4A7C15 ^ w_k) over the key's 16-bit words w_k -- k < 32 the board's byte
  pairs (little endian), k = 32 the count, k = 33 + j move word j -- mix64 the splitmix64 finaliser; the entry is
  h & (entries - 1).
* The payload is the n legal logits and the value as bits.
* One sim-step: every pending row is probed against the table as the step found it; the hits take the stored
  payload and leave the list; the misses run, in list order; then the misses are stored -- a store replaces the
  entry, of several misses on one entry the earliest in the list is stored, a row of more than CACHE_MAXM moves
  is never stored. Two equal rows of one step both miss and both run.

Shared by tests/test_eval_cache_cpu.py and tests/test_eval_cache_gpu.py; not a test module itself."""
import numpy as np

from oracle import oracle as O

from tests import _mcts_search as S
from tests import _mcts_selfplay_leaves as SL

F = np.float32
MAXM = 320        # KV_MAXM
CACHE_MAXM = 96   # KV_CACHE_MAXM
ENTRY_BYTES = 704  # KV_CACHE_ENTRY_BYTES
CLASS_ROWS = 17   # the smallest batch of the > 16-board class
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix64(z):
    """The splitmix64 finaliser."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def make_key(board, words):
    """A row's key: (the 64 board codes as bytes, the n move words as a tuple); n is the tuple's length."""
    b = np.asarray(board, dtype=np.int8).reshape(64).tobytes()
    return b, tuple(int(w) & 0xFFFF for w in words)


def key_words(key):
    """The key as 16-bit words: 32 board byte pairs, n, the move words."""
    b, words = key
    return [b[2 * k] | (b[2 * k + 1] << 8) for k in range(32)] + [len(words) & 0xFFFF] + list(words)


def key_hash(key):
    h = 0
    for k, w in enumerate(key_words(key)):
        h ^= mix64((((k + 1) * GOLD) & M64) ^ w)
    return h


class Table:
    """The direct-mapped table of one network: entries a power of two, slot[i] = (key, payload) or None; 0 entries:
    no cache (every probe misses, nothing is stored). Counts probes, hits and stores as the device does, and for
    the coverage conditions the keys a store evicted and the probes that met such a key again."""

    def __init__(self, entries):
        assert entries == 0 or (entries & (entries - 1)) == 0
        self.entries = entries
        self.slot = [None] * entries
        self.probes = self.hits = self.stores = 0
        self.evicted, self.evicted_reprobed = set(), 0

    def index(self, key):
        return key_hash(key) & (self.entries - 1)

    def probe(self, key):
        """-> the payload stored under exactly this key, or None."""
        self.probes += 1
        if self.entries == 0 or len(key[1]) > CACHE_MAXM:
            return None
        e = self.slot[self.index(key)]
        if e is not None and e[0] == key:
            self.hits += 1
            return e[1]
        if key in self.evicted:
            self.evicted_reprobed += 1
        return None

    def store(self, key, payload):
        i = self.index(key)
        if self.slot[i] is not None and self.slot[i][0] != key:
            self.evicted.add(self.slot[i][0])
        self.slot[i] = (key, payload)
        self.stores += 1

    def clear(self):
        self.slot = [None] * self.entries


def run_step(table, keys, run_misses, log=None):
    """One sim-step on one table. keys: the step's pending rows in list order; run_misses(list of their indices)
    -> one payload per missed row (the network). -> (payload per row, the missed indices). log: a dict that
    takes the rule's own account of the step -- stored: the indices whose rows were stored, lost: the misses that
    lost their entry to an earlier miss of the list."""
    found = [table.probe(k) for k in keys]
    miss = [i for i, p in enumerate(found) if p is None]
    out = list(found)
    claimed, lost = {}, []
    for i, p in zip(miss, run_misses(miss) if miss else []):
        out[i] = p
        if table.entries and len(keys[i][1]) <= CACHE_MAXM:
            if claimed.setdefault(table.index(keys[i]), i) != i:  # the earliest miss of the list on an entry
                lost.append(i)
    for i in sorted(claimed.values()):
        table.store(keys[i], out[i])
    if log is not None:
        log.update(stored=sorted(claimed.values()), lost=lost)
    return out, miss


def state_key(state):
    """The key of a leaf position as the games hand it out (a state after getValidMoves) -> (key, move words)."""
    moves3, st = O.valid_moves(state)
    assert np.array_equal(np.asarray(st), np.asarray(state)), "getValidMoves changes a position it has left"
    words = S.move_words(st, moves3)
    return make_key(st[:64], words), words


class CachedEval:
    """evaluate_many (a play_many evaluator: list of states -> list of (logits[4096], value)) behind a Table.
    roots(): the root batches, uncached. leaves(): one step's batch under run_step; a hit's row is rebuilt from
    the payload alone (the legal moves' logits, every other logit 0). pad_to: the rows a short non-empty list is
    padded to (17 in the > 16-row class, else 0). Logs per step the missed indices, and the totals."""

    def __init__(self, evaluate_many, entries, pad_to):
        self.ev, self.table, self.pad_to = evaluate_many, Table(entries), pad_to
        self.steps = []          # per leaves() call: (rows of the list, the missed indices)
        self.batch_rows = 0      # the padded miss lists, summed
        self.dup_steps = 0       # steps that held two equal rows
        self.emptied = 0         # non-empty lists the hits emptied
        self.cut_below_class = 0  # lists of >= 17 rows cut to 1 .. 16 misses
        self.row_games = None    # set by play_many_cached before a leaves() call: the game of each row
        self.stored_by = {}      # key -> the game whose row was stored under it last
        self.hits_from = []      # per hit of a tagged list: (the probing game, the game that stored the entry)
        self.contests = 0        # misses that lost an entry to an earlier miss of their step

    def roots(self, states):
        return self.ev(states)

    def leaves(self, states):
        if not states:
            return []
        kw = [state_key(st) for st in states]
        keys = [k for k, _ in kw]

        def run(miss):
            rows = self.ev([states[i] for i in miss])
            return [(tuple(np.asarray(lg, dtype=F)[[S.policy_index(w) for w in kw[i][1]]].view(np.uint32).tolist()),
                     int(np.asarray(v, dtype=F).view(np.uint32))) for i, (lg, v) in zip(miss, rows)]

        log = {}
        out, miss = run_step(self.table, keys, run, log)
        self.steps.append((len(states), miss))
        self.contests += len(log["lost"])
        tags, self.row_games = self.row_games, None
        if tags is not None:
            assert len(tags) == len(keys)
            self.hits_from += [(tags[i], self.stored_by[keys[i]]) for i in range(len(keys)) if i not in miss]
            self.stored_by.update((keys[i], tags[i]) for i in log["stored"])
        m = len(miss)
        self.batch_rows += self.pad_to if 0 < m < self.pad_to else m
        self.dup_steps += len(set(keys)) < len(keys)
        self.emptied += m == 0
        self.cut_below_class += len(states) >= CLASS_ROWS and 0 < m < CLASS_ROWS
        rows = []
        for (_, words), (lbits, vbits) in zip(kw, out):
            lg = np.zeros(4096, dtype=F)
            lg[[S.policy_index(w) for w in words]] = np.array(lbits, dtype=np.uint32).view(F)
            rows.append((lg, np.array(vbits, dtype=np.uint32).view(F)[()]))
        return rows


def seating(holds, slots):
    """Where and when each game of a recycling run sits: the first `slots` games take slots 0 .. slots - 1 at
    ply-step 0, every later id the slot that is free first (tests/_mcts_selfplay_leaves.starts_of; holds: the
    ply-steps each game keeps its slot). -> (starts, slot_of, ties): ties counts the later games that found more
    than one slot freed in the same ply-step -- on the device those slots draw their ids in no fixed order
    (k_finish's atomic counter), so only a run without ties has one seating."""
    free = [(0, i) for i in range(slots)]
    starts, slot_of, ties = [], [], 0
    for g, n in enumerate(holds):
        t, i = min(free)
        if g >= slots and sum(1 for ft, _ in free if ft == t) > 1:
            ties += 1
        free.remove((t, i))
        starts.append(t)
        slot_of.append(i)
        free.append((t + n, i))
    return starts, slot_of, ties


def play_many_cached(seeds, gids, sims, plies, leaves, cache_a, cache_b=None, per_game=None, starts=None,
                     slot_of=None, **kw):
    """tests/_mcts_selfplay_leaves.play_many, the root batches through cache_x.roots and every step's batch
    through cache_x.leaves. per_game: one dict of further SL.game keywords per game (its start position).
    starts / slot_of (seating): the ply-step each game begins at and the engine slot it sits in -- more games than
    slots; a step's list is in slot order, which is game order only while no slot has been recycled. Without them
    every game starts at ply-step 0 in the slot of its index.
    -> (per-game outputs, dict(steps, pending: [A's, B's], batches: per sim-step the (A's, B's) pending rows))."""
    per_game = per_game or [{}] * len(seeds)
    gens = [SL.game(s, g, sims, n, leaves, **kw, **pg) for s, g, n, pg in zip(seeds, gids, plies, per_game)]
    ev = (cache_a, cache_b or cache_a)
    starts = list(starts) if starts is not None else [0] * len(gens)
    slot_of = list(slot_of) if slot_of is not None else list(range(len(gens)))
    out, req = [None] * len(gens), {}
    info = dict(steps=0, pending=[0, 0], batches=[])

    def by_slot(ks):
        ks = sorted(ks, key=lambda k: slot_of[k])
        assert len({slot_of[k] for k in ks}) == len(ks), "two games in one slot"
        return ks

    def advance(k, val=None):
        try:
            req[k] = next(gens[k]) if val is None else gens[k].send(val)
        except StopIteration as done:
            out[k] = done.value
            req.pop(k, None)

    eply = 0
    while req or any(s >= eply for s in starts):
        for k, s in enumerate(starts):
            if s == eply:
                advance(k)
        assert all(kind == "root" for kind, _, _ in req.values())
        for x in (SL.A, SL.B):
            ks = by_slot(k for k in req if req[k][1] == x)
            if ks:
                for k, row in zip(ks, ev[x].roots([req[k][2] for k in ks])):
                    advance(k, row)
        while True:
            stepping = by_slot(k for k in req if req[k][0] == "step")
            if not stepping:
                break
            info["steps"] += 1
            got, counts = {k: [] for k in stepping}, [0, 0]
            for x in (SL.A, SL.B):
                ks = [k for k in stepping if req[k][1] == x]
                states = [st for k in ks for st in req[k][2]]
                counts[x] = len(states)
                ev[x].row_games = [k for k in ks for _ in req[k][2]]
                rows = iter(ev[x].leaves(states))
                for k in ks:
                    got[k] = [next(rows) for _ in req[k][2]]
            info["pending"][SL.A] += counts[SL.A]
            info["pending"][SL.B] += counts[SL.B]
            info["batches"].append(tuple(counts))
            for k in stepping:
                advance(k, got[k])
        eply += 1
    return out, info


# The hash-evaluator runs of the cache tests: tests/_mcts_selfplay_leaves.HASH_RUNS without recycling ("tail" cut to
# n_games = slots = 18). tests/test_eval_cache_cpu.py asserts that they hold the cases the GPU comparison needs.
RUNS = {name: dict(cfg) for name, cfg in SL.HASH_RUNS.items()}
RUNS["tail"].update(n_games=18, plies=(8,) * 18)
ARENA_RUN = dict(slots=12, n_games=12, base=0, sims=22, leaves=4, max_moves=4, plies=(4,) * 12)


def _hash_many(states):
    return [SL.hash_eval(st) for st in states]


def _hash_many_b(states):
    return [SL.hash_eval_b(st) for st in states]


def restate(cfg, entries, arena=False):
    """A hash-evaluator run of RUNS / ARENA_RUN with eval_cache = entries -> (games, info, [cache A, cache B])."""
    pad_to = CLASS_ROWS if cfg["slots"] * cfg["leaves"] > 16 else 0
    caches = [CachedEval(_hash_many, entries, pad_to), CachedEval(_hash_many_b, entries, pad_to)]
    gids = [cfg["base"] + k for k in range(cfg["n_games"])]
    games, info = play_many_cached([SL.SEED + g for g in gids], gids, cfg["sims"], cfg["plies"], cfg["leaves"],
                                   caches[0], caches[1] if arena else None, arena=arena)
    return games, info, caches
