"""Self-play, arena and game endings from set start positions (kv_dev_set_starts; start_game, k_init and k_finish
in knightvision_amd/csrc/kv_engine.hip) through the C ABI: the self-play kernels on mates by either colour,
stalemates, kings-only draws, games of 0 plies, resignations, black to move at ply 0, roots wider than a wavefront
and special moves at the root -- none of which a game from the initial position reaches in a few plies.

Every comparison is exact (hash evaluator: integer and dyadic paths; real network: the oracle is fed the HIP
network's own rows). The games are those of tests/_mcts_starts.py: game g starts from the set's position
g % 19 and is seeded SEED + g; tests/test_starts_cpu.py asserts what they hold and pins the references'
termination to the C oracle. Each test prints its engine time."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from knightvision_amd import _lib, arena
from knightvision_amd import engine as engine_mod
from knightvision_amd.engine import EVAL_HASH, GAME_DTYPE, SEED_SEQUENTIAL, SelfPlayEngine, records_by_game
from knightvision_amd.weights import synthetic_state_dict
from oracle import oracle as O

from tests import _eval_cache as EC
from tests import _mcts_arena as AR
from tests import _mcts_starts as ST
from tests._mcts_network import CLASS_ROWS, count_ties, hip_eval

pytestmark = pytest.mark.gpu

SEED, N, SIMS, THIRD = ST.SEED, ST.N_GAMES, ST.SIMS, ST.SLOTS_THIRD
PARTS = ("records", "root visits", "root moves", "game table")


@functools.lru_cache(maxsize=None)
def _run(slots, leaves=0, reuse=False, arena=False, sample_plies=0, sim_groups=0, eval_cache=0, n_games=N, base=0,
         stride=1, starts=True):
    """One hash-evaluator engine run from the set -> (records, root visits, root move words, games, stats)."""
    sd = synthetic_state_dict(42, "init")
    t0 = time.perf_counter()
    with SelfPlayEngine(sd, opponent=sd if arena else None, slots=slots, n_games=n_games, seed=SEED,
                        max_moves=ST.MAX_MOVES, sims=SIMS, c_puct=ST.C_PUCT, eps=ST.EPS, alpha=ST.ALPHA,
                        keep_root_moves=True, leaves=leaves, reuse_tree=reuse, sample_plies=sample_plies,
                        sim_groups=sim_groups, eval_cache=eval_cache, game_id_base=base, game_id_stride=stride,
                        eval_mode=EVAL_HASH) as eng:
        if starts:
            eng._set_starts(ST.start_list())
        t1 = time.perf_counter()
        eng.run()
        out = eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()
    print(f"engine run (slots {slots}, leaves {leaves}, reuse {reuse}, arena {arena}, sample_plies {sample_plies}, "
          f"groups {sim_groups}, cache {eval_cache}): create {t1 - t0:.2f} s, run {time.perf_counter() - t1:.2f} s")
    return out


def _same_games(run, ref, gids=None, reuse=False):
    """An engine run against the references' games: records (board and move per ply), the kv_game rows in full,
    the root_visits / root_moves rows with their padding, and the stats identities."""
    recs, visits, words, games, st = run
    gids = list(range(len(ref))) if gids is None else list(gids)
    assert sorted(games["game_id"].tolist()) == gids
    row = {int(g["game_id"]): g for g in games}
    for gid, r in zip(gids, ref):
        g = row[gid]
        got = (int(g["plies"]), int(g["outcome"]), float(g["reward"]), int(g["reason"]), int(g["n_evals"]))
        print(f"game {gid} ({ST.NAMES[gid % len(ST.NAMES)]}): plies, outcome, reward, reason, n_evals {got}")
        assert got == (r["plies"], r["outcome"], r["reward"], r["reason"], r["n_evals"]), gid
        sel = recs["game_id"] == gid
        assert sel.sum() == r["plies"] and recs["ply"][sel].tolist() == list(range(r["plies"])), gid
        assert recs["move"][sel].tolist() == r["moves"], gid
        assert [bytes(b) for b in recs["board"][sel]] == r["boards"], gid
        for p in range(r["plies"]):
            n = len(r["visits"][p])
            assert visits[sel][p][:n].tolist() == r["visits"][p] and (visits[sel][p][n:] == -1).all(), (gid, p)
            assert words[sel][p][:n].tolist() == r["words"][p] and (words[sel][p][n:] == 0xffff).all(), (gid, p)
    plies = sum(r["plies"] for r in ref)
    assert len(recs) == len(visits) == len(words) == plies  # a game of 0 plies has no record and no row
    assert st["plies"] == plies and st["games_done"] == len(ref) and st["tree_overflows"] == 0
    assert st["leaf_rows_pending"] == sum(r["n_evals"] for r in ref) - plies
    assert st["nn_rows"] == plies + st["leaf_rows_pending"]
    assert st["sims"] + (st["sims_kept"] if reuse else 0) == plies * SIMS
    if not reuse:
        assert st["sims_kept"] == st["roots_carried"] == 0


def _same_runs(a, b):
    """Two runs game for game: the records, their side rows and the game table (ordered by game id)."""
    for k, part in enumerate(PARTS[:3]):
        assert np.array_equal(a[k], b[k]), part
    ga, gb = np.sort(a[3], order="game_id"), np.sort(b[3], order="game_id")
    assert np.array_equal(ga, gb), PARTS[3]


# ---- 1. one leaf against the C oracle, with and without recycling, drawn moves and first maxima
@pytest.mark.parametrize("sample_plies", [0, -1])
def test_one_leaf_is_the_oracle_whatever_the_slots(sample_plies):
    ref = ST.oracle_run(SEED, N, SIMS, sample_plies)
    full, third = _run(N, sample_plies=sample_plies), _run(THIRD, sample_plies=sample_plies)
    _same_games(full, ref)
    _same_games(third, ref)  # recycling: chains of 0-ply games through one slot
    _same_runs(full, third)
    reasons = {(r["reason"], r["outcome"]) for r in ref}
    print(f"sample_plies {sample_plies}: endings (reason, outcome) {sorted(reasons)}")


def test_the_start_of_a_game_depends_on_its_global_id_alone():
    """game_id_base 5, stride 3: the games with global ids 5, 8, ... start from the set's position id % 19 and are
    seeded SEED + id, as the same ids do in any other run."""
    gids = [5 + 3 * k for k in range(9)]
    run = _run(4, n_games=9, base=5, stride=3)
    want = O.mcts_play_batch(SIMS, [SEED + g for g in gids], max_moves=ST.MAX_MOVES, c_puct=ST.C_PUCT, eps=ST.EPS,
                             alpha=ST.ALPHA, keep_visits=True, starts=[ST.start_of(g) for g in gids])
    row = {int(g["game_id"]): g for g in run[3]}
    assert sorted(row) == gids
    for g, r in zip(gids, want):
        sel = run[0]["game_id"] == g
        assert run[0]["move"][sel].tolist() == r["moves"].tolist(), g
        assert (row[g]["plies"], row[g]["outcome"], row[g]["reason"], row[g]["n_evals"]) == \
            (r["plies"], r["outcome"], r["reason"], r["n_evals"]), g
        for p in range(r["plies"]):
            assert np.array_equal(run[1][sel][p], r["visits"][p]), (g, p)


# ---- 2. several leaves in flight
@pytest.mark.parametrize("leaves", [2, 8])
def test_leaves_end_their_games_as_restated(leaves):
    ref = ST.leaves_run(SEED, N, SIMS, leaves)
    _same_games(_run(N, leaves=leaves), ref)
    _same_games(_run(THIRD, leaves=leaves), ref)
    run = _run(THIRD, leaves=leaves)
    assert run[4]["sim_steps"] >= max(sum(r["steps"]) for r in ref)


# ---- 3. carried subtrees with recycling
def test_reuse_drops_the_tree_of_a_finished_game():
    ref = ST.reuse_run(SEED, N, SIMS)
    for slots in (THIRD, N):
        run = _run(slots, reuse=True)
        _same_games(run, ref, reuse=True)
        assert run[4]["sims_kept"] == sum(sum(r["kept"]) for r in ref)
        assert run[4]["roots_carried"] == sum(sum(r["carried"]) for r in ref)
    assert any(sum(r["carried"]) for r in ref)


# ---- 4. arena
@pytest.mark.parametrize("leaves", [1, 4])
def test_arena_attributes_decisive_games(leaves):
    ref = ST.arena_run(SEED, N, SIMS) if leaves == 1 else ST.leaves_run(SEED, N, SIMS, leaves, 0, True)
    run = _run(THIRD, leaves=leaves, arena=True)
    _same_games(run, ref)
    _same_games(_run(N, leaves=leaves, arena=True), ref)
    assert run[4]["arena_rows"][0] > 0 and run[4]["arena_rows"][1] > 0
    black_first = [g for g, r in enumerate(ref) if r["plies"] and not ST.start_of(g)[64]]
    assert black_first and all(ref[g]["players"][0] == (1 if g % 2 == 0 else 0) for g in black_first)


@pytest.mark.parametrize("leaves", [1, 4])
def test_play_match_scores_the_restated_games(leaves, monkeypatch):
    class FromTheSet(SelfPlayEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self._set_starts(ST.start_list())

    monkeypatch.setattr(engine_mod, "SelfPlayEngine", FromTheSet)
    sd = synthetic_state_dict(42, "init")
    t0 = time.perf_counter()
    got = arena.play_match(sd, sd, N, sims=SIMS, slots=THIRD, seed=SEED, max_moves=ST.MAX_MOVES, eps=ST.EPS,
                           alpha=ST.ALPHA, sample_plies=0, c_puct=ST.C_PUCT, eval_mode=EVAL_HASH, leaves=leaves)
    print(f"play_match: {time.perf_counter() - t0:.2f} s")
    ref = ST.arena_run(SEED, N, SIMS) if leaves == 1 else ST.leaves_run(SEED, N, SIMS, leaves, 0, True)
    a_res = [r["outcome"] if g % 2 == 0 else -r["outcome"] for g, r in enumerate(ref)]
    wins, draws, losses = a_res.count(1), a_res.count(0), a_res.count(-1)
    assert wins > 0 and losses > 0 and draws > 0
    score = (wins + draws / 2) / N
    reasons = {}
    for r in ref:
        name = engine_mod.REASONS[r["reason"]]
        reasons[name] = reasons.get(name, 0) + 1
    print(f"A: +{wins} ={draws} -{losses}, score {score:.4f}, reasons {reasons}")
    assert (got["games"], got["wins"], got["draws"], got["losses"]) == (N, wins, draws, losses)
    assert got["score"] == score and got["elo"] == arena.elo_of(score) and got["reasons"] == reasons
    white = [r["outcome"] for g, r in enumerate(ref) if g % 2 == 0]
    black = [-r["outcome"] for g, r in enumerate(ref) if g % 2 == 1]
    assert got["as_white"] == (white.count(1), white.count(0), white.count(-1))
    assert got["as_black"] == (black.count(1), black.count(0), black.count(-1))
    table = np.zeros(N, dtype=GAME_DTYPE)
    for g, r in enumerate(ref):
        table[g] = (g, r["plies"], r["outcome"], r["reward"], r["reason"], r["n_evals"], 0)
    assert np.array_equal(np.sort(got["game_table"], order="game_id"), table)


# ---- 5. two slot groups
def test_two_slot_groups_play_the_same_games():
    one, two = _run(34, sim_groups=1), _run(34, sim_groups=2)
    _same_runs(one, two)
    _same_games(two, ST.oracle_run(SEED, N, SIMS, 0))
    for key in ("plies", "sims", "nn_rows", "leaf_rows_pending", "games_done"):
        assert one[4][key] == two[4][key], key


# ---- 6. the evaluation cache
@pytest.mark.parametrize("entries", [64, 1 << 12])
def test_the_eval_cache_changes_nothing_and_counts_as_restated(entries):
    off, on = _run(N, leaves=2), _run(N, leaves=2, eval_cache=entries)
    _same_runs(off, on)
    for key in ("plies", "sims", "nn_rows", "leaf_rows_pending", "sim_steps", "games_done"):
        assert on[4][key] == off[4][key], key
    cache = EC.CachedEval(EC._hash_many, entries, CLASS_ROWS)
    wide = []
    probe = cache.table.probe

    def counting_probe(key):
        wide.append(len(key[1]) > EC.CACHE_MAXM)
        return probe(key)

    cache.table.probe = counting_probe
    stored = []
    store = cache.table.store
    cache.table.store = lambda key, payload: (stored.append(len(key[1])), store(key, payload))[1]
    games, info = EC.play_many_cached([SEED + g for g in range(N)], list(range(N)), SIMS, [None] * N, 2, cache,
                                      per_game=[dict(start=ST.start_of(g), max_moves=ST.MAX_MOVES) for g in range(N)],
                                      eps=ST.EPS)
    ref = ST.leaves_run(SEED, N, SIMS, 2)
    assert [[x["move"] for x in g] for g in games] == [r["moves"] for r in ref]  # hits rebuild the rows exactly
    t = cache.table
    print(f"eval_cache {entries}: probes / hits / stores {on[4]['cache_probes']} / {on[4]['cache_hits']} / "
          f"{on[4]['cache_stores']} (restated {t.probes} / {t.hits} / {t.stores}), rows wider than "
          f"{EC.CACHE_MAXM} moves probed {sum(wide)}")
    assert (on[4]["cache_probes"], on[4]["cache_hits"], on[4]["cache_stores"]) == (t.probes, t.hits, t.stores)
    assert t.probes == on[4]["leaf_rows_pending"] and sum(wide) > 0 and max(stored) <= EC.CACHE_MAXM
    assert on[4]["sim_steps"] == info["steps"]


# ---- 7. the reference move selection (sims 0)
def test_the_reference_path_from_the_set():
    from oracle import torch_ref
    sd = synthetic_state_dict(42, "init")
    n = len(ST.NAMES)
    t0 = time.perf_counter()
    with SelfPlayEngine(sd, slots=n, n_games=n, seed=SEED, max_moves=ST.MAX_MOVES, batch=16) as eng:
        eng._set_starts(ST.start_list())
        eng.run()
        recs, games = eng.records(), eng.games()
    print(f"reference path, {n} games: {time.perf_counter() - t0:.2f} s")
    by = records_by_game(recs, games)
    row = {int(g["game_id"]): g for g in games}
    ev = torch_ref.make_eval_fn(sd)
    assert sorted(row) == list(range(n))
    for g in range(n):
        r = O.play_game(ev, O.MT(SEED + g, "numpy"), O.MT(SEED + g, "python"), O.Last(), max_moves=ST.MAX_MOVES,
                        batch=16, softmax_fn=torch_ref.torch_softmax, start=ST.start_of(g))
        moves, boards = by[g][:2] if g in by else (np.zeros(0, dtype=np.uint16), np.zeros((0, 64), dtype=np.int8))
        print(f"game {g} ({ST.NAMES[g]}): plies {r['plies']} reason {r['reason']} outcome {r['outcome']}")
        assert np.array_equal(moves, r["moves"]), g
        assert np.array_equal(np.asarray(boards).reshape(-1, 64), r["states"][:, :64]), g
        assert (row[g]["plies"], row[g]["outcome"], row[g]["reason"], row[g]["n_evals"]) == \
            (r["plies"], r["outcome"], r["reason"], len(r["eval_sizes"])), g
        assert float(row[g]["reward"]) == pytest.approx(r["reward"])


def test_sequential_games_around_a_game_of_no_plies():
    """KV_SEED_SEQUENTIAL: one pair of streams and the evaluated row carried from game to game; the second game has
    no legal move, so it appends nothing, flushes nothing and leaves the carried row to the third."""
    from oracle import torch_ref
    sd = synthetic_state_dict(42, "init")
    starts = [ST.MATE_IN_ONE, ST.CHECKMATED_ROOT, ST.KPH, ST.BQ]
    t0 = time.perf_counter()
    with SelfPlayEngine(sd, slots=1, n_games=4, seed=SEED, seed_mode=SEED_SEQUENTIAL, max_moves=ST.MAX_MOVES,
                        batch=16) as eng:
        eng._set_starts(np.stack(starts))
        eng.run()
        recs, games = eng.records(), eng.games()
    print(f"sequential run: {time.perf_counter() - t0:.2f} s")
    ev = torch_ref.make_eval_fn(sd)
    np_mt, py_mt, last = O.MT(SEED, "numpy"), O.MT(SEED, "python"), O.Last()
    row = {int(g["game_id"]): g for g in games}
    assert sorted(row) == [0, 1, 2, 3]
    played = 0
    for g, start in enumerate(starts):
        r = O.play_game(ev, np_mt, py_mt, last, max_moves=ST.MAX_MOVES, batch=16, softmax_fn=torch_ref.torch_softmax,
                        start=start)
        sel = recs["game_id"] == g
        print(f"game {g}: plies {r['plies']} reason {r['reason']} evals {r['eval_sizes'].tolist()}")
        assert recs["move"][sel].tolist() == r["moves"].tolist(), g
        assert np.array_equal(recs["board"][sel], r["states"][:, :64]), g
        assert (row[g]["plies"], row[g]["outcome"], row[g]["reason"], row[g]["n_evals"]) == \
            (r["plies"], r["outcome"], r["reason"], len(r["eval_sizes"])), g
        played += r["plies"] > 0
    assert row[1]["plies"] == 0 and row[1]["n_evals"] == 0 and row[0]["plies"] > 0 and played == 3


# ---- 8. the real network (every oracle leaf is a 17-row forward of its own: 12 plies keep the test at seconds;
# the set's mates, stalemates, 0-ply games and kings-only draws all end sooner)
NET_MAX_MOVES = 12


def test_the_real_network_from_the_set():
    sd = synthetic_state_dict(42, "peaked")
    n = CLASS_ROWS
    t0 = time.perf_counter()
    with SelfPlayEngine(sd, slots=n, n_games=n, seed=SEED, max_moves=NET_MAX_MOVES, sims=SIMS, c_puct=ST.C_PUCT,
                        keep_root_visits=True) as eng:
        eng._set_starts(ST.start_list())
        eng.run()
        recs, visits, games, st = eng.records(), eng.root_visits(), eng.games(), eng.stats()
    print(f"real network, {n} games: {time.perf_counter() - t0:.2f} s, {len(recs)} plies")
    assert st["tree_overflows"] == 0 and len(games) == n
    ev, net = hip_eval(sd)
    ref = {}

    def play(g, plies):
        ref[g] = O.mcts_play_game(SIMS, O.MT(SEED + g, "numpy"), O.MT(SEED + g, "python"), ev,
                                  max_moves=NET_MAX_MOVES, c_puct=ST.C_PUCT, start=ST.start_of(g))
        return ref[g]

    compared, ties = count_ties("peaked", recs, visits, range(n), play)
    net.close()
    print(f"MCTS network parity from the set: {compared} root visit vectors compared, divergences: {ties}")
    assert ties == 0
    row = {int(g["game_id"]): g for g in games}
    for g in range(n):
        assert (row[g]["plies"], row[g]["outcome"], row[g]["reason"], row[g]["n_evals"]) == \
            (ref[g]["plies"], ref[g]["outcome"], ref[g]["reason"], ref[g]["n_evals"]), g


# ---- 8b. decisive arena games on two different real networks
ARENA_NET = dict(names=("BQ", "MATE_IN_ONE", "BQ", "KPF", "KPH"), n_games=10, sims=64, leaves=2)


def _net_eval_many(net):
    """One player's evaluator: the HIP network's rows of a list of positions as one batch of the > 16-board class
    (10 slots at 2 leaves are 20 rows; a shorter list is padded to 17 with copies of its first row)."""
    import torch

    def ev(states):
        codes = np.stack([np.asarray(st[:64], dtype=np.int8) for st in states])
        n = len(codes)
        if n < CLASS_ROWS:
            codes = np.concatenate([codes, np.repeat(codes[:1], CLASS_ROWS - n, axis=0)])
        pol, val = net.forward_boards(torch.from_numpy(np.ascontiguousarray(codes)).cuda())
        torch.cuda.synchronize()
        pol, val = pol.cpu().numpy(), val.cpu().numpy().reshape(-1)
        return [(pol[k], val[k]) for k in range(n)]

    return ev


def test_two_real_networks_win_and_lose_as_restated():
    """init (A) against peaked (B) at 2 leaves, every move the first maximum of the root visits: mates in one for
    either colour with A white (even ids) and A black (odd ids), beside a few longer draws. B is no function of
    A here (under the hash evaluator it is A with the value negated), so B's rows or B's cache table taken for
    A's change the games. Against tests/_mcts_selfplay_leaves.py fed each net's own HIP rows; with eval_cache the
    games are byte for byte the same and the counters tests/_eval_cache.py's, one table per net."""
    from knightvision_amd.engine import packed_from
    from knightvision_amd.model import KVNet
    from tests import _mcts_selfplay_leaves as SL
    cfg = ARENA_NET
    n, sims, leaves = cfg["n_games"], cfg["sims"], cfg["leaves"]
    starts = [ST.POSITIONS[x] for x in cfg["names"]]
    sd_a, sd_b = synthetic_state_dict(42, "init"), synthetic_state_dict(42, "peaked")
    runs = {}
    for entries in (0, 1 << 12):
        t0 = time.perf_counter()
        with SelfPlayEngine(sd_a, opponent=sd_b, slots=n, n_games=n, seed=SEED, max_moves=NET_MAX_MOVES, sims=sims,
                            c_puct=ST.C_PUCT, eps=ST.EPS, alpha=ST.ALPHA, keep_root_moves=True, leaves=leaves,
                            sample_plies=-1, eval_cache=entries) as eng:
            eng._set_starts(np.stack(starts))
            eng.run()
            runs[entries] = eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()
        print(f"arena init / peaked, {n} games, eval_cache {entries}: {time.perf_counter() - t0:.2f} s")
    off, on = runs[0], runs[1 << 12]
    _same_runs(off, on)
    nets = [KVNet(0, packed_from(sd)) for sd in (sd_a, sd_b)]
    try:
        ev_a, ev_b = (_net_eval_many(net) for net in nets)
        kw = dict(arena=True, sample_plies=-1, c_puct=ST.C_PUCT, eps=ST.EPS, alpha=ST.ALPHA)
        per_game = [dict(start=starts[g % len(starts)], max_moves=NET_MAX_MOVES) for g in range(n)]
        caches = [EC.CachedEval(ev_a, 1 << 12, CLASS_ROWS), EC.CachedEval(ev_b, 1 << 12, CLASS_ROWS)]
        ref, info = EC.play_many_cached([SEED + g for g in range(n)], list(range(n)), sims, [None] * n, leaves,
                                        caches[0], caches[1], per_game=per_game, **kw)
        # the restatement without a cache, for the games that decide the test: each net's rows, nothing stored
        plain = [SL.play_many([SEED + g], [g], sims, [None], leaves, ev_a, ev_b, start=per_game[g]["start"],
                              max_moves=NET_MAX_MOVES, **kw)[0][0] for g in (0, 1, 5, 6)]
    finally:
        for net in nets:
            net.close()
    recs, visits, words, games, st = off
    row = {int(g["game_id"]): g for g in games}
    assert sorted(row) == list(range(n))
    winners = []
    for g, p in enumerate(ref):
        plies, outcome, reason, reward = p.result
        sel = recs["game_id"] == g
        assert recs["move"][sel].tolist() == [x["move"] for x in p], g
        assert [bytes(b) for b in recs["board"][sel]] == [e["board"] for e in p.extra], g
        for k, x in enumerate(p):
            m = len(x["visits"])
            assert visits[sel][k][:m].tolist() == x["visits"] and (visits[sel][k][m:] == -1).all(), (g, k)
            assert words[sel][k][:m].tolist() == x["words"] and (words[sel][k][m:] == 0xffff).all(), (g, k)
        n_evals = len(p) + sum(sum(map(sum, x["leaf_pending"])) for x in p)
        assert (int(row[g]["plies"]), int(row[g]["outcome"]), int(row[g]["reason"]), float(row[g]["reward"]),
                int(row[g]["n_evals"])) == (plies, outcome, reason, reward, n_evals), g
        wtm = int(starts[g % len(starts)][64])
        assert [x["player"] for x in p] == [AR.player_of(g, wtm ^ (k & 1)) for k in range(len(p))], g
        if outcome:
            winners.append((g, "A" if (outcome > 0) == (g % 2 == 0) else "B", "white" if outcome > 0 else "black"))
    for g, p in zip((0, 1, 5, 6), plain):
        assert [x["move"] for x in p] == [x["move"] for x in ref[g]] and p.result == ref[g].result, g
        assert [x["visits"] for x in p] == [x["visits"] for x in ref[g]], g
    print(f"decisive games (id, winner, colour): {winners}")
    assert {w for _, w, _ in winners} == {"A", "B"}  # a win for either player ...
    assert {g % 2 for g, _, _ in winners} == {0, 1}  # ... with A white in some of them and black in others
    got = arena.summarize(np.sort(games, order="game_id"))
    a_res = [p.result[1] if g % 2 == 0 else -p.result[1] for g, p in enumerate(ref)]
    assert (got["wins"], got["draws"], got["losses"]) == (a_res.count(1), a_res.count(0), a_res.count(-1))
    assert got["wins"] >= 1 and got["losses"] >= 1
    # the counters: one table per net, each probed with its own player's rows
    ta, tb = caches[0].table, caches[1].table
    s_on = on[4]
    print(f"cache probes / hits / stores {s_on['cache_probes']} / {s_on['cache_hits']} / {s_on['cache_stores']} "
          f"(restated A {ta.probes} / {ta.hits} / {ta.stores}, B {tb.probes} / {tb.hits} / {tb.stores})")
    assert (s_on["cache_probes"], s_on["cache_hits"], s_on["cache_stores"]) == \
        (ta.probes + tb.probes, ta.hits + tb.hits, ta.stores + tb.stores)
    assert ta.hits > 0 and tb.hits > 0 and s_on["sim_steps"] == info["steps"] == st["sim_steps"]
    assert st["leaf_rows_pending"] == sum(info["pending"]) and min(st["arena_rows"]) > 0


# ---- 9. the entry's refusals
def _set(eng, states, n):
    ptr = None if states is None else np.ascontiguousarray(states, dtype=np.int8).ctypes.data_as(C.POINTER(C.c_int8))
    rc = _lib.lib().kv_dev_set_starts(eng.h, ptr, n)
    return rc, _lib.lib().kv_last_error().decode()


def test_set_starts_refusals():
    sd = synthetic_state_dict(42, "init")
    good = ST.start_list()
    with SelfPlayEngine(sd, slots=2, n_games=2, seed=SEED, max_moves=2, sims=4, eval_mode=EVAL_HASH) as eng:
        for states, n, text in ((good, 0, "0 states with a pointer"), (None, 3, "3 states with NULL"),
                                (good, -1, "-1 states")):
            rc, msg = _set(eng, states, n)
            assert rc == -1 and text in msg, msg
        for at, value in ((3, 13), (3, -1), (64, 2), (65, 8), (68, -1), (75, 8), (76, -2)):
            bad = good.copy()
            bad[1, at] = value
            rc, msg = _set(eng, bad, len(bad))
            assert rc == -1 and "position 1 is not a state vector" in msg, (at, msg)
        bad = good.copy()
        bad[2, 75] = -1  # a row without a column
        bad[2, 76] = 3
        rc, msg = _set(eng, bad, len(bad))
        assert rc == -1 and "position 2 is not a state vector" in msg
        assert _set(eng, good, len(good))[0] == 0  # a refused call left the engine fresh
        eng.run()
        rc, msg = _set(eng, good, len(good))
        assert rc == -1 and "has run self-play (kv_run)" in msg, msg
        rc, msg = _set(eng, None, 0)
        assert rc == -1 and "fresh engine only" in msg, msg
    with engine_mod.PositionSearch(sd, max_positions=2, max_sims=4, eval_mode=EVAL_HASH) as ps:
        ps.search(np.stack([O.initial_state()]), 4)
        rc = _lib.lib().kv_dev_set_starts(ps.h, good.ctypes.data_as(C.POINTER(C.c_int8)), len(good))
        assert rc == -1 and "has searched positions (kv_search)" in _lib.lib().kv_last_error().decode()


def test_null_restores_the_initial_position():
    plain = _run(5, n_games=7, starts=False)
    sd = synthetic_state_dict(42, "init")
    with SelfPlayEngine(sd, slots=5, n_games=7, seed=SEED, max_moves=ST.MAX_MOVES, sims=SIMS, c_puct=ST.C_PUCT,
                        eps=ST.EPS, alpha=ST.ALPHA, keep_root_moves=True, eval_mode=EVAL_HASH) as eng:
        eng._set_starts(ST.start_list())
        eng._set_starts(None)
        eng.run()
        again = eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()
    for k, part in enumerate(PARTS):
        assert np.array_equal(plain[k], again[k]), part
    timings = {"res_conv_ms", "step_ms"}
    assert {k: v for k, v in plain[4].items() if k not in timings} == \
        {k: v for k, v in again[4].items() if k not in timings}
    assert (plain[0]["board"][plain[0]["ply"] == 0] == O.initial_state()[:64]).all()
