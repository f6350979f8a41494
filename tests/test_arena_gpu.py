"""Arena on the GPU (kv_config.arena / sample_plies; k_arena_split and eng_arena_ply in kv_engine.hip) through the
C ABI, against its plain-Python restatement (tests/_mcts_arena.py) and against the self-play engine:

* Hash evaluator (player B's value negated): every PUCT score is bit-reproducible on both sides, so moves, root
  visit vectors and root move words must be identical.
* A = B must be the self-play run byte for byte: every network row is bit-identical inside its batch class, so
  a wrong split, gather, scatter or padding row is the only thing that can change a byte.
* A != B on the real ChessNet: the restatement's evaluators return each net's own HIP rows, evaluated in the
  > 16-board class the engine's batches are in.
* A game does not depend on how the slots split between the nets (17 slots of one colour against 17 + 17), nor
  on whether the two players' chains run on one stream or two.

The engine runs and the restated games are computed once per configuration and shared by the tests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd.engine import EVAL_HASH, EVAL_LAZY, SelfPlayEngine, packed_from
from knightvision_amd.weights import synthetic_state_dict

from tests import _mcts_arena as AR

pytestmark = pytest.mark.gpu

SEED = 49
CLASS_ROWS = 17  # smallest batch of the Winograd (> 16 boards) class


@functools.lru_cache(maxsize=None)
def _run(a, b, slots, n_games, sims, steps, max_moves=None, hash_eval=False, sim_groups=0, sample_plies=0,
         stride=1):
    """One engine run (b None: self-play of a) -> (records, root visits, root move words, games, stats)."""
    opp = None if b is None else synthetic_state_dict(42, b)
    with SelfPlayEngine(synthetic_state_dict(42, a), opponent=opp, slots=slots, n_games=n_games, seed=SEED,
                        max_moves=max_moves, sims=sims, c_puct=1.5, keep_root_moves=True, sim_groups=sim_groups,
                        sample_plies=sample_plies, game_id_stride=stride,
                        eval_mode=EVAL_HASH if hash_eval else 0) as eng:
        eng.run(steps)
        return eng.records(), eng.root_visits(), eng.root_moves(), eng.games(), eng.stats()


_NETS = {}


def _net(variant):
    from knightvision_amd.model import KVNet
    if variant not in _NETS:
        _NETS[variant] = KVNet(0, packed_from(synthetic_state_dict(42, variant)))
    return _NETS[variant]


@pytest.fixture(scope="module", autouse=True)
def _close_nets():
    yield
    while _NETS:
        _NETS.popitem()[1].close()


def _hip_eval_many(variant):
    """One player's evaluator: the HIP network's rows of a list of positions as one batch of the engine's class
    (fewer than 17 positions are padded with copies of the first, as the engine pads a player's list)."""
    net = _net(variant)

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


def _plies_of(run, games):
    return tuple(int((run[0]["game_id"] == g).sum()) for g in games)


@functools.lru_cache(maxsize=None)
def _restated_hash(games, sims, plies, sample_plies=0, same=False):
    """{g: per-ply dicts} under the hash evaluator (same: B is A, a self-play engine)."""
    eb = AR.hash_eval if same else AR.hash_eval_b
    return {g: AR.play(SEED + g, g, sims, n, AR.hash_eval, eb, sample_plies=sample_plies, eps=0.25)
            for g, n in zip(games, plies)}


@functools.lru_cache(maxsize=None)
def _restated_nets(a, b, games, sims, plies):
    return dict(zip(games, AR.play_many([SEED + g for g in games], games, sims, plies, _hip_eval_many(a),
                                        _hip_eval_many(b), eps=0.25)))


def _divergences(run, restated, sims):
    """Plies at which a game's record, root visit vector or root move words differ from the restatement's."""
    recs, visits, words = run[0], run[1], run[2]
    bad = []
    for g, plies in restated.items():
        sel = recs["game_id"] == g
        assert (np.diff(recs["ply"][sel]) == 1).all() and sel.sum() == len(plies)
        for p, ply in enumerate(plies):
            n = len(ply["visits"])
            ok = (recs["move"][sel][p] == ply["move"] and np.array_equal(visits[sel][p][:n], ply["visits"])
                  and (visits[sel][p][n:] == -1).all() and np.array_equal(words[sel][p][:n], ply["words"])
                  and (words[sel][p][n:] == 0xffff).all() and visits[sel][p][:n].sum() == sims)
            if not ok:
                bad.append((g, p))
                print(f"game {g} ply {p} (player {'AB'[ply['player']]}): GPU visits {visits[sel][p][:n]} move "
                      f"{recs['move'][sel][p]}, restated {ply['visits']} move {ply['move']}")
                break  # the games part here
    return bad


def _same_bytes(x, y, what=(0, 1, 2, 3)):
    return all(x[k].tobytes() == y[k].tobytes() for k in what)


def _rows_add_up(st):
    return st["arena_rows"][0] + st["arena_rows"][1] == st["leaf_batch_rows"]


# ---- 1. hash evaluator, the <= 16-board class
def test_hash_games_identical_to_restatement():
    slots, sims, steps = 6, 16, 8
    run = _run("init", "init", slots, slots, sims, steps, hash_eval=True)
    games = tuple(range(slots))
    plies = _plies_of(run, games)
    assert plies == (steps,) * slots
    rest = _restated_hash(games, sims, plies)
    assert _divergences(run, rest, sims) == []
    for p in range(steps):  # both lists non-empty at every step
        assert {rest[g][p]["player"] for g in games} == {0, 1}
    st = run[4]
    assert st["arena_rows"] == (steps * sims * 3, steps * sims * 3) and _rows_add_up(st)  # 3 + 3 slots, no padding
    assert st["plies"] == slots * steps and st["sims"] == slots * steps * sims
    # B's negated value matters: the games are not the self-play games of the hash evaluator
    solo = _run("init", None, slots, slots, sims, steps, hash_eval=True)
    assert solo[4]["arena_rows"] == (0, 0)
    assert not _same_bytes(run, solo, (0, 1))


# ---- 2. A = B is the self-play run, byte for byte
def test_same_weights_is_selfplay_byte_for_byte():
    """18 slots (9 + 9, both batches padded to 17), 22 games of 4 plies: recycled slots and a tail of 4 games."""
    arena = _run("init", "init", 18, 22, 16, -1, max_moves=4)
    solo = _run("init", None, 18, 22, 16, -1, max_moves=4)
    assert len(solo[3]) == 22 and len(solo[0]) == 88
    for k, name in enumerate(("records", "root visits", "root moves", "game table")):
        if arena[k].tobytes() != solo[k].tobytes():
            n = min(len(arena[k]), len(solo[k]))
            first = next((i for i in range(n) if arena[k][i].tobytes() != solo[k][i].tobytes()), n)
            print(f"{name}: {len(arena[k])} arena rows, {len(solo[k])} self-play rows, first difference at row "
                  f"{first}: record {arena[0][min(first, len(arena[0]) - 1)][['game_id', 'ply', 'move']]}")
        assert arena[k].tobytes() == solo[k].tobytes(), name
    for key in ("plies", "sims", "nn_rows", "records", "games_done"):
        assert arena[4][key] == solo[4][key], key
    st = arena[4]
    # plies 0..3 of the 18 first games, then of the 4 last: at every ply half the games' movers are A's, and
    # every list of 9 or 2 slots is padded to 17 rows
    assert _rows_add_up(st) and st["arena_rows"] == (8 * 16 * 17, 8 * 16 * 17)


# ---- 3. A != B on the real nets
def test_two_nets_identical_to_restatement():
    """34 slots x 32 sims x 6 plies (17 + 17, no padding); games 0..3 against the restatement fed each net's own
    HIP rows."""
    run = _run("init", "peaked", 34, 34, 32, 6, sim_groups=1)
    games = tuple(range(4))
    plies = _plies_of(run, games)
    assert plies == (6,) * 4
    rest = _restated_nets("init", "peaked", games, 32, plies)
    bad = _divergences(run, rest, 32)
    print(f"arena network parity: {sum(len(g) for g in rest.values())} root vectors compared, divergences {len(bad)}")
    assert bad == []
    st = run[4]
    assert st["arena_rows"] == (6 * 32 * 17, 6 * 32 * 17) and _rows_add_up(st)
    solo = _run("init", None, 34, 34, 32, 6)
    assert len(solo[0]) == len(run[0]) and (solo[0]["move"] != run[0]["move"]).any()


# ---- 4. layout independence, an empty list
def test_games_independent_of_the_split_and_an_empty_list():
    """The even game ids on 17 slots: every slot has the same mover, so one list is empty at every ply."""
    full = _run("init", "peaked", 34, 34, 32, 6, sim_groups=1)
    even = _run("init", "peaked", 17, 17, 32, 6, stride=2)
    assert sorted(set(even[0]["game_id"])) == list(range(0, 34, 2))
    for g in range(0, 34, 2):
        sa, sb = full[0]["game_id"] == g, even[0]["game_id"] == g
        assert sa.sum() == 6 and sb.sum() == 6
        for k in (0, 1, 2):
            assert full[k][sa].tobytes() == even[k][sb].tobytes(), (g, k)
    assert even[4]["arena_rows"] == (3 * 32 * 17, 3 * 32 * 17) and _rows_add_up(even[4])


# ---- 5. one stream against two chains
@pytest.mark.parametrize("slots,n_games,steps,max_moves", [(34, 34, 6, None), (40, 50, -1, 4)])
def test_one_stream_and_two_chains_identical(slots, n_games, steps, max_moves):
    one = _run("init", "peaked", slots, n_games, 32, steps, max_moves=max_moves, sim_groups=1)
    two = _run("init", "peaked", slots, n_games, 32, steps, max_moves=max_moves, sim_groups=2)
    assert len(one[0]) > 0 and (max_moves is None or len(one[3]) == n_games)
    for k, name in enumerate(("records", "root visits", "root moves", "game table")):
        assert one[k].tobytes() == two[k].tobytes(), name
    for key in ("plies", "sims", "nn_rows", "records", "arena_rows", "leaf_batch_rows"):
        assert one[4][key] == two[4][key], key
    assert _rows_add_up(two[4]) and min(two[4]["arena_rows"]) > 0


# ---- 6. sample_plies
@pytest.mark.parametrize("arena", [True, False])
@pytest.mark.parametrize("sample_plies", [2, -1])
def test_sample_plies(sample_plies, arena):
    slots, sims, steps = 6, 16, 8
    run = _run("init", "init" if arena else None, slots, slots, sims, steps, hash_eval=True,
               sample_plies=sample_plies)
    games = tuple(range(slots))
    plies = _plies_of(run, games)
    assert plies == (steps,) * slots
    rest = _restated_hash(games, sims, plies, sample_plies=sample_plies, same=not arena)
    assert _divergences(run, rest, sims) == []
    recs, visits, words = run[0], run[1], run[2]
    first = 0 if sample_plies < 0 else sample_plies
    late = recs["ply"] >= first
    assert late.sum() == slots * (steps - first)
    for r, v, w in zip(recs[late], visits[late], words[late]):
        j = int(np.argmax(v))  # the first maximum (the padding is -1)
        assert int(r["move"]) == AR.policy_index(int(w[j])), (r["game_id"], r["ply"])
    if sample_plies > 0:  # the drawn plies are those of the run that draws every ply
        drawn = _run("init", "init" if arena else None, slots, slots, sims, steps, hash_eval=True)
        early, early_d = recs["ply"] < first, drawn[0]["ply"] < first
        assert recs[early].tobytes() == drawn[0][early_d].tobytes()
        assert not _same_bytes(run, drawn, (0,))


# ---- 7. refusals
def _cfg(**kw):
    base = dict(device=0, slots=4, n_games=4, game_id_base=0, game_id_stride=1, seed=SEED, seed_mode=0, max_moves=0,
                batch=16, eps=0.25, alpha=0.3, sims=8, c_puct=1.5, eval_mode=EVAL_HASH, record_cap=1 << 10,
                recycle=1, precision=0, algo=0, tree_edge_cap=0, keep_root_visits=0)
    base.update(kw)
    return _lib.Config(**base)


def _refused(rc):
    assert rc == -1, rc  # KV_EINVAL
    return _lib.lib().kv_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    (dict(arena=1, sims=0), "needs sims >= 1"),
    (dict(arena=1, reuse_tree=1), "not the other player's"),
    (dict(arena=1, sims=0, eval_mode=EVAL_LAZY), "arena"),
    (dict(arena=1, sims=8, eval_mode=EVAL_LAZY), "lazy"),
    (dict(arena=2), "arena 2 must be 0 or 1"),
    (dict(arena=1, slots=33, sim_groups=2), "sim_groups 2"),
    (dict(sample_plies=-2), "sample_plies -2"),
    (dict(sample_plies=1, sims=0), "must be 0 with sims 0"),
])
def test_create_refusals(kw, text):
    h = C.c_void_p()
    msg = _refused(_lib.lib().kv_create(C.byref(_cfg(**kw)), C.byref(h)))
    assert text in msg, msg
    assert not h.value


def test_entry_point_refusals():
    L = _lib.lib()
    packed = packed_from(synthetic_state_dict(42, "init"))
    pw = packed.ctypes.data_as(C.POINTER(C.c_float))
    h = C.c_void_p()
    _lib.check(L.kv_create(C.byref(_cfg(arena=1)), C.byref(h)), "kv_create")
    try:
        _lib.check(L.kv_load_weights(h, pw, packed.size), "kv_load_weights")
        assert "kv_load_weights_b" in _refused(L.kv_run(h, 1, -1))  # player B's weights are missing
        states = np.zeros((1, 80), dtype=np.int8)
        out = (_lib.SearchResult * 1)()
        p = _lib.SearchParams(sims=4, leaves=1, eps=0.0, alpha=0.3, seed=0)
        msg = _refused(L.kv_search(h, states.ctypes.data_as(C.POINTER(C.c_int8)), 1, C.byref(p), out))
        assert "arena engine" in msg, msg
        _lib.check(L.kv_load_weights_b(h, pw, packed.size), "kv_load_weights_b")
        _lib.check(L.kv_run(h, 1, -1), "kv_run")
        cal = _lib.Calib()
        _lib.check(L.kv_engine_calibration_b(h, C.byref(cal)), "kv_engine_calibration_b")
    finally:
        L.kv_destroy(h)
    h = C.c_void_p()
    _lib.check(L.kv_create(C.byref(_cfg()), C.byref(h)), "kv_create")
    try:
        assert "arena 0" in _refused(L.kv_load_weights_b(h, pw, packed.size))
        assert "arena 0" in _refused(L.kv_engine_calibration_b(h, C.byref(_lib.Calib())))
    finally:
        L.kv_destroy(h)


# ---- 8. the Python surface and the loop
def test_play_match_and_the_loop():
    from knightvision_amd import arena
    from knightvision_amd.learn import reinforcement_loop
    from knightvision_amd.model import ChessNet
    a, b = synthetic_state_dict(42, "init"), synthetic_state_dict(42, "peaked")
    r = arena.play_match(a, b, 18, sims=8, slots=18, seed=SEED, max_moves=6, sample_plies=2)
    assert r["games"] == 18 == r["wins"] + r["draws"] + r["losses"] and len(r["game_table"]) == 18
    assert sum(r["as_white"]) == 9 and sum(r["as_black"]) == 9
    assert r["reasons"] == {"max_moves": 18} and r["draws"] == 18 and r["score"] == 0.5 and r["elo"] == 0.0
    # 6 plies x 8 sims, 9 slots of each player at every ply, padded to 17 rows
    assert r["stats"]["arena_rows"] == (6 * 8 * 17, 6 * 8 * 17) and _rows_add_up(r["stats"])
    torch.manual_seed(0)
    m = ChessNet()
    stats = reinforcement_loop(m, iterations=2, games_per_iter=8, device="cuda:0", epochs=1, batch_size=64,
                               max_moves=12, slots=8, log=None, arena_games=18, arena_sims=8)
    for st, updated in zip(stats, (False, True)):  # (iteration 1 has nothing to train on yet)
        ar = st["arena"]
        assert ar["games"] == 18 == ar["wins"] + ar["draws"] + ar["losses"] and ar["updated"] is updated
        assert sum(ar["as_white"]) == 9 and sum(ar["as_black"]) == 9
    assert stats[1]["optimizer_steps"] > 0
