"""CPU side of the start-position tests (kv_dev_set_starts; tests/_mcts_starts.py): the references start
anywhere, the Python restatements' termination (tests/_mcts_endings.py) is the C oracle's, and the runs
tests/test_starts_gpu.py compares the engine with hold -- from the references alone -- every ending, root
width, special move and mode-specific case those tests rely on."""
import numpy as np
import pytest

from oracle import oracle as O

from tests import _mcts_endings as E
from tests import _mcts_selfplay_leaves as SL
from tests import _mcts_starts as ST

SEED, N, SIMS = ST.SEED, ST.N_GAMES, ST.SIMS
KEYS = ("moves", "visits", "boards", "plies", "outcome", "reason", "reward", "n_evals")


def test_the_set_holds_the_moves_it_is_meant_to():
    flags = {n: set(int(f) for f in O.valid_moves(ST.POSITIONS[n])[0][:, 2]) for n in ST.NAMES}
    assert 4 in flags["PROMO"] and 1 in flags["EP"] and 2 in flags["CASTLE"]
    m = O.valid_moves(ST.CASTLE)[0]
    assert sorted(int(to) for fr, to, fl in m if fl & 2) == [ST.sq("c1"), ST.sq("g1")]  # both castlings
    assert tuple(ST.EP[75:77]) == (2, 3) and not ST.CASTLE[69:75].any()
    assert [int(ST.POSITIONS[n][64]) for n in ("BQ", "KRK_B", "BLACK_MG", "BLACK_OPEN", "KPK_CAPTURE")] == [0] * 5
    for n in ("CHECKMATED_ROOT", "STALEMATE_ROOT"):
        assert len(O.valid_moves(ST.POSITIONS[n])[0]) == 0
    assert O.in_check(ST.CHECKMATED_ROOT) and not O.in_check(ST.STALEMATE_ROOT) and O.is_draw(ST.KINGS_ONLY_ROOT)
    widths = [len(O.valid_moves(ST.POSITIONS[n])[0]) for n in ("WIDE_A", "WIDE_B", "WIDE_C")]
    assert widths[0] > 64 and widths[1] > 128 and widths[2] > 128, widths
    assert len(ST.NAMES) == 19 and N == 38  # two rounds: the engine's start list wraps


def test_the_oracle_starts_anywhere_and_defaults_to_the_initial_position():
    a = O.mcts_play_batch(8, [5, 6], max_moves=4, keep_visits=True)
    b = O.mcts_play_batch(8, [5, 6], max_moves=4, keep_visits=True, starts=[O.initial_state()] * 2)
    c = O.mcts_play_game(8, O.MT(5, "numpy"), O.MT(5, "python"), max_moves=4, start=O.initial_state())
    for x, y in zip(a, b):
        assert np.array_equal(x["moves"], y["moves"]) and np.array_equal(x["visits"], y["visits"])
    assert np.array_equal(a[0]["moves"], c["moves"]) and np.array_equal(a[0]["visits"], c["visits"])
    # a batch from the set is its single games, and a start with no move is a game of 0 plies
    many = O.mcts_play_batch(SIMS, [SEED + g for g in range(6)], max_moves=ST.MAX_MOVES, keep_visits=True,
                             starts=[ST.start_of(g) for g in range(6)])
    for g, r in enumerate(many):
        one = O.mcts_play_game(SIMS, O.MT(SEED + g, "numpy"), O.MT(SEED + g, "python"), max_moves=ST.MAX_MOVES,
                               start=ST.start_of(g))
        assert np.array_equal(r["moves"], one["moves"]) and (r["plies"], r["reason"]) == (one["plies"], one["reason"])
    assert (many[3]["plies"], many[3]["reason"], many[3]["outcome"], many[3]["n_evals"]) == (0, 2, 1, 0)
    assert (many[4]["plies"], many[4]["reason"], many[4]["outcome"]) == (0, 3, 0)
    assert (many[5]["plies"], many[5]["reason"]) == (1, 4)  # kings only: isDraw is tested after a move


def test_the_reference_path_starts_anywhere():
    def ev(planes):
        return np.zeros((len(planes), 4096), dtype=np.float32), np.zeros(len(planes), dtype=np.float32)
    a = O.play_game(ev, O.MT(7, "numpy"), O.MT(7, "python"), O.Last(), max_moves=6)
    b = O.play_game(ev, O.MT(7, "numpy"), O.MT(7, "python"), O.Last(), max_moves=6, start=O.initial_state())
    assert np.array_equal(a["moves"], b["moves"]) and np.array_equal(a["states"], b["states"])
    r = O.play_game(ev, O.MT(7, "numpy"), O.MT(7, "python"), O.Last(), max_moves=6, start=ST.CHECKMATED_ROOT)
    assert (r["plies"], r["reason"], r["outcome"], len(r["eval_sizes"])) == (0, 2, 1, 0)
    r = O.play_game(ev, O.MT(7, "numpy"), O.MT(7, "python"), O.Last(), max_moves=6, start=ST.MATE_IN_ONE)
    assert np.array_equal(r["states"][0], O.valid_moves(ST.MATE_IN_ONE)[1])


def test_sample_plies_in_the_oracle_is_the_first_maximum():
    for g, r in enumerate(ST.oracle_run(SEED, N, SIMS, -1)):
        vec = ST.start_of(g)
        for mv, v in zip(r["moves"], r["visits"]):
            m3 = O.valid_moves(vec)[0]
            pick = v.index(max(v))
            assert int(m3[pick][0]) * 64 + int(m3[pick][1]) == mv
            vec = O.make_valid_move(vec, pick)


@pytest.mark.parametrize("sample_plies", [0, -1])
def test_the_python_termination_is_the_oracles(sample_plies):
    """Leaves 1, no reuse, no arena: the ending-aware restatements equal kvo_mcts_play_batch from the same starts
    on moves, visits, boards and the whole game row."""
    want = ST.oracle_run(SEED, N, SIMS, sample_plies)
    mine = ST.leaves_run(SEED, N, SIMS, 1, sample_plies)
    for g, (x, y) in enumerate(zip(mine, want)):
        assert {k: x[k] for k in KEYS} == {k: y[k] for k in KEYS}, g
    if sample_plies == 0:  # (tests/_mcts_selfplay_reuse.py draws every move)
        for g, (x, y) in enumerate(zip(ST.reuse_run(SEED, N, SIMS, False), want)):
            assert {k: x[k] for k in KEYS} == {k: y[k] for k in KEYS}, g
    # the arena restatement with one evaluator for both players is the self-play game
    from tests import _mcts_arena as AR
    for g in (1, 9, 12, 29):
        p = AR.play(SEED + g, g, SIMS, None, AR.hash_eval, AR.hash_eval, sample_plies=sample_plies, eps=ST.EPS,
                    start=ST.start_of(g), max_moves=ST.MAX_MOVES)
        y = want[g]
        assert [x["move"] for x in p] == y["moves"] and [x["visits"] for x in p] == y["visits"]
        assert p.result == (y["plies"], y["outcome"], y["reason"], y["reward"])
        assert len(p) + sum(e["pending"] for e in p.extra) == y["n_evals"]


def test_a_game_that_ends_without_a_move_holds_its_slot_one_more_step():
    games = ST.oracle_run(SEED, N, SIMS)
    mine = ST.leaves_run(SEED, N, SIMS, 1)
    for r, m in zip(games, mine):
        on_move = r["reason"] in (0, 1, 4)
        assert m["holds"] == r["plies"] + (0 if on_move else 1)
    assert SL.starts_of([0, 0, 3, 2], 1, holds=[1, 1, 3, 3]) == [0, 1, 2, 5]  # a chain of 0-ply games in one slot
    assert SL.starts_of([3, 2, 2], 2) == [0, 0, 2]
    assert E.Played().result is None


def test_the_one_leaf_runs_hold_every_case():
    sampled = ST.coverage(ST.oracle_run(SEED, N, SIMS, 0))
    first_max = ST.coverage(ST.oracle_run(SEED, N, SIMS, -1))
    assert not ST.GENERAL - sampled, sorted(ST.GENERAL - sampled)
    assert "max@64+" in first_max and {"root>64", "root>96", "root>128"} <= first_max


def test_the_arena_runs_hold_wins_for_both_players_in_both_colours():
    need = {"A_wins_A_white", "A_wins_A_black", "B_wins_A_white", "B_wins_A_black", "first_black"}
    for games in (ST.arena_run(SEED, N, SIMS), ST.leaves_run(SEED, N, SIMS, 4, 0, True)):
        got = ST.coverage(games)
        assert need <= got, sorted(need - got)
        assert sum(r["outcome"] != 0 for r in games) and sum(r["outcome"] == 0 for r in games)


def test_the_reuse_run_carries_and_drops():
    games = ST.reuse_run(SEED, N, SIMS)
    got = ST.coverage(games)
    assert {"carried", "dropped_at_end"} <= got
    dropped = [g for g, r in enumerate(games) if r["plies"] and r["child_kept"][-1] and r["holds"] == r["plies"]]
    assert set(dropped) & set(ST.recycled_after(games, ST.SLOTS_THIRD))  # ... in a slot that starts another game
    assert {"reason2+", "reason3@1+", "reason3@0", "reason2@0", "reason4@1", "reason1+", "reason1-"} <= got


@pytest.mark.parametrize("leaves", [2, 8])
def test_the_leaves_runs_hold_a_terminal_leaf_and_a_mate(leaves):
    got = ST.coverage(ST.leaves_run(SEED, N, SIMS, leaves))
    assert "terminal_leaf_mid_game" in got and ({"reason2+", "reason2-"} & got)
    assert {"root>128", "reason3@0", "reason2@0", "reason4@1"} <= got


def test_set_starts_refuses_a_null_engine():
    from knightvision_amd import _lib
    L = _lib.lib()
    assert "kv_dev_set_starts" in _lib.EXPORTED and hasattr(L, "kv_dev_set_starts")
    assert L.kv_dev_set_starts(None, None, 0) == -1
    assert "kv_dev_set_starts: NULL engine" in L.kv_last_error().decode()
    st = ST.start_list()
    import ctypes as C
    assert L.kv_dev_set_starts(None, st.ctypes.data_as(C.POINTER(C.c_int8)), len(st)) == -1
