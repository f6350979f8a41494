"""Carried subtrees in MCTS self-play (kv_config.reuse_tree), the parts that need no GPU: the config
validation and the ctypes mirrors of kv_config / kv_stats, and the plain-Python restatement
(tests/_mcts_selfplay_reuse.py) pinned against the C oracle with reuse disabled, then checked for its own
invariants with reuse enabled."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _mcts_selfplay_reuse as R

SEEDS, PLIES, SIMS = (49, 50, 51), 8, 48


def _cfg(**kw):
    from knightvision_amd import _lib
    base = dict(device=0, slots=4, n_games=4, game_id_base=0, game_id_stride=1, seed=42, seed_mode=0, max_moves=0,
                batch=16, eps=0.25, alpha=0.3, sims=16, c_puct=1.5, eval_mode=0, record_cap=0, recycle=1,
                precision=0, algo=0, tree_edge_cap=0, keep_root_visits=0, reuse_tree=0)
    base.update(kw)
    return _lib.Config(**base)


@pytest.mark.parametrize("kw, msg", [
    (dict(reuse_tree=2), "reuse_tree 2 must be 0 or 1"),
    (dict(reuse_tree=-1), "reuse_tree -1 must be 0 or 1"),
    (dict(reuse_tree=1, sims=0), "needs sims >= 1"),
])
def test_kv_create_rejects_bad_reuse_configs(kw, msg):
    """Validated before the device is touched: KV_EINVAL and the reason in kv_last_error()."""
    from knightvision_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _cfg(**kw)
    assert L.kv_create(C.byref(cfg), C.byref(h)) == -1  # KV_EINVAL
    assert msg in L.kv_last_error().decode()
    assert not h.value


def test_config_and_stats_mirrors_match_library():
    from knightvision_amd import _lib
    L = _lib.lib()
    assert L.kv_sizeof_config() == C.sizeof(_lib.Config)
    assert L.kv_sizeof_stats() == C.sizeof(_lib.Stats)
    assert _lib.Config._fields_[-1][0] == "reuse_tree"
    assert [f for f, _ in _lib.Stats._fields_[-3:]] == ["sims_kept", "roots_carried", "leaf_batch_rows"]


def test_compact_step_macro_mirrored():
    import os
    import re
    from knightvision_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "kv.h")).read()
    assert int(re.search(r"#define KV_REUSE_COMPACT_STEP (\d+)", hdr).group(1)) == _lib.REUSE_COMPACT_STEP


@functools.lru_cache(maxsize=None)
def _games(reuse):
    return {s: R.play(s, SIMS, PLIES, reuse) for s in SEEDS}


def test_restatement_without_reuse_equals_oracle():
    """Reuse disabled: the Python root mix, PUCT and choice are the C oracle's, move for move and vector for
    vector (hash evaluator)."""
    from oracle import oracle as O
    for seed, plies in _games(False).items():
        r = O.mcts_play_game(SIMS, O.MT(seed, "numpy"), O.MT(seed, "python"), None, max_moves=PLIES, c_puct=1.5)
        assert len(r["moves"]) == PLIES
        for p, ply in enumerate(plies):
            assert ply["move"] == r["moves"][p], (seed, p)
            n = len(ply["visits"])
            assert np.array_equal(r["visits"][p][:n], ply["visits"]) and (r["visits"][p][n:] == -1).all(), (seed, p)
            assert ply["kept"] == 0 and ply["rem"] == SIMS


def test_restatement_with_reuse_invariants():
    for seed, plies in _games(True).items():
        assert plies[0]["kept"] == 0
        for p, ply in enumerate(plies):
            assert sum(ply["visits"]) == SIMS, (seed, p)
            assert ply["kept"] + ply["rem"] == SIMS and len(ply["pending"]) == ply["rem"]
            assert ply["nodes"] <= SIMS + 1, (seed, p)
            if p:
                assert ply["kept"] == plies[p - 1]["played_n"] - 1, (seed, p)


def test_restatement_games_do_carry():
    """The chosen seeds carry: at least half of every game's plies after the first start from a tree with two
    or more visits, so no test over these games can pass by never carrying."""
    for seed, plies in _games(True).items():
        carried = sum(ply["kept"] >= 2 for ply in plies[1:])
        assert 2 * carried >= len(plies) - 1, (seed, [ply["kept"] for ply in plies])
    # and the first ply is the same search either way
    for seed in SEEDS:
        assert _games(True)[seed][0]["visits"] == _games(False)[seed][0]["visits"]
