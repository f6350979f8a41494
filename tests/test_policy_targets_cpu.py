"""CPU checks of the learn loop's "visits" policy target: the sparse PolicyTargets
(knightvision_amd/policy_targets.py) built from padded engine rows, their row
operations and dense form, the dense torch restatement of the soft-target
loss (train_ops.policy_loss off the GPU), the move words riding the
end-of-iteration gather (world 1 and a gloo world of 2), and the argument
checks that need no device."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

MAXM = 320


def word(frm, to, flags=0):
    return frm | (to << 6) | (flags << 12)


def padded(rows):
    out = np.full((len(rows), MAXM), 0xffff, dtype=np.uint16)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def hand_made():
    """4 rows: a promotion pair sharing one policy index, a zero-count move, a single move, an empty list."""
    moves = [[word(52, 60, 1), word(52, 60, 2), word(0, 63), word(63, 0)],
             [word(12, 28), word(6, 21), word(1, 18)],
             [word(4, 5, 3)],
             []]
    visits = [[3, 1, 0, 12], [0, 65000, 7], [16], []]
    return padded(visits), padded(moves), visits, moves


def test_from_engine_index_formula_prefixes_and_zero_counts():
    from knightvision_amd.policy_targets import PolicyTargets
    v, m, visits, moves = hand_made()
    t = PolicyTargets.from_engine(v, m)
    assert len(t) == 4 and t.off.dtype == torch.int64 and t.idx.dtype == torch.int16 and t.cnt.dtype == torch.int16
    assert t.off.tolist() == [0, 4, 7, 8, 8]  # prefix lengths, the zero-count entries kept
    want_idx = [(w & 63) * 64 + ((w >> 6) & 63) for r in moves for w in r]
    assert (t.idx.to(torch.int64) & 0xffff).tolist() == want_idx
    assert want_idx[:4] == [52 * 64 + 60, 52 * 64 + 60, 63, 63 * 64]
    assert (t.cnt.to(torch.int64) & 0xffff).tolist() == [c for r in visits for c in r]  # 65000 read as unsigned
    # the engine's host visits are int32 with -1 padding: the same targets
    v32 = np.where(v == 0xffff, -1, v.astype(np.int32))
    t32 = PolicyTargets.from_engine(v32, m)
    assert torch.equal(t32.off, t.off) and torch.equal(t32.cnt, t.cnt) and torch.equal(t32.idx, t.idx)
    bad = m.copy()
    bad[1, 3] = word(8, 16)  # one move word more than visit counts
    with pytest.raises(ValueError):
        PolicyTargets.from_engine(v, bad)


def test_dense_sums_repeats_and_normalises():
    from knightvision_amd.policy_targets import PolicyTargets
    v, m, _, _ = hand_made()
    t = PolicyTargets.from_engine(v, m)
    d = t.dense(torch.arange(4))
    assert d.shape == (4, 4096) and d.dtype == torch.float32
    assert d[0, 52 * 64 + 60] == 4 / 16 and d[0, 63] == 0 and d[0, 63 * 64] == 12 / 16
    assert d[1, 6 * 64 + 21].item() == pytest.approx(65000 / 65007) and d[1, 12 * 64 + 28] == 0
    assert d[2, 4 * 64 + 5] == 1 and (d[3] == 0).all()
    assert torch.equal(d.sum(1) > 0, torch.tensor([True, True, True, False]))
    assert torch.allclose(d[:3].sum(1), torch.ones(3))
    # an all-zero row (legal moves, no visits): pi = 0
    z = PolicyTargets.from_engine(padded([[0, 0]]), padded([[word(1, 2), word(3, 4)]]))
    assert z.off.tolist() == [0, 2] and (z.dense() == 0).all()
    assert torch.equal(t.dense(torch.tensor([2, 0, 2])), d[[2, 0, 2]])


def test_select_and_cat_round_trip():
    from knightvision_amd.policy_targets import PolicyTargets
    v, m, _, _ = hand_made()
    t = PolicyTargets.from_engine(v, m)
    d = t.dense()
    pick = torch.tensor([3, 1, 1, 0])
    s = t.select(pick)
    assert s.off.tolist() == [0, 0, 3, 6, 10] and torch.equal(s.dense(), d[pick])
    mask = torch.tensor([True, False, True, True])
    assert torch.equal(t[mask].dense(), d[mask])
    back = PolicyTargets.cat([t.select(torch.tensor([0, 1])), t.select(torch.tensor([2])), t.select(torch.tensor([3]))])
    assert torch.equal(back.off, t.off) and torch.equal(back.idx, t.idx) and torch.equal(back.cnt, t.cnt)
    e = PolicyTargets.cat([PolicyTargets.empty(), t, PolicyTargets.empty()])
    assert torch.equal(e.off, t.off) and torch.equal(e.idx, t.idx)
    assert len(t.select(torch.zeros(0, dtype=torch.int64))) == 0


def test_one_hot_is_the_hard_cross_entropy_and_all_zero_row_is_zero():
    from knightvision_amd.policy_targets import PolicyTargets
    from knightvision_amd.train_ops import policy_loss
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(6, 4096, generator=g) * 3
    mv = torch.tensor([0, 4095, 77, 1234, 64, 63])
    t = PolicyTargets.one_hot(mv)
    rows = torch.tensor([5, 3, 0, 1, 2, 4])
    ce, ent = policy_loss(logits, t, rows)
    want = F.cross_entropy(logits, mv[rows], reduction="none")
    assert torch.allclose(ce, want, rtol=0, atol=1e-5)
    lp = F.log_softmax(logits, 1)
    assert torch.allclose(ent, -(lp.exp() * lp).sum(1), rtol=0, atol=1e-5)
    assert ce.mean().item() == pytest.approx(F.cross_entropy(logits, mv[rows]).item(), abs=1e-5)
    z = PolicyTargets.from_engine(padded([[0, 0, 0]]), padded([[word(1, 2), word(3, 4), word(5, 6)]]))
    ce0, ent0 = policy_loss(logits[:1], z, torch.tensor([0]))
    assert ce0.item() == 0.0 and ent0.item() > 0
    with pytest.raises(ValueError):
        policy_loss(logits[:, :100], t, rows)


def test_batches_hand_each_batch_its_rows():
    """train.batches(..., targets=...) -> every Batch carries the targets and its sample indices; batch_loss on
    the CPU (dense restatement) with one-hot targets is the move-played loss."""
    from knightvision_amd import train as T
    from knightvision_amd.policy_targets import PolicyTargets
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 13, (10, 64), generator=g).to(torch.int8)
    moves = torch.randint(0, 4096, (10,), generator=g)
    rew = torch.ones(10)
    t = PolicyTargets.one_hot(moves)
    bs = list(T.batches(codes, moves, rew, 4, True, torch.Generator().manual_seed(2), targets=t))
    assert [b.rows.numel() for b in bs] == [4, 4, 2] and all(b.targets is t for b in bs)
    assert sorted(torch.cat([b.rows for b in bs]).tolist()) == list(range(10))
    for b in bs:
        assert torch.equal(moves[b.rows], b.moves)
    plain = list(T.batches(codes, moves, rew, 4, False))
    assert all(b.targets is None and b.rows is None for b in plain)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Linear(768, 4096)
            self.v = torch.nn.Linear(768, 1)

        def forward(self, x):
            return self.p(x.flatten(1)), self.v(x.flatten(1))

    torch.manual_seed(0)
    net = Net()
    b = bs[0]
    soft = T.batch_loss(net, b, amp=False)
    hard = T.batch_loss(net, T.Batch(b.boards, b.moves, b.outcomes), amp=False)
    for a, c in zip(soft[:4], hard[:4]):
        assert a.item() == pytest.approx(c.item(), abs=1e-5)


def test_pack_round_trips_move_words():
    from knightvision_amd.distributed import pack_pi, unpack_pi
    rng = np.random.default_rng(7)
    lens = [0, 320, 1, 23, 64, 65]
    rows = [[word(int(a), int(b), int(f)) for a, b, f in zip(rng.integers(0, 64, n), rng.integers(0, 64, n),
                                                            rng.integers(0, 16, n))] for n in lens]
    rows[1][0] = word(63, 62, 15)  # 0xffbf: the largest word a list can hold is not the padding
    m = padded(rows)
    t = torch.from_numpy(m.view(np.uint8).reshape(len(lens), 2 * MAXM).copy())
    counts, packed = pack_pi(t)
    assert counts.tolist() == lens and packed.numel() == sum(lens)
    assert np.array_equal(unpack_pi(counts, packed, MAXM).numpy().view(np.uint16), m)


def _experience(rank, world, n_games):
    """Records of this rank's games (plies out of order), their visit rows and move words, each row's
    contents a function of (game id, ply) so the receiver can check the pairing."""
    from knightvision_amd.engine import GAME_DTYPE, RECORD_DTYPE
    ids = list(range(rank, n_games, world))
    recs, games = [], np.zeros(len(ids), dtype=GAME_DTYPE)
    for k, gid in enumerate(ids):
        n = 3 + gid
        r = np.zeros(n, dtype=RECORD_DTYPE)
        r["game_id"] = gid
        r["ply"] = np.arange(n)[::-1]
        r["move"] = gid * 100 + np.arange(n)[::-1]
        recs.append(r)
        games[k]["game_id"] = gid
        games[k]["plies"] = n
    recs = np.concatenate(recs) if recs else np.zeros(0, dtype=RECORD_DTYPE)
    vis, mv = _rows_of(recs)
    return recs, games, vis, mv


def _rows_of(recs):
    vis, mv = [], []
    for r in recs:
        n = 1 + (int(r["game_id"]) * 7 + int(r["ply"])) % 5
        vis.append([int(r["ply"]) + j for j in range(n)])
        mv.append([word((int(r["game_id"]) + j) % 64, (int(r["ply"]) + 2 * j + 1) % 64, j % 4) for j in range(n)])
    return padded(vis), padded(mv)


def _bytes(a):
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], 2 * MAXM).copy())


def test_gather_experience_world_one_returns_words_in_record_order():
    from knightvision_amd.distributed import gather_experience
    recs, games, vis, mv = _experience(0, 1, 4)
    r, g, p, m = gather_experience(recs, games, dst=0, pi=_bytes(vis), pi_moves=_bytes(mv))
    assert list(zip(r["game_id"], r["ply"])) == sorted(zip(recs["game_id"], recs["ply"]))
    want_v, want_m = _rows_of(r)
    assert m.dtype == np.uint16 and m.shape == (len(r), MAXM)
    assert np.array_equal(p, want_v) and np.array_equal(m, want_m)
    # without pi_moves the return shape is the present one
    assert len(gather_experience(recs, games, dst=0, pi=_bytes(vis))) == 3
    assert len(gather_experience(recs, games, dst=0)) == 2
    with pytest.raises(ValueError):
        gather_experience(recs, games, dst=0, pi_moves=_bytes(mv))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, n_games, port, out_q):
    import torch.distributed as dist
    from knightvision_amd.distributed import gather_experience
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    recs, games, vis, mv = _experience(rank, world, n_games)
    r, g, p, m = gather_experience(recs, games, dst=None, pi=_bytes(vis), pi_moves=_bytes(mv))
    root = gather_experience(recs, games, dst=0, pi=_bytes(vis), pi_moves=_bytes(mv))
    assert len(root) == 4 and (root[3] is None) == (rank != 0)
    if rank == 0:
        assert np.array_equal(root[3], m) and np.array_equal(root[2], p)
    out_q.put((rank, r["game_id"].tolist(), r["ply"].tolist(), p.tolist(), m.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_experience_world_two_is_the_rank_order_union():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    n_games = 5
    procs = [ctx.Process(target=_worker, args=(r, 2, n_games, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the union: both ranks' rows concatenated in rank order, then ordered by (game id, ply)
    parts = [_experience(r, 2, n_games) for r in range(2)]
    recs = np.concatenate([p[0] for p in parts])
    vis, mv = np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
    order = np.lexsort((recs["ply"], recs["game_id"]))
    for rank, ids, ply, p, m in res:
        assert ids == recs["game_id"][order].tolist() and ply == recs["ply"][order].tolist()
        assert np.array_equal(np.array(p, dtype=np.uint16), vis[order])
        assert np.array_equal(np.array(m, dtype=np.uint16), mv[order])


def test_extend_dataset_filters_targets_with_the_samples():
    """learn.extend_dataset in "visits" mode: the target rows follow the decisive filter, and samples that came
    without a search (a dataset built in "move" form) get their one-hot rows."""
    from knightvision_amd.engine import GAME_DTYPE, RECORD_DTYPE
    from knightvision_amd.learn import extend_dataset
    recs = np.zeros(24, dtype=RECORD_DTYPE)
    recs["game_id"] = np.repeat([0, 1, 2], 8)  # game 2 never finished: no row in `games`
    recs["ply"] = np.tile(np.arange(8), 3)
    recs["move"] = np.arange(24) * 3
    games = np.zeros(2, dtype=GAME_DTYPE)
    games["game_id"] = [0, 1]
    games["reward"] = [1.0, 0.2]  # >= 10 decisive records are needed to filter: 8 here, so all 16 stay
    vis, mv = _rows_of(recs)
    data = extend_dataset(None, recs, games, "cpu", pi=(vis, mv), policy_targets=True)
    assert len(data) == 4 and data[0].shape == (16, 64) and len(data[3]) == 16
    want_v, want_m = _rows_of(recs[:16])
    assert np.array_equal((data[3].cnt.numpy().view(np.uint16)), want_v[want_v != 0xffff])
    games["reward"] = [1.0, -1.0]
    recs2 = recs.copy()
    recs2["game_id"] = np.repeat([0, 1, 1], 8)
    recs2["ply"] = np.arange(24) % 16
    games2 = games.copy()
    games2["reward"] = [0.2, 1.0]  # 16 decisive records: game 0's 8 are dropped with their target rows
    vis2, mv2 = _rows_of(recs2)
    old = tuple(x.clone() for x in data[:3])  # a three-element dataset: its samples get one-hot rows
    both = extend_dataset(old, recs2, games2, "cpu", pi=(vis2, mv2), policy_targets=True)
    assert both[0].shape[0] == 32 and len(both[3]) == 32
    assert both[3].off[:17].tolist() == list(range(17))
    assert (both[3].idx[:16].to(torch.int64) & 0xffff).tolist() == data[1].tolist()
    kv, _ = _rows_of(recs2[8:])
    assert np.array_equal(both[3].cnt[16:].numpy().view(np.uint16), kv[kv != 0xffff])
    assert torch.equal(both[2][16:], torch.ones(16))
    plain = extend_dataset(None, recs, games, "cpu")
    assert len(plain) == 3
    with pytest.raises(ValueError):
        extend_dataset(None, recs, games, "cpu", policy_targets=True)


def test_visits_target_needs_a_search():
    """policy_target="visits" with sims = 0 is refused before any device is touched."""
    from knightvision_amd.learn import reinforcement_loop, selfplay_shard
    with pytest.raises(ValueError, match="sims"):
        reinforcement_loop(None, 1, 8, "cuda:0", sims=0, policy_target="visits", log=None)
    with pytest.raises(ValueError):
        reinforcement_loop(None, 1, 8, "cuda:0", sims=16, policy_target="pi", log=None)
    with pytest.raises(ValueError, match="sims"):
        selfplay_shard(None, 8, 0, "cuda:0", sims=0, policy_targets=True)


def test_root_moves_null_engine_is_einval():
    from knightvision_amd import _lib
    L = _lib.lib()
    n = C.c_size_t()
    assert L.kv_root_moves(None, None, 0, C.byref(n)) == -1 and "NULL" in L.kv_last_error().decode()
    assert L.kv_root_moves_device(None, None, 0, C.byref(n), None) == -1
    assert L.kv_tr_policy_loss_f16(None, None, None, None, None, 0, None, None, None, None) == -1
    assert L.kv_tr_policy_loss_backward_f16(None, None, None, None, None, 0, None, None, None, None, None, None) == -1
