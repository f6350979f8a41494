"""Sparse policy targets of the learn loop's "visits" mode: each sample's MCTS
root visit distribution pi over its legal moves, as a CSR over the dataset's
samples on the dataset's device.

    off int64 [N + 1]   row i holds entries off[i] .. off[i + 1]
    idx int16 [nnz]     policy index of the entry's root move (uint16 bits)
    cnt int16 [nnz]     its visit count (uint16 bits: counts reach KV_MAX_SIMS = 65,000,
                        so every consumer reads them as unsigned -- as distributed.pack_pi)

One entry per legal root move, in root-list order; a move the search never
visited keeps its zero count, so the row is also the position's legal set.
pi_k = (sum of cnt over the row's entries with idx k) / (sum of the row's cnt);
a row whose counts are all zero has pi = 0 (its cross-entropy is 0). About 4 B
per legal move (~92 B per sample at 23 moves) against 1,280 B for the padded
visits and move words.

The policy index of a root move word w (from | to << 6 | flags << 12,
SelfPlayEngine.root_moves()) is (w & 63) * 64 + ((w >> 6) & 63), the index
kv_net_forward_boards_legal documents. A sample without a search (a PGN / JSONL
sample, a record of a sims = 0 run) gets the one-entry row (move, 1), whose
soft cross-entropy is the hard one.

Optional per-sample weights `w` (float32 [N]; None: none, every consumer then
takes the code path it always took): 1 for a sample whose row is a policy
target, 0 for one whose row is not -- a fast ply of playout cap randomization
(kv_config.fast_sims), searched too shallowly to train the policy on. They are
filtered, indexed and concatenated with the rows (a part without weights counts
as all ones), and train.batch_loss weighs the policy term by them.
"""
from __future__ import annotations

import numpy as np
import torch

from .distributed import pack_pi

N_POLICY = 4096


def _u16(t: torch.Tensor) -> torch.Tensor:
    """int16 holding uint16 bits -> int64 values."""
    return t.to(torch.int64) & 0xffff


def move_word_index(words: torch.Tensor) -> torch.Tensor:
    """uint16 move words (as int16 bits or any wider integer) -> policy indices int64."""
    w = words.to(torch.int64) & 0xffff
    return (w & 63) * 64 + ((w >> 6) & 63)


def _padded_rows(x, device) -> torch.Tensor:
    """[n, MAXM] padded uint16 rows (numpy of any integer dtype, -1 or 0xffff padded; a torch int16 / uint8
    byte-pair tensor) -> uint8 [n, 2 * MAXM], pack_pi's input form."""
    if isinstance(x, torch.Tensor):
        t = x if x.dtype == torch.uint8 else x.to(torch.int16).contiguous().view(torch.uint8)
        return t.reshape(x.shape[0], -1).to(device)
    a = np.ascontiguousarray(np.asarray(x).astype(np.uint16))
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1)).to(device)


class PolicyTargets:
    def __init__(self, off: torch.Tensor, idx: torch.Tensor, cnt: torch.Tensor, w: torch.Tensor | None = None):
        assert off.dtype == torch.int64 and idx.dtype == torch.int16 and cnt.dtype == torch.int16
        assert off.dim() == 1 and off.numel() >= 1 and idx.shape == cnt.shape and idx.dim() == 1
        self.off, self.idx, self.cnt = off.contiguous(), idx.contiguous(), cnt.contiguous()
        if w is not None:
            assert w.dim() == 1 and w.numel() == off.numel() - 1
            w = w.to(device=off.device, dtype=torch.float32).contiguous()
        self.w = w

    def __len__(self) -> int:
        return int(self.off.numel()) - 1

    @property
    def device(self) -> torch.device:
        return self.off.device

    @property
    def nnz(self) -> int:
        return int(self.idx.numel())

    def to(self, device) -> "PolicyTargets":
        return PolicyTargets(self.off.to(device), self.idx.to(device), self.cnt.to(device),
                             None if self.w is None else self.w.to(device))

    def weights(self) -> torch.Tensor:
        """The per-sample weights float32 [N]; all ones when the targets carry none."""
        return self.w if self.w is not None else torch.ones(len(self), dtype=torch.float32, device=self.device)

    def lengths(self) -> torch.Tensor:
        return self.off[1:] - self.off[:-1]

    # ---- builders
    @staticmethod
    def empty(device="cpu") -> "PolicyTargets":
        z = torch.zeros(0, dtype=torch.int16, device=device)
        return PolicyTargets(torch.zeros(1, dtype=torch.int64, device=device), z, z.clone())

    @staticmethod
    def from_packed(counts: torch.Tensor, visits: torch.Tensor, words: torch.Tensor) -> "PolicyTargets":
        """pack_pi's compact form (the form the rows cross ranks in): counts int16 [n] entries per row, the
        rows' visit counts and move words int16 [sum counts] (uint16 bits)."""
        if visits.shape != words.shape or int(_u16(counts).sum()) != visits.numel():
            raise ValueError("PolicyTargets.from_packed: counts, visits and move words do not line up")
        off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=visits.device)
        off[1:] = torch.cumsum(_u16(counts).to(visits.device), 0)
        return PolicyTargets(off, move_word_index(words).to(torch.int16), visits.to(torch.int16))

    @staticmethod
    def from_engine(visits, moves, device="cpu", weights=None) -> "PolicyTargets":
        """visits / moves uint16 [n, MAXM] (SelfPlayEngine.root_visits() / root_moves(), row for row; the
        visits' -1 padding reads as 0xffff): each row's legal-move prefix, zero counts kept. weights: optional
        [n] per-sample weights (1 - engine.fast_mask(records) with kv_config.fast_sims)."""
        v, m = _padded_rows(visits, device), _padded_rows(moves, device)
        if v.shape != m.shape:
            raise ValueError(f"PolicyTargets.from_engine: visits {tuple(v.shape)} and moves {tuple(m.shape)} differ")
        cv, pv = pack_pi(v)
        cm, pm = pack_pi(m)
        if not torch.equal(cv, cm):
            raise ValueError("PolicyTargets.from_engine: a row's visits and move words differ in length")
        out = PolicyTargets.from_packed(cv, pv, pm)
        if weights is not None:
            wt = torch.as_tensor(np.asarray(weights, dtype=np.float32) if not isinstance(weights, torch.Tensor)
                                 else weights).reshape(-1)
            if wt.numel() != len(out):
                raise ValueError(f"PolicyTargets.from_engine: {wt.numel()} weights for {len(out)} rows")
            out = PolicyTargets(out.off, out.idx, out.cnt, wt)
        return out

    @staticmethod
    def one_hot(move_index: torch.Tensor) -> "PolicyTargets":
        """The row (move, 1) per sample: the target of a sample that has no search."""
        mv = move_index.reshape(-1)
        n = mv.numel()
        return PolicyTargets(torch.arange(n + 1, dtype=torch.int64, device=mv.device), mv.to(torch.int16),
                             torch.ones(n, dtype=torch.int16, device=mv.device))

    @staticmethod
    def cat(parts) -> "PolicyTargets":
        parts = list(parts)
        dev = parts[0].device
        offs, base = [torch.zeros(1, dtype=torch.int64, device=dev)], 0
        for p in parts:
            offs.append(p.off[1:].to(dev) + base)
            base += p.nnz
        w = None
        if any(p.w is not None for p in parts):  # a part without weights: every row a policy target
            w = torch.cat([p.weights().to(dev) for p in parts])
        return PolicyTargets(torch.cat(offs), torch.cat([p.idx.to(dev) for p in parts]),
                             torch.cat([p.cnt.to(dev) for p in parts]), w)

    # ---- row operations
    def select(self, rows: torch.Tensor) -> "PolicyTargets":
        """The rows a bool mask [N] keeps, or the rows of an index tensor, in its order (repeats allowed)."""
        rows = rows.to(self.device)
        if rows.dtype == torch.bool:
            rows = torch.nonzero(rows).reshape(-1)
        rows = rows.to(torch.int64).reshape(-1)
        ln = self.lengths()[rows]
        off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=self.device)
        off[1:] = torch.cumsum(ln, 0)
        # entry e of the new row r comes from self.off[rows[r]] + (e - off[r])
        src = torch.repeat_interleave(self.off[rows] - off[:-1], ln) + torch.arange(int(off[-1]), device=self.device)
        return PolicyTargets(off, self.idx[src], self.cnt[src], None if self.w is None else self.w[rows])

    __getitem__ = select

    def dense(self, rows: torch.Tensor | None = None, dtype=torch.float32) -> torch.Tensor:
        """pi of the given rows (all when None) as [B, 4096]: repeated indices of a row add, a row whose
        counts are all zero is all zeros."""
        t = self if rows is None else self.select(rows)
        n = len(t)
        out = torch.zeros((n, N_POLICY), dtype=dtype, device=t.device)
        r = torch.repeat_interleave(torch.arange(n, device=t.device), t.lengths())
        out.index_put_((r, _u16(t.idx)), _u16(t.cnt).to(dtype), accumulate=True)
        tot = out.sum(1, keepdim=True)
        return out / torch.where(tot > 0, tot, torch.ones_like(tot))
