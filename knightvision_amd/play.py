"""Inference-only move choice for the GUI / evaluation callers (SURVEY.md 8f
rank 3): play_vs_model.get_ai_move (scripts/play_vs_model.py:34-49) and the
masked argmax of stockfish_play.py:64-84, on the HIP network (batch 1, the
split-K small-batch class) and the device rules.
"""
from __future__ import annotations

import numpy as np
import torch

from .ai import encode_board, encode_move


def get_ai_move(gs, model):
    """Greedy move of play_vs_model.get_ai_move: softmax of the policy row,
    the legal entries in list order, normalised; the first maximum wins, the
    first move when every legal probability is 0."""
    valid = gs.getValidMoves()
    x = torch.tensor(np.asarray([encode_board(gs.board)], dtype=np.float32))
    with torch.no_grad():
        logits, _ = model(x)
    policy = torch.softmax(logits.squeeze(), dim=0).cpu().numpy()
    legal = [policy[encode_move(m.startRow, m.startCol, m.endRow, m.endCol)] for m in valid]
    total = sum(legal)
    if total == 0:
        return valid[0]
    norm = [w / total for w in legal]
    return valid[norm.index(max(norm))]


def search_move(gs, searcher, sims=800, leaves=32):
    """The PUCT search's move for the position (engine.PositionSearch): the entry of gs.getValidMoves() at the
    root list index with the most visits (the first of equal maxima); None at a root that is not searched
    (no legal move, or kings only)."""
    valid = gs.getValidMoves()
    row = searcher.search(gs._state()[None], sims, leaves=leaves)[0]
    if row["status"] != 0:
        return None
    return valid[int(row["best"])]


class SearchSession:
    """A game followed by one search tree (engine.PositionSearch's session calls): the subtree under every
    move played is searched on at the next best_move() instead of being rebuilt. Both sides' moves go through
    push(); a move the search never expanded simply starts a fresh tree."""

    def __init__(self, gs, searcher, sims=800, leaves=32):
        self.gs, self.searcher, self.sims, self.leaves = gs, searcher, sims, leaves
        self.row = None    # the last search result of the current position
        self.kept = 0      # root visits the last best_move() found already there
        self._live = False  # the searcher's session stands at gs's position

    def best_move(self):
        """The search's move for the current position (search_move's rule), None at a root that is not
        searched; the first call searches the position, later ones resume its tree."""
        valid = self.gs.getValidMoves()
        if self._live:
            rows, kept = self.searcher.resume(self.sims, leaves=self.leaves)
            self.row, self.kept = rows[0], int(kept[0])
        else:
            self.row, self.kept = self.searcher.search(self.gs._state()[None], self.sims, leaves=self.leaves)[0], 0
            self._live = True
        if self.row["status"] != 0:
            return None
        return valid[int(self.row["best"])]

    def push(self, move):
        """Play `move` (an entry of gs.getValidMoves()) on the game and in the tree."""
        index = self.gs.getValidMoves().index(move)
        if self._live:
            self.searcher.advance([index])
        self.gs.makeMove(move)
        self.row = None


def masked_argmax_move(logits: torch.Tensor, legal_indices) -> int:
    """stockfish_play.py:64-84: argmax of the logits restricted to the legal
    move indices (encode_move), -1 when there are none."""
    if len(legal_indices) == 0:
        return -1
    row = logits.reshape(-1)
    mask = torch.full_like(row, float("-inf"))
    idx = torch.as_tensor(list(legal_indices), device=row.device, dtype=torch.long)
    mask[idx] = 0.0
    return int(torch.argmax(row + mask).item())
