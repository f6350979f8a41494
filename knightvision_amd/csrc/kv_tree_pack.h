// Re-rooting a search tree in place: the subtree of one node packed to the front of the tree's pools
// (DESIGN.md "Search sessions"). Shared by k_search_advance (kv_search.hip) and k_mcts_carry (kv_mcts.hip).
// The kept set is one bit per old node id in LDS (8 KB at KV_MAX_SIMS) with the count of kept nodes below
// each 32-id word beside it, so the old id -> new id map is a rank query, new id = kept nodes below the old
// id, and needs no table of ids.
#pragma once
#include "kv_engine.h"

namespace kv {

constexpr int KEEP_WORDS = 65536 / 32 + 2;  // a bit for every 16-bit child id, and the word a 64-id chunk reads past
static_assert(KV_MAX_SIMS + 2 <= 65536, "node ids are 16-bit");

__device__ inline int keep_rank(const uint32_t* keep, const int* below, int id) {
    return below[id >> 5] + __popc(keep[id >> 5] & ((1u << (id & 31)) - 1u));
}

// the kept ids of the 64-id chunk at `base` that lie above chunk bit `b` (b = -1: all)
__device__ inline uint64_t keep_chunk_above(const uint32_t* keep, int base, int b) {
    const uint64_t mk = (uint64_t)keep[base >> 5] | ((uint64_t)keep[(base >> 5) + 1] << 32);
    return b >= 63 ? 0ull : mk & (~0ull << (b + 1));
}

struct PackedTree {
    int nodes;         // kept nodes by the renumbering
    int moved;         // nodes the move phase wrote (equal to `nodes` unless the tree is inconsistent)
    int edges;         // end of the last kept edge block
    float root_value;  // NodeRec::value of the new root, as a float
};

// The subtree of node c (0 < c < ncount) of the tree at edge base eb / node base nb becomes the tree: c is
// node 0 with its edges at offset 0 and visit count root_n, kept nodes are renumbered in old-id order, edge
// blocks move down to 16-edge boundaries, e_child is remapped, N / W / P / move words and NodeRec::value are
// carried bit for bit. All 64 lanes of the tree's wavefront; keep / below: KEEP_WORDS words of LDS each.
__device__ inline PackedTree tree_pack_subtree(const Tree& t, size_t eb, size_t nb, int c, int ncount, int root_n,
                                               uint32_t* keep, int* below) {
    const int lane = threadIdx.x;
    PackedTree out = {0, 0, 0, 0.f};
    // mark: one ascending pass over the old ids, a child's id being larger than its parent's
    for (int x = lane; x < KEEP_WORDS; x += 64) keep[x] = 0;
    __syncthreads();
    if (lane == 0) keep[c >> 5] = 1u << (c & 31);
    for (int base = c & ~63; base < ncount; base += 64) {
        const NodeRec mine = base + lane < ncount ? t.node[nb + base + lane] : NodeRec{0, 0, 0, 0};
        int b = -1;
        for (;;) {
            __syncthreads();  // the marks of the node before
            const uint64_t mk = keep_chunk_above(keep, base, b);
            if (mk == 0ull) break;
            b = __ffsll((unsigned long long)mk) - 1;
            if (base + b >= ncount) break;
            const int first = __shfl(mine.first, b), cnt = __shfl(mine.cnt, b);
            for (int j = lane; j < cnt; j += 64) {
                const int ch = t.e_child[eb + first + j];
                if (ch != NO_CHILD) atomicOr(&keep[ch >> 5], 1u << (ch & 31));
            }
        }
    }
    __syncthreads();
    // renumber: kept nodes below every word, each lane summing a run of words
    {
        const int words = (ncount + 31) >> 5, per = (words + 63) >> 6;
        const int w0 = min(lane * per, words), w1 = min(w0 + per, words);
        int mine = 0;
        for (int x = w0; x < w1; ++x) mine += __popc(keep[x]);
        int total = 0;
        int run = wave_excl_scan(mine, lane, total);
        for (int x = w0; x < w1; ++x) {
            below[x] = run;
            run += __popc(keep[x]);
        }
        out.nodes = total;
    }
    __syncthreads();
    // move, in old id order: new id <= old id and new offset <= old offset, so a block only ever
    // lands on places already read; each 64-edge chunk is read whole before it is written
    int new_id = 0, edges = 0;
    for (int base = c & ~63; base < ncount; base += 64) {
        const NodeRec mine = base + lane < ncount ? t.node[nb + base + lane] : NodeRec{0, 0, 0, 0};
        int b = -1;
        for (;;) {
            const uint64_t mk = keep_chunk_above(keep, base, b);
            if (mk == 0ull) break;
            b = __ffsll((unsigned long long)mk) - 1;
            if (base + b >= ncount) break;
            const int first = __shfl(mine.first, b), cnt = __shfl(mine.cnt, b), val = __shfl(mine.value, b);
            const int nf = (edges + 15) & ~15;
            for (int j0 = 0; j0 < cnt; j0 += 64) {
                const int j = j0 + lane;
                const bool in = j < cnt;
                const size_t eo = eb + first + (in ? j : 0);
                const uint16_t e_mv = t.e_move[eo], e_n = t.e_N[eo];
                const float e_p = t.e_P[eo], e_w = t.e_W[eo];
                const int ch = t.e_child[eo];
                __syncthreads();
                if (in) {
                    const size_t en = eb + nf + j;
                    t.e_move[en] = e_mv;
                    t.e_P[en] = e_p;
                    t.e_N[en] = e_n;
                    t.e_W[en] = e_w;
                    t.e_child[en] = ch == NO_CHILD ? NO_CHILD : (uint16_t)keep_rank(keep, below, ch);
                }
                __syncthreads();
            }
            if (new_id == 0) out.root_value = __int_as_float(val);
            // the root's visit count is the played edge's: 1 + the sum of its own edges' (a fresh root's 1)
            if (lane == 0) t.node[nb + new_id] = NodeRec{nf, cnt, new_id == 0 ? root_n : 0, val};
            new_id += 1;
            edges = nf + cnt;
        }
    }
    out.moved = new_id;
    out.edges = edges;
    __syncthreads();
    return out;
}

}  // namespace kv
