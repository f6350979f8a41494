// PUCT search of given positions (kv_search, include/kv.h): the self-play
// search of kv_mcts.hip from any root, with L descents in flight per tree and
// sim-step under virtual loss, so that one position fills a network batch of L
// rows (DESIGN.md "MCTS semantics"; restated on the CPU in
// tests/_mcts_search.py). One wavefront per tree.
//
// Per search:
//   load   : state vectors -> slots, boards and root move lists (wave_valid_moves);
//            a root with kings only or without a legal move is not searched
//   root   : k_mcts_root itself (kv_mcts.hip) on the positions' network rows
//   step x : select (up to L descents per tree, one after the other: each sees
//            the in-flight counts V of the ones before it, every in-flight
//            descent counting as a loss for the mover; a pending leaf that an
//            earlier descent of the step already holds ends the step's descents)
//            -> the pending leaves of all trees as one network batch, row
//            tree * L + j -> backup (expansions and W / N updates in j order,
//            V back to 0). Backup of step k and select of step k + 1 are one launch.
//   result : root visits, q, priors, best move, principal variation
// A search session (kv_search_advance / kv_search_continue) follows a game:
//   advance: play a root move; its child's subtree is packed to the front of the
//            tree's pools in place (or the tree dropped when there is no child)
//   resume : the per-call reset, then the sim-steps above up to the root's
//            visit target, carried visits counting
// kv_run with kv_config.leaves > 1 plays self-play and arena games on the same sim-step (k_leaves_* below, the
// device functions shared through their SP parameter; the dense leaf batch is kv_engine.hip's).
// The kernels are templated on HASV: without it (L = 1) no V is read or
// written and every score is kv_mcts.hip's puct() itself, so the search is
// the self-play one bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>

#include "kv_engine.h"
#include "kv_tree_pack.h"

#pragma clang fp contract(off)

namespace kv {

// PUCT score with V descents in flight through the edge, each a loss for the
// mover; puct()'s operation order (V = 0 gives its bits)
__device__ inline float puct_inflight(float c_puct, float P, float sq, int N, int V, float W) {
    const int nv = N + V;
    const float u = c_puct * P * sq / (float)(1 + nv);
    const float q = nv > 0 ? (W - (float)V) / (float)nv : 0.0f;
    return q + u;
}

__global__ __launch_bounds__(64) void k_search_load(Tree t, SearchWs w, Slot* slots, int8_t* boards, uint16_t* moves,
                                                    int8_t* root_rows, uint32_t* np_mt, const int8_t* states,
                                                    unsigned long long seed, int L, Ctr* ctr) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int8_t* v = states + (size_t)i * 80;
    const int8_t code = v[lane];
    Pos p = wave_pos(code, v[64], v[65], v[66], v[67], v[68],
                     (v[69] ? F_WKM : 0) | (v[70] ? F_BKM : 0) | (v[71] ? F_WRK : 0) | (v[72] ? F_WRQ : 0) |
                         (v[73] ? F_BRK : 0) | (v[74] ? F_BRQ : 0),
                     v[75] < 0 ? -1 : v[75] * 8 + v[76]);
    const bool kings_only = __ballot(code != 0 && code != 1 && code != 7) == 0ull;  // GameState.isDraw
    int n = 0;
    if (!kings_only) {
        n = wave_valid_moves(p, moves + (size_t)i * MAXM, MAXM, lane);
        if (n > MAXM && lane == 0) atomicOr(&ctr->error, 1);
        n = n < MAXM ? n : MAXM;
    }
    // the board the network sees is the one getValidMoves leaves (k_movegen)
    const int8_t after = kings_only ? code : (int8_t)pos_at(p, lane);
    boards[(size_t)i * 64 + lane] = after;
    root_rows[(size_t)i * 64 + lane] = after;
    for (int j = lane; j < L; j += 64) w.lcnt[(size_t)i * L + j] = 0;
    if (t.e_V)
        for (int j = lane; j < n; j += 64) t.e_V[(size_t)i * t.ecap + j] = 0;
    if (lane != 0) return;
    SearchSlot ss;
    ss.status = kings_only ? SR_DRAW : n > 0 ? SR_SEARCHED : in_check(p) ? SR_CHECKMATED : SR_STALEMATE;
    ss.done = 0;
    ss.vroot = 0;
    ss.accepted = 0;
    ss.steps = 0;
    ss.leaf_rows = 0;
    ss.term_value = ss.status == SR_CHECKMATED ? (p.wtm ? -1.f : 1.f) : 0.f;
    ss.pad = 0;
    w.ss[i] = ss;
    Slot s = slots[i];
    s.status = ss.status == SR_SEARCHED ? ST_ACTIVE : ST_IDLE;  // k_mcts_root takes the active slots
    s.ply = 0;
    s.wtm = p.wtm;
    s.wkr = p.wkr; s.wkc = p.wkc; s.bkr = p.bkr; s.bkc = p.bkc;
    s.flags = p.flags;
    s.ep = p.ep;
    s.nmoves = n;
    if (ss.status == SR_SEARCHED) s.rows_total += 1;  // the root's network row (kv_stats.nn_rows)
    slots[i] = s;
    mt_seed_genrand(np_mt + (size_t)i * MT_WORDS, (uint32_t)(seed + (unsigned long long)i));
}

// one tree's descents of a sim-step, by the 64 threads of its workgroup. SP: the tree is a self-play slot's
// (kv_config.leaves > 1, k_leaves_* below): it is searched while the slot is active and its root holds fewer than
// sims backups, and ss.done is written for the step's compaction (sims for a slot that takes no descent)
// (kv_config.fast_sims: fewer than the ply's own target, Tree::tgt). FORCED (SP trees with kv_config.forced_k > 0):
// kv_mcts.hip's forced rule at node 0 of a full ply, on N + V and the root's visit sum nd.N + vroot - 1
template <bool HASV, bool SP = false, bool FORCED = false>
__device__ inline void search_select_tree(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards,
                                          Ctr* ctr, int sims, int L, int i) {
    if (SP && t.tgt != nullptr) sims = t.tgt[i];
    const bool force = FORCED && sims == t.sims;  // a fast ply has no forcing
    int forced = 0;
    __shared__ int8_t root_bd[64];
    __shared__ int8_t bd[64];
    __shared__ int s_meta[8];                // wtm wkr wkc bkr bkc flags ep
    __shared__ int s_held[KV_MAX_LEAVES];    // leaf edges of the step's accepted pending descents
    const int lane = threadIdx.x;
    SearchSlot ss = w.ss[i];
    const size_t row0 = (size_t)i * L;
    int accepted = 0;
    if (SP) {
        const bool active = slots[i].status == ST_ACTIVE;
        ss.status = active ? SR_SEARCHED : SR_DRAW;
        ss.done = active ? t.node[(size_t)i * t.ncap].N - 1 : sims;
    }
    if (ss.status == SR_SEARCHED && ss.done < sims) {
        const Slot s = slots[i];
        root_bd[lane] = boards[(size_t)i * 64 + lane];
        const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
        const int r = min(L, sims - ss.done);
        int vroot = 0, held = 0;
        for (int j = 0; j < r; ++j) {
            __syncthreads();  // the descent before: its board reads, its V writes
            bd[lane] = root_bd[lane];
            if (lane == 0) {
                s_meta[0] = s.wtm; s_meta[1] = s.wkr; s_meta[2] = s.wkc; s_meta[3] = s.bkr; s_meta[4] = s.bkc;
                s_meta[5] = s.flags; s_meta[6] = s.ep;
            }
            __syncthreads();
            const size_t row = row0 + j;
            int* path = w.paths + row * t.ncap;
            int node = 0, depth = 0, leaf = -1, parent_n = 0;
            bool by_force = false;
            for (;;) {
                const NodeRec nd = t.node[nb + node];
                const int first = nd.first, cnt = nd.cnt;
                const float sq = t.sqrt_tab[node == 0 ? nd.N + vroot : parent_n];
                float best = -INFINITY;
                int bi = 0x7fffffff;
                for (int k = lane; k < cnt; k += 64) {
                    const size_t e = eb + first + k;
                    float sc = HASV ? puct_inflight(t.c_puct, t.e_P[e], sq, t.e_N[e], t.e_V[e], t.e_W[e])
                                    : puct(t.c_puct, t.e_P[e], sq, t.e_N[e], t.e_W[e]);
                    if (FORCED && force && node == 0 &&
                        forced_edge(t.forced_k, t.e_P[e], t.e_N[e] + t.e_V[e], nd.N + vroot - 1))
                        sc = INFINITY;
                    if (sc > best) {  // lanes see their edges in increasing k: strict > keeps the first
                        best = sc;
                        bi = k;
                    }
                }
                wave_argmax_first(best, bi);
                if (FORCED && force && node == 0) by_force = best == INFINITY;
                if (bi >= cnt) bi = 0;  // no score compared greater (NaN priors): stay inside the node's edges
                const int e = first + bi;
                if (lane == 0) {
                    path[depth] = e;
                    make_move_board(bd, s_meta[0], s_meta[1], s_meta[2], s_meta[3], s_meta[4], s_meta[5], s_meta[6],
                                    t.e_move[eb + e]);
                }
                ++depth;
                __syncthreads();
                const int child = t.e_child[eb + e];
                if (child == NO_CHILD || depth >= t.ncap) {
                    leaf = e;
                    break;
                }
                parent_n = t.e_N[eb + e];
                if (HASV) parent_n += t.e_V[eb + e];
                node = child;
            }
            // a leaf edge that an earlier descent of this step holds for the network: the same position
            // again, so this descent is dropped before anything was incremented and the step's descents end
            if (HASV && __ballot(lane < held && s_held[lane] == leaf) != 0ull) break;
            SearchLeaf lf;
            lf.path_len = depth;
            lf.leaf_edge = leaf;
            lf.pending = 0;
            lf.n = 0;
            lf.value = 0.f;
            lf.pad[0] = lf.pad[1] = lf.pad[2] = 0;
            const int8_t code = bd[lane];
            int8_t out = code;
            if (__ballot(code != 0 && code != 1 && code != 7) != 0ull) {  // else isDraw: value 0
                Pos p = wave_pos(code, s_meta[0], s_meta[1], s_meta[2], s_meta[3], s_meta[4], s_meta[5], s_meta[6]);
                const int n = wave_valid_moves(p, w.lmoves + row * MAXM, MAXM, lane);
                if (n > MAXM && lane == 0) atomicOr(&ctr->error, 1);
                if (n == 0) {
                    lf.value = in_check(p) ? (p.wtm ? -1.f : 1.f) : 0.f;  // mate / stalemate
                } else {
                    out = (int8_t)pos_at(p, lane);  // the board the reference would encode (after getValidMoves)
                    lf.pending = 1;
                    lf.n = n < MAXM ? n : MAXM;
                }
            }
            if (lf.pending) w.lboards[row * 64 + lane] = out;
            if (HASV)  // accepted: one more descent in flight on every edge of the path
                for (int d = lane; d < depth; d += 64) t.e_V[eb + path[d]] += 1;
            vroot += 1;
            if (FORCED && by_force) forced += 1;  // (an accepted descent: a dropped one counts nowhere)
            if (lane == 0) {
                w.lf[row] = lf;
                w.lcnt[row] = lf.pending ? lf.n : 0;
                if (lf.pending) s_held[held] = leaf;
            }
            held += lf.pending;
            accepted += 1;
        }
    }
    for (int j = accepted + lane; j < L; j += 64) w.lcnt[row0 + j] = 0;  // no logits for the unused rows
    if (lane == 0) {
        ss.accepted = accepted;
        ss.vroot = accepted;
        w.ss[i] = ss;
        if (FORCED && forced) t.forced[i] += forced;  // (k_mcts_choose adds the ply's count to Ctr::forced_descents)
    }
}

// one tree's backups of a sim-step, by the 64 threads of its workgroup. SP (a self-play slot): the leaf rows are
// also counted in MctsSlot::pad[1], which k_mcts_choose adds to Ctr::nn_rows, and the host's counter is the
// compaction's (k_leaves_compact), not w.remaining
template <bool HASV, bool SP = false>
__device__ inline void search_backup_tree(const Tree& t, const SearchWs& w, Ctr* ctr, int sims, int L, int i) {
    __shared__ float pri[MAXM];
    const int lane = threadIdx.x;
    SearchSlot ss = w.ss[i];
    if (ss.status != SR_SEARCHED || ss.accepted == 0) return;
    MctsSlot m = t.ms[i];
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    for (int j = 0; j < ss.accepted; ++j) {
        const size_t row = (size_t)i * L + j;
        const SearchLeaf lf = w.lf[row];
        float v = lf.value;
        if (lf.pending) {
            v = w.lvalues[row];
            // mcts_backup_slot's priors: max, e_k = det_expf(l_k - max) kept in LDS, lane partial sums
            // over k = lane, lane+64, ... in order, xor butterfly
            const float* lg = w.llogits + row * MAXM;
            const uint16_t* lm = w.lmoves + row * MAXM;
            const int n = lf.n;
            float mx = -INFINITY;
            for (int k = lane; k < n; k += 64) {
                const float l = lg[k];
                pri[k] = l;
                mx = fmaxf(mx, l);
            }
            mx = wave_max(mx);
            float part = 0.f;
            for (int k = lane; k < n; k += 64) {
                const float e = det_expf(pri[k] - mx);
                pri[k] = e;
                part += e;
            }
            const float sum = wave_sum(part);
            const int first = (m.edge_count + 15) & ~15;
            const bool fits = first + n <= t.ecap && m.node_count < t.ncap;
            if (fits) {
                for (int k = lane; k < n; k += 64) {
                    const size_t e = eb + first + k;
                    t.e_move[e] = lm[k];
                    t.e_P[e] = sum > 0.f ? pri[k] / sum : 1.0f / (float)n;
                    t.e_N[e] = 0;
                    t.e_W[e] = 0.f;
                    t.e_child[e] = NO_CHILD;
                    if (HASV) t.e_V[e] = 0;
                }
                if (lane == 0) {
                    t.node[nb + m.node_count] = NodeRec{first, n, 0, __float_as_int(v)};
                    t.e_child[eb + lf.leaf_edge] = (uint16_t)m.node_count;
                }
                m.node_count += 1;
                m.edge_count = first + n;
            } else {
                // the expansion does not fit the tree's pools: counted and raised as an error
                // (kv_search -> KV_EOVERFLOW), never silent
                m.overflow += 1;
                if (lane == 0) {
                    atomicAdd(&ctr->tree_overflows, 1ull);
                    atomicOr(&ctr->error, 4);
                }
            }
            m.pad[0] += 1;
            if (SP) m.pad[1] += 1;
            ss.leaf_rows += 1;
        }
        // along the path (its edges are distinct): the mover at depth d is the root side flipped d times
        const int* path = w.paths + row * t.ncap;
        for (int d = lane; d < lf.path_len; d += 64) {
            const size_t e = eb + path[d];
            const bool white_moved = ((m.root_wtm != 0) ^ (d & 1)) != 0;
            if (HASV) t.e_V[e] -= 1;
            t.e_N[e] += 1;
            t.e_W[e] = t.e_W[e] + (white_moved ? v : -v);
        }
        __syncthreads();  // this backup's tree writes before the next one's reads
    }
    if (lane == 0) {
        t.node[nb].N += ss.accepted;
        ss.done += ss.accepted;
        ss.steps += 1;
        ss.accepted = 0;
        ss.vroot = 0;
        w.ss[i] = ss;
        t.ms[i] = m;
        if (!SP && ss.done < sims) atomicAdd(w.remaining, 1);  // the host's one readback per step
    }
}

template <bool HASV>
__global__ __launch_bounds__(64) void k_search_select(Tree t, SearchWs w, const Slot* slots, const int8_t* boards,
                                                      Ctr* ctr, int sims, int L) {
    search_select_tree<HASV>(t, w, slots, boards, ctr, sims, L, blockIdx.x);
}

// backup of sim-step k and select of sim-step k + 1 of the same tree in one launch (k_mcts_backup_select);
// the barrier orders the backup's tree writes before the descents read them (workgroup scope)
template <bool HASV>
__global__ __launch_bounds__(64) void k_search_backup_select(Tree t, SearchWs w, const Slot* slots,
                                                             const int8_t* boards, Ctr* ctr, int sims, int L) {
    search_backup_tree<HASV>(t, w, ctr, sims, L, blockIdx.x);
    __syncthreads();
    search_select_tree<HASV>(t, w, slots, boards, ctr, sims, L, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_search_result(Tree t, SearchWs w, const Slot* slots, Ctr* ctr, int sims,
                                                      int session) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const SearchSlot ss = w.ss[i];
    const MctsSlot m = t.ms[i];
    kv_search_result* o = w.res + i;
    const bool searched = ss.status == SR_SEARCHED;
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    const int n = searched ? t.node[nb].cnt : 0;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = lane; j < MAXM; j += 64) {
        const bool in = j < n;
        const int N = in ? t.e_N[eb + j] : -1;
        o->moves[j] = in ? t.e_move[eb + j] : (uint16_t)0;
        o->visits[j] = N;
        o->q[j] = N > 0 ? t.e_W[eb + j] / (float)N : 0.0f;
        o->prior[j] = in ? t.e_P[eb + j] : 0.0f;
        if (in && (float)N > best) {
            best = (float)N;
            bi = j;
        }
    }
    wave_argmax_first(best, bi);
    // principal variation: the first maximum of the visit counts at every node, through expanded children
    int node = 0, len = 0;
    uint16_t pv = 0;  // lane d keeps ply d
    while (searched && len < 16) {
        const NodeRec nd = t.node[nb + node];
        float b = -INFINITY;
        int k0 = 0x7fffffff;
        for (int k = lane; k < nd.cnt; k += 64) {
            const float N = (float)t.e_N[eb + nd.first + k];
            if (N > b) {
                b = N;
                k0 = k;
            }
        }
        wave_argmax_first(b, k0);
        if (!(b > 0.f)) break;  // no visited edge below this node
        const size_t e = eb + nd.first + k0;
        if (lane == len) pv = t.e_move[e];
        ++len;
        const int child = t.e_child[e];
        if (child == NO_CHILD) break;
        node = child;
    }
    if (lane < 16) o->pv[lane] = lane < len ? pv : (uint16_t)0;
    if (lane != 0) return;
    o->status = ss.status;
    o->n_moves = n;
    o->sims = ss.done;
    o->best = searched ? bi : -1;
    o->pv_len = len;
    o->steps = ss.steps;
    // a session's continue counts this call only: no root row for a carried tree, the new backups
    const SessionSlot se = session ? w.sess[i] : SessionSlot{};
    o->nn_rows = searched ? (session ? se.root_row : 1) + ss.leaf_rows : 0;
    o->pad = 0;
    o->root_value = searched ? m.root_value : ss.term_value;
    const int bN = searched ? t.e_N[eb + bi] : 0;
    o->best_q = bN > 0 ? t.e_W[eb + bi] / (float)bN : 0.0f;
    if (searched) {
        atomicAdd(&ctr->sims, (unsigned long long)(ss.done - (session ? se.kept : 0)));
        atomicAdd(&ctr->nn_rows, (unsigned long long)ss.leaf_rows);
    }
}

// ---- self-play and arena with several leaves per game (kv_config.leaves > 1, DESIGN.md "Several leaves per game
// in self-play"): the sim-step above on the slots' own trees, after k_mcts_root. One wavefront per slot; the leaf
// of descent j of slot i is row i * L + j of w. e_V is all 0 between sim-steps (every accepted descent's increments
// are taken back by its backup, an expansion zeroes its edges'), so the roots k_mcts_root builds need no reset.
template <bool FORCED>
__global__ __launch_bounds__(64) void k_leaves_select(Tree t, SearchWs w, const Slot* slots, const int8_t* boards,
                                                      Ctr* ctr, int sims, int L) {
    search_select_tree<true, true, FORCED>(t, w, slots, boards, ctr, sims, L, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_leaves_backup(Tree t, SearchWs w, Ctr* ctr, int sims, int L) {
    search_backup_tree<true, true>(t, w, ctr, sims, L, blockIdx.x);
}

// backup of sim-step k and select of sim-step k + 1 of the same slot in one launch (k_mcts_backup_select)
template <bool FORCED>
__global__ __launch_bounds__(64) void k_leaves_backup_select(Tree t, SearchWs w, const Slot* slots,
                                                             const int8_t* boards, Ctr* ctr, int sims, int L) {
    search_backup_tree<true, true>(t, w, ctr, sims, L, blockIdx.x);
    __syncthreads();
    search_select_tree<true, true, FORCED>(t, w, slots, boards, ctr, sims, L, blockIdx.x);
}

int leaves_select(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr, int sims,
                  int n, int L, hipStream_t st) {
    // (kv_config.forced_k > 0: the FORCED instances; 0 launches the kernels without the feature)
    hipLaunchKernelGGL(t.forced_k > 0.f ? k_leaves_select<true> : k_leaves_select<false>, dim3(n), dim3(64), 0, st, t,
                       w, slots, boards, ctr, sims, L);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int leaves_backup(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr, int sims,
                  int n, int L, bool select, hipStream_t st) {
    if (select)
        hipLaunchKernelGGL(t.forced_k > 0.f ? k_leaves_backup_select<true> : k_leaves_backup_select<false>, dim3(n),
                           dim3(64), 0, st, t, w, slots, boards, ctr, sims, L);
    else
        hipLaunchKernelGGL(k_leaves_backup, dim3(n), dim3(64), 0, st, t, w, ctr, sims, L);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

// ---- search sessions (DESIGN.md "Search sessions") ----
// the re-root itself (mark / renumber / move) is tree_pack_subtree, kv_tree_pack.h

// Play root edge edge[i] in tree i: the slot's position becomes the one after the move (k_search_load's root
// move generation), and the subtree of the edge's child is packed to the front of the tree's pools in place;
// without a child the tree is dropped and the next continue builds a fresh root. One wavefront per tree.
__global__ __launch_bounds__(64) void k_search_advance(Tree t, SearchWs w, Slot* slots, int8_t* boards,
                                                       uint16_t* moves, int8_t* root_rows, const int* edge,
                                                       int8_t* states, Ctr* ctr) {
    __shared__ uint32_t keep[KEEP_WORDS];
    __shared__ int below[KEEP_WORDS];
    __shared__ int8_t bd[64];
    __shared__ int s_meta[8];  // wtm wkr wkc bkr bkc flags ep
    const int i = blockIdx.x, lane = threadIdx.x;
    const int k = edge[i];
    if (k < 0) return;  // this tree stays as it is
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    SearchSlot ss = w.ss[i];
    MctsSlot m = t.ms[i];
    Slot s = slots[i];
    if (ss.status != SR_SEARCHED || k >= s.nmoves) {  // the host checked both against the last result
        if (lane == 0) atomicOr(&ctr->error, 32);
        return;
    }
    // a tree dropped by the advance before and not continued since has no node yet: dropped again
    const bool built = w.sess[i].fresh == 0;
    const uint16_t mv = moves[(size_t)i * MAXM + k];  // the root list is node 0's move words
    const int c = built ? (int)t.e_child[eb + k] : (int)NO_CHILD;
    const int played_n = built ? (int)t.e_N[eb + k] : 0;
    // 1. the position after the move, as the oracle's make_valid_move gives it
    bd[lane] = boards[(size_t)i * 64 + lane];
    if (lane == 0) {
        s_meta[0] = s.wtm; s_meta[1] = s.wkr; s_meta[2] = s.wkc; s_meta[3] = s.bkr; s_meta[4] = s.bkc;
        s_meta[5] = s.flags; s_meta[6] = s.ep;
    }
    __syncthreads();
    if (lane == 0) make_move_board(bd, s_meta[0], s_meta[1], s_meta[2], s_meta[3], s_meta[4], s_meta[5], s_meta[6], mv);
    __syncthreads();
    const int8_t code = bd[lane];
    int8_t* so = states + (size_t)i * 80;
    so[lane] = code;
    if (lane < 16) {
        const int fl = s_meta[5], ep = s_meta[6];
        int8_t x = 0;
        if (lane <= 4) x = (int8_t)s_meta[lane];
        else if (lane <= 10) x = (int8_t)((fl >> (lane - 5)) & 1);  // F_WKM .. F_BRQ in vector order
        else if (lane == 11) x = (int8_t)(ep < 0 ? -1 : ep >> 3);
        else if (lane == 12) x = (int8_t)(ep < 0 ? -1 : ep & 7);
        so[64 + lane] = x;
    }
    // 2. the new root's move list, keeping the board as getValidMoves leaves it (k_search_load)
    Pos p = wave_pos(code, s_meta[0], s_meta[1], s_meta[2], s_meta[3], s_meta[4], s_meta[5], s_meta[6]);
    const bool kings_only = __ballot(code != 0 && code != 1 && code != 7) == 0ull;
    uint16_t* ml = moves + (size_t)i * MAXM;
    int n = 0;
    if (!kings_only) {
        n = wave_valid_moves(p, ml, MAXM, lane);
        if (n > MAXM && lane == 0) atomicOr(&ctr->error, 1);
        n = n < MAXM ? n : MAXM;
    }
    const int8_t after = kings_only ? code : (int8_t)pos_at(p, lane);
    boards[(size_t)i * 64 + lane] = after;
    root_rows[(size_t)i * 64 + lane] = after;
    const int status = kings_only ? SR_DRAW : n > 0 ? SR_SEARCHED : in_check(p) ? SR_CHECKMATED : SR_STALEMATE;
    const bool carried = c != NO_CHILD;
    int kept_nodes = 0, kept_edges = 0;
    float root_value = 0.f;
    if (carried) {
        // 3. the child's subtree packed to the front of the pools (mark / renumber / move)
        const PackedTree pk = tree_pack_subtree(t, eb, nb, c, m.node_count, played_n, keep, below);
        kept_nodes = pk.nodes;
        kept_edges = pk.edges;
        root_value = pk.root_value;
        const int new_id = pk.moved;
        // self-check: the regenerated root move list is node 0's
        const NodeRec r0 = t.node[nb];
        bool bad = status != SR_SEARCHED || r0.cnt != n || new_id != kept_nodes;
        for (int j = lane; j < n && j < r0.cnt; j += 64) bad = bad || t.e_move[eb + r0.first + j] != ml[j];
        if (__ballot(bad) != 0ull && lane == 0) atomicOr(&ctr->error, 32);
    }
    if (lane != 0) return;
    ss.status = status;
    ss.done = carried ? played_n - 1 : 0;
    ss.vroot = 0;
    ss.accepted = 0;
    ss.steps = 0;
    ss.leaf_rows = 0;
    ss.term_value = status == SR_CHECKMATED ? (p.wtm ? -1.f : 1.f) : 0.f;
    w.ss[i] = ss;
    SessionSlot se = {};
    se.status = status;
    se.n_moves = n;
    se.kept = carried ? played_n - 1 : 0;
    se.fresh = carried ? 0 : 1;
    w.sess[i] = se;
    m.node_count = kept_nodes;  // 0 for a dropped tree until its root is built
    m.edge_count = kept_edges;
    if (carried) {
        m.root_value = root_value;
        m.root_wtm = p.wtm;
    }
    t.ms[i] = m;
    s.status = ST_IDLE;  // k_search_resume hands the fresh roots to k_mcts_root
    s.ply = 0;
    s.wtm = p.wtm;
    s.wkr = p.wkr; s.wkc = p.wkc; s.bkr = p.bkr; s.bkc = p.bkc;
    s.flags = p.flags;
    s.ep = p.ep;
    s.nmoves = n;
    slots[i] = s;
}

// The per-call reset of a continue: the call's own counters, the carried visits, and for a dropped tree
// what k_search_load prepares for k_mcts_root.
__global__ __launch_bounds__(64) void k_search_resume(Tree t, SearchWs w, Slot* slots, uint32_t* np_mt,
                                                      unsigned long long seed, int L) {
    const int i = blockIdx.x, lane = threadIdx.x;
    SearchSlot ss = w.ss[i];
    SessionSlot se = w.sess[i];
    const bool searched = ss.status == SR_SEARCHED;
    const bool fresh = se.fresh != 0 && searched;
    for (int j = lane; j < L; j += 64) w.lcnt[(size_t)i * L + j] = 0;
    const int n = slots[i].nmoves;
    if (fresh && t.e_V)
        for (int j = lane; j < n; j += 64) t.e_V[(size_t)i * t.ecap + j] = 0;
    if (lane != 0) return;
    if (fresh) ss.done = 0;
    ss.vroot = 0;
    ss.accepted = 0;
    ss.steps = 0;
    ss.leaf_rows = 0;
    w.ss[i] = ss;
    se.status = ss.status;
    se.n_moves = searched ? n : 0;
    se.kept = searched ? ss.done : 0;
    se.fresh = 0;
    se.root_row = fresh ? 1 : 0;
    w.sess[i] = se;
    Slot s = slots[i];
    s.status = fresh ? ST_ACTIVE : ST_IDLE;  // k_mcts_root takes the active slots
    if (fresh) s.rows_total += 1;            // the root's network row (kv_stats.nn_rows)
    slots[i] = s;
    if (fresh) mt_seed_genrand(np_mt + (size_t)i * MT_WORDS, (uint32_t)(seed + (unsigned long long)i));
}

int search_advance(const Tree& t, const SearchWs& w, Slot* slots, int8_t* boards, uint16_t* moves, int8_t* root_rows,
                   const int* edge, int8_t* states, int n, Ctr* ctr, hipStream_t st) {
    hipLaunchKernelGGL(k_search_advance, dim3(n), dim3(64), 0, st, t, w, slots, boards, moves, root_rows, edge, states,
                       ctr);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int search_resume(const Tree& t, const SearchWs& w, Slot* slots, uint32_t* np_mt, unsigned long long seed, int n,
                  int L, hipStream_t st) {
    hipLaunchKernelGGL(k_search_resume, dim3(n), dim3(64), 0, st, t, w, slots, np_mt, seed, L);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int search_load(const Tree& t, const SearchWs& w, Slot* slots, int8_t* boards, uint16_t* moves, int8_t* root_rows,
                uint32_t* np_mt, const int8_t* states, unsigned long long seed, int n, int L, Ctr* ctr,
                hipStream_t st) {
    hipLaunchKernelGGL(k_search_load, dim3(n), dim3(64), 0, st, t, w, slots, boards, moves, root_rows, np_mt, states,
                       seed, L, ctr);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int search_select(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr, int sims,
                  int n, int L, hipStream_t st) {
    if (L > 1)
        hipLaunchKernelGGL(k_search_select<true>, dim3(n), dim3(64), 0, st, t, w, slots, boards, ctr, sims, L);
    else
        hipLaunchKernelGGL(k_search_select<false>, dim3(n), dim3(64), 0, st, t, w, slots, boards, ctr, sims, L);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int search_backup_select(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr,
                         int sims, int n, int L, hipStream_t st) {
    if (L > 1)
        hipLaunchKernelGGL(k_search_backup_select<true>, dim3(n), dim3(64), 0, st, t, w, slots, boards, ctr, sims, L);
    else
        hipLaunchKernelGGL(k_search_backup_select<false>, dim3(n), dim3(64), 0, st, t, w, slots, boards, ctr, sims,
                           L);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int search_result(const Tree& t, const SearchWs& w, const Slot* slots, Ctr* ctr, int sims, int n, bool session,
                  hipStream_t st) {
    hipLaunchKernelGGL(k_search_result, dim3(n), dim3(64), 0, st, t, w, slots, ctr, sims, session ? 1 : 0);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

}  // namespace kv
