// PUCT Monte-Carlo tree search on MI355X (no reference counterpart: the
// reference samples moves from the network policy, self_play.py:150-167; the
// semantics below are build-defined and restated on the CPU in
// oracle/kv_oracle.c kvo_mcts_*). One wavefront per concurrent game.
//
// Per move of each game slot:
//   root   : network row of the position; priors = the reference's own mixed
//            move distribution (softmax x (1-eps) + Dirichlet x eps over the
//            legal list, normalised; self_play.py:147-166), so the numpy
//            stream is consumed exactly as in the reference; node 0 created.
//   sims x : select (PUCT from the root: Q + c_puct * P * sqrt(N_parent) /
//            (1 + N_child), Q = W/N or 0, first maximum in move-list order) ->
//            apply the path's moves to the slot's board -> leaf = first edge
//            with no child: isDraw => value 0; no legal moves => mate (-1 for
//            the side to move) or stalemate 0; else the leaf board joins this
//            step's network batch (one row per slot) -> backup: priors =
//            softmax over the legal moves' logits only, node created, N += 1
//            and W += value from the mover's side along the path (the value
//            head is white-perspective, self_play.py:253).
//            Softmaxes use det_expf (kv_engine.h) with a fixed summation
//            order, so the CPU restatement reproduces every prior bit for bit.
//            An expansion that does not fit the slot's edge pool (sized
//            MAXM x (sims + 1) by default, so it cannot happen unless the
//            caller shrinks it) raises KV_EOVERFLOW.
//   choose : random.choices over the root visit counts on the CPython stream
//            (tau = 1), then makeMove / record / termination as the reference.
//            kv_config.sample_plies: from that ply on (-1: from the first) the first
//            maximum of the visit counts instead, the CPython stream not advanced.
// kv_config.arena (kv_engine.hip eng_arena_ply): each ply's root and leaf rows come from the net of the side to
// move at the root; select / backup then also run over a slot list (one player's slots) instead of a range.
// With kv_config.reuse_tree the subtree under the move just played is carried into the next ply
// (k_mcts_carry, DESIGN.md "Carried subtrees in self-play"): the root takes the fresh root's mixed priors, N,
// W and the children below it stay, and a slot searches only while its root holds fewer than sims visits.
// With kv_config.fast_sims (DESIGN.md "Playout cap randomization") every ply has a visit target of its own, sims or
// fast_sims (ply_target, kv_engine.h): k_mcts_root_pcr writes it into Tree::tgt and mixes a fast ply's noise in with
// eps = 0, the REUSE kernels search a slot while its root holds fewer visits than that, and rem is written against
// the next ply's target (k_mcts_carry, or k_mcts_targets without reuse_tree).
// With kv_config.forced_k (DESIGN.md "Forced playouts and policy target pruning") a full ply's select takes a root
// edge that holds fewer visits than its forced count before any PUCT score (forced_edge, kv_engine.h), and
// k_mcts_choose takes those visits out again where PUCT would not have made them (pruned_count): the move is drawn
// from the pruned counts T, which go to Tree::root_targets; root_visits, k_mcts_carry and every counter keep the raw N.
// Tree: structure-of-arrays edge pools per slot in HBM (move u16, P f32, N u16,
// W f32, child u16 per edge: 14 B; a node's edges start on a 16-edge boundary)
// and one 16-byte record per node (first edge, edge count; N for the root only:
// a non-root node's visit count is its parent edge's N).
#include <hip/hip_runtime.h>
#include <math.h>

#include "kv_engine.h"
#include "kv_tree_pack.h"

#pragma clang fp contract(off)

namespace kv {

// one slot's root, by the 256 threads of its workgroup. PCR (kv_config.fast_sims, Tree::tgt != NULL): the ply's
// visit target is written and a fast ply mixes its noise in with eps = 0; the false instance is the kernel without
// the feature
template <bool PCR>
__device__ __forceinline__ void mcts_root_slot(const DevCfg& cfg, const Tree& t, Slot* slots, const uint16_t* moves,
                                               const float* logits, const float* values, float* probs,
                                               uint32_t* np_mt, Ctr* ctr) {
    __shared__ uint32_t mt3[MT_RW];
    __shared__ double gam[4096];
    __shared__ double vals[MAXM];
    __shared__ int scratch[RNG_SCRATCH];
    const int i = blockIdx.x, lane = threadIdx.x;
    Slot s = slots[i];
    if (s.status != ST_ACTIVE) return;
    float* lp = probs + (size_t)i * 4096;
    if (lane < 64) wave_softmax_4096_det(logits + (size_t)i * 4096, lp, lane);
    __syncthreads();
    const int n = s.nmoves;
    const uint16_t* ml = moves + (size_t)i * MAXM;
    // kv_config.fast_sims: the ply's visit target; a fast ply's noise is drawn as ever and weighted by 0
    double eps = cfg.eps;
    if (PCR) {
        bool fast;
        const int target = ply_target(cfg, s.game_id, s.ply, &fast);
        if (fast) eps = 0.0;
        if (lane == 0) t.tgt[i] = target;
    }
    mixed_legal_weights(cfg, lp, ml, n, gam, np_mt + (size_t)i * MT_WORDS, mt3, scratch, vals, lane, eps);
    __shared__ double s_total;
    if (lane == 0) {
        double total = 0.0;
        for (int j = 0; j < n; ++j) total = total + vals[j];
        s_total = total;
    }
    __syncthreads();
    const double total = s_total;
    if (!isfinite(total)) {  // all-zero gamma draws: NaN weights (k_sample's error 8)
        if (lane == 0) atomicOr(&ctr->error, 8);
        return;
    }
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    if (t.rem != nullptr && t.ms[i].pad[2] != 0) {
        // a carried tree (k_mcts_carry): node 0 keeps its visits, values and children and takes only the
        // priors a fresh root would get; the regenerated move list must be node 0's move words
        const NodeRec r0 = t.node[nb];
        bool bad = r0.cnt != n || r0.first != 0;
        for (int j = lane; j < n && j < r0.cnt; j += 256) bad = bad || t.e_move[eb + j] != ml[j];
        if (__syncthreads_or(bad)) {
            if (lane == 0) {
                atomicOr(&ctr->error, 32);
                t.node[nb].N = t.sims + 1;  // never searched on: the slot is not live in any sim-step
            }
            return;
        }
        for (int j = lane; j < n; j += 256)
            t.e_P[eb + j] = total == 0.0 ? 1.0f / (float)n : (float)(vals[j] / total);
        if (lane == 0) {
            MctsSlot m = t.ms[i];
            m.root_value = values[i];
            m.path_len = 0;
            m.leaf_pending = 0;
            m.pad[0] = 1;
            m.pad[1] = 0;
            m.pad[4] = r0.N - 1;  // the visits carried in: they count toward sims
            t.ms[i] = m;
            slots[i].last_value = values[i];
        }
        return;
    }
    for (int j = lane; j < n; j += 256) {
        t.e_move[eb + j] = ml[j];
        t.e_P[eb + j] = total == 0.0 ? 1.0f / (float)n : (float)(vals[j] / total);
        t.e_N[eb + j] = 0;
        t.e_W[eb + j] = 0.f;
        t.e_child[eb + j] = NO_CHILD;
    }
    if (lane == 0) {
        t.node[nb] = NodeRec{0, n, 1, 0};
        MctsSlot m = t.ms[i];
        m.node_count = 1;
        m.edge_count = n;
        m.root_value = values[i];
        m.root_wtm = s.wtm;
        m.path_len = 0;
        m.leaf_pending = 0;
        m.pad[0] = 1;  // network rows consumed this move
        m.pad[1] = 0;  // leaf rows sent to the network this move (Ctr::nn_rows at the choice)
        m.pad[4] = 0;
        t.ms[i] = m;
        slots[i].last_value = values[i];
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_mcts_root(DevCfg cfg, Tree t, Slot* slots, const uint16_t* moves,
                                                   const float* logits, const float* values, float* probs,
                                                   uint32_t* np_mt, Ctr* ctr) {
    mcts_root_slot<false>(cfg, t, slots, moves, logits, values, probs, np_mt, ctr);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_mcts_root_pcr(
    DevCfg cfg, Tree t, Slot* slots, const uint16_t* moves, const float* logits, const float* values, float* probs,
    uint32_t* np_mt, Ctr* ctr) {
    mcts_root_slot<true>(cfg, t, slots, moves, logits, values, probs, np_mt, ctr);
}

// one slot's select, by the 64 threads of its workgroup. REUSE (kv_config.reuse_tree): a slot whose root
// already holds sims visits (carried ones counting; with kv_config.fast_sims the ply's own target, Tree::tgt) is not
// live: no descent, no leaf. FORCED (kv_config.forced_k > 0, DESIGN.md "Forced playouts and policy target
// pruning"): on a full ply a root edge under its forced count scores +INFINITY, so the first such edge in list order
// is taken; the false instances are the kernels without the feature
template <bool REUSE, bool FORCED = false>
__device__ inline void mcts_select_slot(const DevCfg& cfg, const Tree& t, const Slot* slots, const int8_t* boards,
                                        int8_t* nn_boards, Ctr* ctr, int i) {
    __shared__ int8_t bd[64];
    __shared__ int s_meta[8];  // wtm wkr wkc bkr bkc flags ep
    const int lane = threadIdx.x;
    const Slot s = slots[i];
    if (s.status != ST_ACTIVE || (REUSE && t.node[(size_t)i * t.ncap].N - 1 >= (t.tgt ? t.tgt[i] : t.sims))) {
        if (lane == 0) t.leaf_cnt[i] = 0;  // no logits for this row of the batch
        return;
    }
    bd[lane] = boards[(size_t)i * 64 + lane];
    if (lane == 0) {
        s_meta[0] = s.wtm; s_meta[1] = s.wkr; s_meta[2] = s.wkc; s_meta[3] = s.bkr; s_meta[4] = s.bkc;
        s_meta[5] = s.flags; s_meta[6] = s.ep;
    }
    __syncthreads();
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    int* path = t.path + nb;
    int node = 0, depth = 0, leaf = -1, parent_n = 0;
    const bool force = FORCED && (t.tgt == nullptr || t.tgt[i] == cfg.sims);  // a fast ply has no forcing
    for (;;) {
        const NodeRec nd = t.node[nb + node];
        const int first = nd.first, cnt = nd.cnt;
        // a non-root node's visit count is its parent edge's (both rise in
        // the same backups), so only the root keeps one in its record
        const float sq = t.sqrt_tab[node == 0 ? nd.N : parent_n];
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = lane; j < cnt; j += 64) {
            const size_t e = eb + first + j;
            float sc = puct(t.c_puct, t.e_P[e], sq, t.e_N[e], t.e_W[e]);
            if (FORCED && force && node == 0 && forced_edge(t.forced_k, t.e_P[e], t.e_N[e], nd.N - 1)) sc = INFINITY;
            if (sc > best) {  // lanes see their edges in increasing j: strict > keeps the first
                best = sc;
                bi = j;
            }
        }
        wave_argmax_first(best, bi);
        if (FORCED && force && node == 0 && lane == 0 && best == INFINITY) t.forced[i] += 1;
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
        node = child;
    }
    MctsSlot m = t.ms[i];
    m.path_len = depth;
    m.leaf_edge = leaf;
    m.leaf_pending = 0;
    m.leaf_n = 0;
    m.leaf_value = 0.f;
    const int8_t code = bd[lane];
    if (__ballot(code != 0 && code != 1 && code != 7) == 0ull) {
        // GameState.isDraw after the move ends the game (self_play.py:180)
        m.leaf_value = 0.f;
    } else {
        Pos p = wave_pos(code, s_meta[0], s_meta[1], s_meta[2], s_meta[3], s_meta[4], s_meta[5], s_meta[6]);
        const int n = wave_valid_moves(p, t.leaf_moves + (size_t)i * MAXM, MAXM, lane);
        if (n > MAXM && lane == 0) atomicOr(&ctr->error, 1);
        m.leaf_wtm = p.wtm;
        if (n == 0) {
            m.leaf_value = in_check(p) ? (p.wtm ? -1.f : 1.f) : 0.f;  // mate / stalemate
        } else {
            bd[lane] = (int8_t)pos_at(p, lane);  // the board the reference would encode (after getValidMoves)
            m.leaf_pending = 1;
            m.leaf_n = n < MAXM ? n : MAXM;
            m.pad[1] += 1;
        }
    }
    if (lane == 0) {
        t.ms[i] = m;
        t.leaf_cnt[i] = m.leaf_pending ? m.leaf_n : 0;  // the logits the network computes for this slot
    }
    __syncthreads();
    nn_boards[(size_t)i * 64 + lane] = bd[lane];
}

// one slot's backup, by the 64 threads of its workgroup (REUSE: a no-op for a slot that was not live in the
// step's select -- its root count has not changed since)
template <bool REUSE>
__device__ inline void mcts_backup_slot(const DevCfg& cfg, const Tree& t, const Slot* slots, const float* logits,
                                        const float* values, float* probs, Ctr* ctr, int i) {
    __shared__ float pri[MAXM];
    const int lane = threadIdx.x;
    const Slot s = slots[i];
    if (s.status != ST_ACTIVE) return;
    if (REUSE && t.node[(size_t)i * t.ncap].N - 1 >= (t.tgt ? t.tgt[i] : t.sims)) return;
    MctsSlot m = t.ms[i];
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    float v = m.leaf_value;
    if (m.leaf_pending) {
        v = values[i];
        // priors = softmax over the legal moves' logits only, which the network
        // wrote compactly in list order (kv_net_forward_boards_legal):
        // max, e_j = det_expf(l_j - max) kept in LDS, lane partial sums over
        // j = lane, lane+64, ... in order, xor butterfly
        const float* lg = t.leaf_logits + (size_t)i * MAXM;
        const uint16_t* lm = t.leaf_moves + (size_t)i * MAXM;
        const int n = m.leaf_n;
        float mx = -INFINITY;
        for (int j = lane; j < n; j += 64) {
            const float l = lg[j];
            pri[j] = l;
            mx = fmaxf(mx, l);
        }
        mx = wave_max(mx);
        float part = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float e = det_expf(pri[j] - mx);
            pri[j] = e;
            part += e;
        }
        const float sum = wave_sum(part);
        // a node's edges start on a 16-edge boundary, so the descent's P / W
        // (and N / child / move) reads of one node touch the fewest HBM lines
        const int first = (m.edge_count + 15) & ~15;
        const bool fits = first + n <= t.ecap && m.node_count < t.ncap;
        if (fits) {
            for (int j = lane; j < n; j += 64) {
                const size_t e = eb + first + j;
                t.e_move[e] = lm[j];
                t.e_P[e] = sum > 0.f ? pri[j] / sum : 1.0f / (float)n;  // sum >= 1 for finite logits
                t.e_N[e] = 0;
                t.e_W[e] = 0.f;
                t.e_child[e] = NO_CHILD;
            }
        }
        if (lane == 0) {
            if (fits) {
                const int id = m.node_count;
                t.node[nb + id] = NodeRec{first, n, 0, 0};
                t.e_child[eb + m.leaf_edge] = (uint16_t)id;
                m.node_count += 1;
                m.edge_count = first + n;
            } else {
                // the expansion does not fit the slot's pools: counted and
                // raised as an error (kv_run -> KV_EOVERFLOW), never silent
                m.overflow += 1;
                atomicAdd(&ctr->tree_overflows, 1ull);
                atomicOr(&ctr->error, 4);
            }
            m.pad[0] += 1;
        }
    }
    if (lane == 0) {
        // backup along the path: the mover at depth d is the root side flipped d times
        // (a non-root node's visit count is its parent edge's N: only the
        // root's record is updated)
        const int* path = t.path + nb;
        t.node[nb].N += 1;
        for (int d = 0; d < m.path_len; ++d) {
            const size_t e = eb + path[d];
            const bool white_moved = ((m.root_wtm != 0) ^ (d & 1)) != 0;
            t.e_N[e] += 1;
            t.e_W[e] = t.e_W[e] + (white_moved ? v : -v);
        }
        t.ms[i] = m;
    }
}

template <bool REUSE, bool FORCED>
__global__ __launch_bounds__(64) void k_mcts_select(DevCfg cfg, Tree t, const Slot* slots, const int8_t* boards,
                                                    int8_t* nn_boards, Ctr* ctr, int slot0, const int* list) {
    mcts_select_slot<REUSE, FORCED>(cfg, t, slots, boards, nn_boards, ctr,
                                    list ? list[blockIdx.x] : slot0 + blockIdx.x);
}

template <bool REUSE>
__global__ __launch_bounds__(64) void k_mcts_backup(DevCfg cfg, Tree t, const Slot* slots, const float* logits,
                                                    const float* values, float* probs, Ctr* ctr, int slot0,
                                                    const int* list) {
    mcts_backup_slot<REUSE>(cfg, t, slots, logits, values, probs, ctr, list ? list[blockIdx.x] : slot0 + blockIdx.x);
}

// backup of sim-step k and select of sim-step k+1 for the same slot in one
// launch (a slot's next descent depends only on its own tree): one kernel
// boundary less per sim-step. The barrier orders thread 0's tree writes
// before the descent reads them (workgroup scope).
template <bool REUSE, bool FORCED>
__global__ __launch_bounds__(64) void k_mcts_backup_select(DevCfg cfg, Tree t, const Slot* slots,
                                                           const int8_t* boards, const float* logits,
                                                           const float* values, float* probs, int8_t* nn_boards,
                                                           Ctr* ctr, int slot0, const int* list) {
    const int i = list ? list[blockIdx.x] : slot0 + blockIdx.x;  // (uniform over the workgroup)
    mcts_backup_slot<REUSE>(cfg, t, slots, logits, values, probs, ctr, i);
    __syncthreads();
    mcts_select_slot<REUSE, FORCED>(cfg, t, slots, boards, nn_boards, ctr, i);
}

// kv_config.forced_k, policy target pruning (DESIGN.md "Forced playouts and policy target pruning"): the pruned
// count T of root edge j of a full ply, given the first maximum b of the raw counts and its PUCT score `best`.
// From N visits, at most f times (f the forced count: the smallest m for which m * m < (k * P) * S fails, capped
// at N) one visit is taken off while the edge, at its fixed q = W / N and one visit fewer, still scores below
// `best`; what is left of a pruned edge at 1 goes to 0. puct()'s operation order, fp32, no contraction.
__device__ inline int pruned_count(float k, float c_puct, float P, float sq, int N, float W, int S, float best) {
    if (N <= 0) return 0;
    const float thr = (k * P) * (float)S;
    int f = 0;
    while (f < N && (float)f * (float)f < thr) ++f;
    const float q = W / (float)N;
    int tv = N;
    for (int r = 0; r < f; ++r) {
        const float sc = q + c_puct * P * sq / (float)(1 + (tv - 1));
        if (!(sc < best)) break;
        tv -= 1;
    }
    if (tv < N && tv == 1) tv = 0;
    return tv;
}

// FORCED (kv_config.forced_k > 0): the move is chosen from the pruned counts T, which also go to Tree::root_targets;
// the false instance is the kernel without the feature
template <bool FORCED>
__global__ __launch_bounds__(64) void k_mcts_choose(DevCfg cfg, Tree t, Slot* slots, int8_t* boards,
                                                    uint32_t* py_mt, kv_record* rec, int8_t* last_board, Ctr* ctr) {
    __shared__ double vals[MAXM];
    __shared__ double cum[MAXM];
    __shared__ int s_pick;
    __shared__ uint16_t s_T[FORCED ? MAXM : 1];
    const int i = blockIdx.x, lane = threadIdx.x;
    Slot s = slots[i];
    if (s.status != ST_ACTIVE) return;
    const MctsSlot m = t.ms[i];
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    const int n = t.node[nb].cnt;
    int pruned = 0;
    if (FORCED) {
        const bool full = t.tgt == nullptr || t.tgt[i] == cfg.sims;  // a fast ply: T = N
        float top = -INFINITY;
        int b = 0x7fffffff, S = 0;
        for (int j = lane; j < n; j += 64) {
            const int N = t.e_N[eb + j];
            S += N;
            if ((float)N > top) {  // (counts are below 2^16: exact as floats)
                top = (float)N;
                b = j;
            }
        }
        wave_argmax_first(top, b);
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) S += __shfl_xor(S, w);
        const float sq = t.sqrt_tab[t.node[nb].N];
        const float best = n > 0 ? puct(t.c_puct, t.e_P[eb + b], sq, t.e_N[eb + b], t.e_W[eb + b]) : 0.f;
        for (int j = lane; j < n; j += 64) {
            const int N = t.e_N[eb + j];
            const int T = !full || j == b
                              ? N
                              : pruned_count(t.forced_k, t.c_puct, t.e_P[eb + j], sq, N, t.e_W[eb + j], S, best);
            s_T[j] = (uint16_t)T;
            vals[j] = (double)T;
            pruned += N - T;
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) pruned += __shfl_xor(pruned, w);
    } else {
        for (int j = lane; j < n; j += 64) vals[j] = (double)t.e_N[eb + j];
    }
    __syncthreads();
    if (lane == 0) {
        if (cfg.sample_plies != 0 && (cfg.sample_plies < 0 || s.ply >= cfg.sample_plies)) {
            // kv_config.sample_plies: the first maximum of the visit counts in list order, no draw
            int best = 0;
            for (int j = 1; j < n; ++j)
                if (vals[j] > vals[best]) best = j;
            s_pick = best;
        } else {
            s_pick = choose_weighted(vals, cum, n, py_mt + (size_t)i * MT_WORDS);
        }
    }
    __syncthreads();
    // the move's counters in one update per slot (one device-scope atomic per
    // slot and sim-step on a shared counter cost ~3.5 us per select / backup)
    if (lane == 0) {
        // reuse_tree: the ply's new backups; the visits its root carried in are counted beside them, at the
        // choice like sims, so that sims + sims_kept == plies x cfg.sims whenever kv_run returns
        const int kept = t.rem != nullptr ? m.pad[4] : 0;
        if (t.tgt != nullptr) {
            // fast_sims: the ply's own target; a carried root that already held it ran no step
            const int target = t.tgt[i];
            atomicAdd(&ctr->sims, (unsigned long long)(target > kept ? target - kept : 0));
            if (target != cfg.sims) atomicAdd(&ctr->plies_fast, 1ull);
        } else {
            atomicAdd(&ctr->sims, (unsigned long long)(cfg.sims - kept));
        }
        atomicAdd(&ctr->nn_rows, (unsigned long long)m.pad[1]);
        if (FORCED) {
            const int forced = t.forced[i];
            t.forced[i] = 0;
            if (forced) atomicAdd(&ctr->forced_descents, (unsigned long long)forced);
            if (pruned) atomicAdd(&ctr->visits_pruned, (unsigned long long)pruned);
        }
        if (t.rem != nullptr) {
            t.ms[i].pad[3] = s_pick;  // the played root edge, for k_mcts_carry
            if (m.pad[2] != 0) {
                atomicAdd(&ctr->sims_kept, (unsigned long long)kept);
                atomicAdd(&ctr->roots_carried, 1ull);
            }
        }
    }
    s.last_value = m.root_value;  // resign test on the root's network value (:185)
    s.n_evals += m.pad[0];
    const int fast_ply = t.tgt != nullptr && t.tgt[i] != cfg.sims ? 1 : 0;  // kv_record.pad bit 0
    const unsigned long long ridx =
        commit_move(cfg, s, i, t.e_move[eb + s_pick], boards, rec, last_board, ctr, lane, fast_ply);
    if (t.root_visits && (long long)ridx < cfg.record_cap) {
        uint16_t* rv = t.root_visits + (size_t)ridx * MAXM;
        for (int j = lane; j < MAXM; j += 64) rv[j] = j < n ? t.e_N[eb + j] : (uint16_t)0xffff;
        if (t.root_moves) {
            uint16_t* rm = t.root_moves + (size_t)ridx * MAXM;
            for (int j = lane; j < MAXM; j += 64) rm[j] = j < n ? t.e_move[eb + j] : (uint16_t)0xffff;
        }
        if (FORCED && t.root_targets) {
            uint16_t* rt = t.root_targets + (size_t)ridx * MAXM;
            for (int j = lane; j < MAXM; j += 64) rt[j] = j < n ? s_T[j] : (uint16_t)0xffff;
        }
    }
    if (lane == 0) slots[i] = s;
}

// kv_config.reuse_tree, once per ply after k_finish: a slot whose game goes on after the move at root edge k
// keeps the subtree of that edge's child as its tree (tree_pack_subtree, a session's re-root); without a
// child, or when the game ended, a recycled slot started a new game or the slot is idle, the tree is dropped
// and the next ply builds a fresh root. rem[i] = the sim-steps the slot's next ply runs (0: not active).
// One wavefront per slot.
__global__ __launch_bounds__(64) void k_mcts_carry(DevCfg cfg, Tree t, const Slot* slots, Ctr* ctr) {
    __shared__ uint32_t keep[KEEP_WORDS];
    __shared__ int below[KEEP_WORDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    const Slot s = slots[i];
    MctsSlot m = t.ms[i];
    const size_t eb = (size_t)i * t.ecap, nb = (size_t)i * t.ncap;
    const int k = m.pad[3];
    // the game goes on: still active after k_finish with a move committed (a recycled slot is at ply 0), the
    // move being the one k_mcts_choose picked this ply
    const bool goes_on = s.status == ST_ACTIVE && s.ply > 0 && k >= 0 && m.node_count >= 1 && k < t.node[nb].cnt;
    int c = NO_CHILD, played_n = 0;
    if (goes_on) {
        c = t.e_child[eb + k];
        played_n = t.e_N[eb + k];
    }
    bool carried = c != NO_CHILD;
    if (carried && (c <= 0 || c >= m.node_count || played_n < 1 || played_n > t.sims)) {
        if (lane == 0) atomicOr(&ctr->error, 32);  // not a tree this search built: dropped
        carried = false;
    }
    PackedTree pk = {0, 0, 0, 0.f};
    if (carried) {
        pk = tree_pack_subtree(t, eb, nb, c, m.node_count, played_n, keep, below);
        if (pk.moved != pk.nodes && lane == 0) atomicOr(&ctr->error, 32);
    }
    if (lane != 0) return;
    m.pad[2] = carried ? 1 : 0;
    m.pad[3] = -1;
    if (carried) {
        m.node_count = pk.nodes;
        m.edge_count = pk.edges;
        m.root_wtm = s.wtm;  // the side to move after the committed move: the old root's, flipped
    }
    t.ms[i] = m;
    int target = t.sims;  // fast_sims: the next ply's own (k_mcts_root writes the same value into Tree::tgt)
    if (t.tgt != nullptr) {
        bool fast;
        target = ply_target(cfg, s.game_id, s.ply, &fast);
    }
    const int kept = carried ? played_n - 1 : 0;
    t.rem[i] = s.status != ST_ACTIVE ? 0 : target > kept ? target - kept : 0;
}

// kv_config.fast_sims without reuse_tree, once per ply after k_finish in k_mcts_carry's place: rem[i] = the next
// ply's visit target (every root is fresh), 0 for a slot that is not active
__global__ __launch_bounds__(64) void k_mcts_targets(DevCfg cfg, Tree t, const Slot* slots) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= cfg.slots) return;
    const Slot s = slots[i];
    bool fast;
    t.rem[i] = s.status != ST_ACTIVE ? 0 : ply_target(cfg, s.game_id, s.ply, &fast);
}

// Test evaluator (KV_EVAL_HASH): all logits 0 (uniform priors, exact in
// float), value = dyadic hash of the 64 board codes. Lets the CPU restatement
// reproduce every PUCT score bit for bit.
__global__ void k_hash_eval(const int8_t* boards, int rows, float* logits, float* values, int negate) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= rows) return;
    for (int j = lane; j < 4096; j += 64) logits[(size_t)r * 4096 + j] = 0.f;
    if (lane == 0) {
        uint32_t h = 2166136261u;
        for (int q = 0; q < 64; ++q) {
            h ^= (uint8_t)boards[(size_t)r * 64 + q];
            h *= 16777619u;
        }
        const float v = (float)((int)(h % 129u) - 64) / 64.0f;
        values[r] = negate ? -v : v;  // (the arena's player B)
    }
}

// the hash evaluator's leaf logits (all 0) in kv_net_forward_boards_legal's layout
__global__ void k_hash_legal(int* cnt, float* out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    for (int j = lane; j < cnt[r]; j += 64) out[(size_t)r * MAXM + j] = 0.f;
}

int hash_legal(const Tree& t, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_hash_legal, dim3(rows), dim3(64), 0, st, t.leaf_cnt, t.leaf_logits);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_root(const DevCfg& cfg, const Tree& t, Slot* slots, const uint16_t* moves, const float* logits,
              const float* values, float* probs, uint32_t* np_mt, Ctr* ctr, hipStream_t st) {
    if (t.tgt != nullptr)
        hipLaunchKernelGGL(k_mcts_root_pcr, dim3(cfg.slots), dim3(256), 0, st, cfg, t, slots, moves, logits, values,
                           probs, np_mt, ctr);
    else
        hipLaunchKernelGGL(k_mcts_root, dim3(cfg.slots), dim3(256), 0, st, cfg, t, slots, moves, logits, values,
                           probs, np_mt, ctr);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_select(const DevCfg& cfg, const Tree& t, const Slot* slots, const int8_t* boards, int8_t* nn_boards,
                Ctr* ctr, hipStream_t st, int slot0, int count, bool reuse, const int* list) {
    // (kv_config.forced_k > 0: the FORCED instances; 0 launches the kernels without the feature)
    const auto k = t.forced_k > 0.f ? (reuse ? k_mcts_select<true, true> : k_mcts_select<false, true>)
                                    : (reuse ? k_mcts_select<true, false> : k_mcts_select<false, false>);
    hipLaunchKernelGGL(k, dim3(count), dim3(64), 0, st, cfg, t, slots, boards, nn_boards, ctr, slot0, list);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_backup(const DevCfg& cfg, const Tree& t, const Slot* slots, const float* logits, const float* values,
                float* probs, Ctr* ctr, hipStream_t st, int slot0, int count, bool reuse, const int* list) {
    if (reuse)
        hipLaunchKernelGGL(k_mcts_backup<true>, dim3(count), dim3(64), 0, st, cfg, t, slots, logits, values, probs,
                           ctr, slot0, list);
    else
        hipLaunchKernelGGL(k_mcts_backup<false>, dim3(count), dim3(64), 0, st, cfg, t, slots, logits, values, probs,
                           ctr, slot0, list);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_backup_select(const DevCfg& cfg, const Tree& t, const Slot* slots, const int8_t* boards, const float* logits,
                       const float* values, float* probs, int8_t* nn_boards, Ctr* ctr, hipStream_t st, int slot0,
                       int count, bool reuse, const int* list) {
    const auto k = t.forced_k > 0.f ? (reuse ? k_mcts_backup_select<true, true> : k_mcts_backup_select<false, true>)
                                    : (reuse ? k_mcts_backup_select<true, false> : k_mcts_backup_select<false, false>);
    hipLaunchKernelGGL(k, dim3(count), dim3(64), 0, st, cfg, t, slots, boards, logits, values, probs, nn_boards, ctr,
                       slot0, list);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_choose(const DevCfg& cfg, const Tree& t, Slot* slots, int8_t* boards, uint32_t* py_mt, kv_record* rec,
                int8_t* last_board, Ctr* ctr, hipStream_t st) {
    hipLaunchKernelGGL(t.forced_k > 0.f ? k_mcts_choose<true> : k_mcts_choose<false>, dim3(cfg.slots), dim3(64), 0, st,
                       cfg, t, slots, boards, py_mt, rec, last_board, ctr);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_carry(const DevCfg& cfg, const Tree& t, const Slot* slots, Ctr* ctr, hipStream_t st) {
    hipLaunchKernelGGL(k_mcts_carry, dim3(cfg.slots), dim3(64), 0, st, cfg, t, slots, ctr);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int mcts_targets(const DevCfg& cfg, const Tree& t, const Slot* slots, hipStream_t st) {
    hipLaunchKernelGGL(k_mcts_targets, dim3((cfg.slots + 63) / 64), dim3(64), 0, st, cfg, t, slots);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int hash_eval(const int8_t* boards, int rows, float* logits, float* values, hipStream_t st, bool negate) {
    hipLaunchKernelGGL(k_hash_eval, dim3(rows), dim3(64), 0, st, boards, rows, logits, values, negate ? 1 : 0);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

}  // namespace kv
