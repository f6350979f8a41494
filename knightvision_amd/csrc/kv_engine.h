// Shared device state of the self-play engine (kv_engine.hip: reference
// move selection; kv_mcts.hip: PUCT search; kv_search.hip: the search of
// given positions, kv_search).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kv_common.h"
#include "kv_movegen.h"
#include "kv_rng.h"

#pragma clang fp contract(off)

namespace kv {

int net_forward_boards_internal(kv_net* net, const int8_t* boards_dev, int B, float* policy, float* value,
                                hipStream_t st);
int net_forward_boards_legal_internal(kv_net* net, const int8_t* boards_dev, int B, const uint16_t* moves,
                                      const int* n_moves, int maxm, float* legal, float* value, hipStream_t st);
int net_set_res_events(kv_net* net, hipEvent_t a, hipEvent_t b);
int net_view_create(kv_net* parent, kv_net** out);
void net_view_destroy(kv_net* v);
void net_set_cu_share(kv_net* net, int share);
void net_dom_info(const kv_net* net, int* algo, int* launches, double* flop, int* path, int* split,
                  const char** kernel);

enum : int { ST_IDLE = 0, ST_ACTIVE = 1, ST_FINISHED = 2 };
enum : int { END_NONE = 0, END_NOMOVES = 1, END_DRAW = 2, END_RESIGN = 3, END_MAXED = 4 };

struct Slot {
    long long game_id;
    int status;
    int ply;
    int wtm, wkr, wkc, bkr, bkc, flags, ep;
    int nmoves;
    int buf;
    int has_last;
    float last_value;
    int consumed;
    int need_flush;
    int n_evals;
    int end_kind;
    int outcome;
    int reason;
    int rows_total;   // network rows this slot has appended (all its games; k_count sums them)
    int plies_total;  // moves this slot has committed (all its games)
    int movegen_clean;  // k_movegen's getValidMoves left the position as it found it
    int pad[8];
};
static_assert(sizeof(Slot) == 128, "slot is one cache line");

struct Ctr {
    unsigned long long rec_count;
    unsigned long long games_count;
    unsigned long long next_game;
    unsigned long long plies;
    unsigned long long nn_rows;
    unsigned long long sims;
    unsigned long long nn_rows_slots;  // k_count: sum of Slot::rows_total (nn_rows adds the MCTS leaf rows)
    unsigned long long tree_overflows;  // MCTS expansions that did not fit the slot's pools (error flag 4)
    int active;
    int error;
    int need_eval;  // KV_EVAL_LAZY: some slot consumes a network row this step
    int comp_rows;  // KV_EVAL_LAZY above 16 slots: network rows of this step's compact batch
    unsigned long long sims_kept;      // reuse_tree: root visits the committed plies' roots carried in
    unsigned long long roots_carried;  // reuse_tree: committed plies whose root was a carried tree
    int arena_n[2];  // arena: this ply's active slots whose mover plays on net A / net B (k_arena_split)
    unsigned long long plies_fast;  // fast_sims: committed plies searched to the fast target (the rest are full)
    // forced_k: accepted descents at whose root an edge was forced, and the visits the committed plies' targets
    // lost to the pruning, sum of (S - sum T); both counted at the move choice
    unsigned long long forced_descents;
    unsigned long long visits_pruned;
};

struct DevCfg {
    int slots;
    long long n_games;
    long long id_base, id_stride;
    unsigned long long seed;
    int seed_mode;
    int max_moves;
    int batch;
    double eps, alpha;
    long long record_cap;
    int recycle;
    int rows;  // NN rows per step (slots, or 2*slots with flush rows)
    long long games_cap;  // game-record ring capacity
    int sims;             // 0: reference move selection; >0: PUCT search
    int eval_mode;        // KV_EVAL_*
    int sample_plies;     // MCTS move choice: 0 every ply drawn, k > 0 first maximum from ply k on, -1 on every ply
    // kv_dev_set_starts (test-only; nullptr: every game starts from the initial position): n_starts 80-byte
    // state vectors, the game with global id g starts from starts[g % n_starts]
    const int8_t* starts;
    int n_starts;
    int fast_sims;  // kv_config.fast_sims (0: off) and full_q16: a ply's kind and visit target (ply_target)
    int full_q16;
};

// kv_config.fast_sims (DESIGN.md "Playout cap randomization"): the visit target of ply `ply` of game `game_id`, a
// pure function of the value the game's two streams are seeded with and the ply -- sims on a full ply, fast_sims on
// a fast one (*fast set). A splitmix64 finaliser over the two; no draw from either MT19937 stream.
__device__ inline int ply_target(const DevCfg& cfg, long long game_id, int ply, bool* fast) {
    unsigned long long x = (cfg.seed + (unsigned long long)game_id) * 0x9E3779B97F4A7C15ull +
                           (unsigned long long)(ply + 1) * 0xD1B54A32D192ED03ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    const bool full = (int)(x >> 48) < cfg.full_q16;
    *fast = !full;
    return full ? cfg.sims : cfg.fast_sims;
}

__device__ inline Pos slot_pos(const Slot& s, const int8_t* board) {
    Pos p;
    pos_from_board(p, board, s.wtm, s.wkr, s.wkc, s.bkr, s.bkc, s.flags, s.ep);
    return p;
}

__device__ inline void slot_store_pos(Slot& s, int8_t* board, const Pos& p) {
    pos_to_board(p, board);
    s.wtm = p.wtm;
    s.wkr = p.wkr; s.wkc = p.wkc; s.bkr = p.bkr; s.bkc = p.bkc;
    s.flags = p.flags;
    s.ep = p.ep;
}


struct MctsSlot {  // per-slot search scratch (kv_mcts.hip)
    int node_count;
    int edge_count;
    int path_len;
    int leaf_edge;
    int leaf_pending;  // 1: the leaf row is in this step's network batch
    int leaf_n;
    int leaf_wtm;
    float leaf_value;  // terminal value (white perspective) when !leaf_pending
    float root_value;
    int root_wtm;
    int overflow;      // expansions skipped because the slot's edge / node pool was full (an error)
    // pad[0], pad[1]: network rows consumed / leaf rows sent this move (k_mcts_root). With reuse_tree
    // (Tree::rem): pad[2] 1: the tree is a carried one (k_mcts_carry), pad[3] the root edge k_mcts_choose
    // picked (-1 once k_mcts_carry has taken it), pad[4] the root visits this ply's root carried in
    int pad[5];
};

constexpr uint16_t NO_CHILD = 0xffff;  // e_child of an unexpanded edge

struct __attribute__((aligned(16))) NodeRec {
    int first, cnt, N;
    int value;  // kv_search.hip: bits of the network value the node got at its expansion (a session's re-root)
};

struct Tree {  // per-slot SoA edge pools + node records, slot i at i*ecap / i*ncap
    uint16_t* e_move;
    float* e_P;
    uint16_t* e_N;      // visit count (<= sims <= KV_MAX_SIMS)
    float* e_W;
    uint16_t* e_child;  // child node id (< ncap) or NO_CHILD
    NodeRec* node;    // [slot][ncap]: first edge, edge count, visit count (one 16-B load per tree level)
    int* path;        // [slot][ncap]
    uint16_t* leaf_moves;  // [slot][MAXM]
    int* leaf_cnt;         // [slot]: moves of the leaf in this step's network batch (0: none)
    float* leaf_logits;    // [slot][MAXM]: their policy logits (kv_net_forward_boards_legal)
    MctsSlot* ms;
    const float* sqrt_tab;  // (float)sqrt((double)n), n < ncap + 2
    uint16_t* root_visits;  // optional [record_cap][MAXM]: root visit counts (pi) of each committed move, 0xffff padded
    int ecap, ncap;
    float c_puct;
    int sims;
    uint16_t* e_V;  // position search with several leaves in flight (kv_search.hip): descents in flight per edge
    uint16_t* root_moves;  // optional [record_cap][MAXM]: the root's move words beside root_visits, 0xffff padded
    // reuse_tree or fast_sims (else NULL) [slot]: sim-steps the slot's next ply runs, its target - carried visits; 0:
    // idle, or a fast ply whose carried root already holds its target
    int* rem;
    int* tgt;  // fast_sims only (else NULL) [slot]: the visit target of the ply k_mcts_root built, sims or fast_sims
    // kv_config.forced_k (DESIGN.md "Forced playouts and policy target pruning"; 0: off, the three below unused)
    float forced_k;
    int* forced;             // [slot]: this ply's accepted descents whose root had a forced edge (k_mcts_choose zeroes it)
    uint16_t* root_targets;  // optional [record_cap][MAXM]: the pruned counts T beside root_visits, 0xffff padded
};

// kv_config.forced_k, the forced rule at the root: an edge with n > 0 visits (in-flight descents counting) is forced
// while n * n < (k * P) * S, S the root's visit sum as the descent sees it. fp32, no contraction, no sqrtf.
__device__ inline bool forced_edge(float k, float P, int n, int S) {
    return n > 0 && (float)n * (float)n < (k * P) * (float)S;
}

// ---- position search (kv_search.hip): per-tree state, per-(tree, j) descents of the running sim-step ----
enum : int { SR_SEARCHED = 0, SR_CHECKMATED = 1, SR_STALEMATE = 2, SR_DRAW = 3 };

struct SearchSlot {
    int status;     // SR_*
    int done;       // backups completed
    int vroot;      // descents in flight (nonzero only inside a sim-step)
    int accepted;   // descents of the running sim-step
    int steps;      // sim-steps run
    int leaf_rows;  // leaves sent to the network
    float term_value;  // SR_CHECKMATED / SR_STALEMATE / SR_DRAW: the root's value, white perspective
    int pad;
};

struct SearchLeaf {
    int path_len;
    int leaf_edge;
    int pending;  // 1: row tree * L + j of the step's network batch is this leaf
    int n;        // its legal moves
    float value;  // terminal value (white perspective) when !pending
    int pad[3];
};

struct LeafCtr {  // kv_config.leaves > 1: what k_leaves_compact tells the host once per sim-step
    int pend[2];    // pending leaf rows of the step (arena: of player A's / player B's slots; self-play: [0])
    int stepping;   // slots that took a descent in the step
    int remaining;  // of those, the slots whose root still holds fewer than sims backups after the step's
};

// kv_config.eval_cache (kv_cache.hip): one network's table -- entries of KV_CACHE_ENTRY_BYTES, a claim word per
// entry (CACHE_NO_CLAIM between sim-steps), mask = entries - 1 -- and the counters of kv_stats
struct CacheTab {
    uint4* ent;
    int* claim;
    unsigned mask;
};
struct CacheCtr {
    unsigned long long probes, hits, stores;
};
constexpr int CACHE_NO_CLAIM = 0x7f7f7f7f;  // (a byte pattern: hipMemset writes it)

struct SessionSlot {  // per-tree state of a search session (kv_search_advance / kv_search_continue)
    int status;    // SR_* of the current root
    int n_moves;   // its move count
    int kept;      // visits the root held when the last advance / continue began counting (0: dropped or fresh)
    int fresh;     // 1: the tree was dropped, the next continue builds the root from its network row
    int root_row;  // 1: the running continue took a root row for this tree
    int pad[3];
};

struct SearchWs {  // workspaces of kv_search, rows = positions x leaves; reserved at the first search, only grown
    SearchSlot* ss;       // [slots]
    SearchLeaf* lf;       // [rows]
    int* paths;           // [rows][ncap]
    int8_t* lboards;      // [rows][64]
    uint16_t* lmoves;     // [rows][MAXM]
    int* lcnt;            // [rows]
    float* llogits;       // [rows][MAXM]
    float* lvalues;       // [rows]
    int* remaining;       // trees with done < sims after the last backup
    kv_search_result* res;  // [slots]
    SessionSlot* sess;    // [slots]
};

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the wave's maximum and, among equal maxima, the smallest index (kv_mcts.hip, kv_search.hip)
__device__ inline void wave_argmax_first(float& best, int& idx) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m);
        const int oi = __shfl_xor(idx, m);
        if (ob > best || (ob == best && oi < idx)) {
            best = ob;
            idx = oi;
        }
    }
}

// PUCT score; identical op order in kvo_mcts (oracle), no contraction
__device__ inline float puct(float c_puct, float P, float sq, int N, float W) {
    const float u = c_puct * P * sq / (float)(1 + N);
    const float q = N > 0 ? W / (float)N : 0.0f;
    return q + u;
}

// torch.softmax over 4096 fp32 logits (self_play.py:150): max, exp(x-max),
// sum, x * (1/sum)
__device__ void wave_softmax_4096(const float* lg, float* out, int lane) {
    float v[64];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        v[j] = lg[j * 64 + lane];
        m = fmaxf(m, v[j]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        v[j] = expf(v[j] - m);
        s += v[j];
    }
    s = wave_sum(s);
    const float inv = 1.0f / s;
#pragma unroll
    for (int j = 0; j < 64; ++j) out[j * 64 + lane] = v[j] * inv;
}

// exp(x) for the MCTS priors (build-defined; no reference counterpart),
// made of IEEE double basic operations only -- Cody-Waite reduction by ln 2,
// degree-11 Taylor polynomial, exact power-of-two scaling, one rounding to
// float -- so that oracle/kv_oracle.c det_expf reproduces it bit for bit
// (ocml's expf and glibc's expf differ in the last bit). Results below
// e^-87 (float subnormals) are 0.
__device__ inline float det_expf(float x) {
    if (!(x >= -87.0f)) return 0.0f;
    const double xd = (double)x;
    const double kd = rint(xd * 1.4426950408889634);
    const double r = (xd - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    double p = 2.5052108385441720e-08;  // 1/11!
    p = p * r + 2.7557319223985893e-07;
    p = p * r + 2.7557319223985888e-06;
    p = p * r + 2.4801587301587302e-05;
    p = p * r + 1.9841269841269841e-04;
    p = p * r + 1.3888888888888889e-03;
    p = p * r + 8.3333333333333332e-03;
    p = p * r + 4.1666666666666664e-02;
    p = p * r + 1.6666666666666666e-01;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double scale = __longlong_as_double((long long)((int)kd + 1023) << 52);
    return (float)(p * scale);
}

// softmax over 4096 logits with det_expf (MCTS root): max, e = det_expf(x -
// max), each lane sums its 64 entries j*64+lane in j order, xor-butterfly
// over the wave (offsets 32..1), x * (1/sum)
__device__ void wave_softmax_4096_det(const float* lg, float* out, int lane) {
    float v[64];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        v[j] = lg[j * 64 + lane];
        m = fmaxf(m, v[j]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        v[j] = det_expf(v[j] - m);
        s += v[j];
    }
    s = wave_sum(s);
    const float inv = 1.0f / s;
#pragma unroll
    for (int j = 0; j < 64; ++j) out[j * 64 + lane] = v[j] * inv;
}

// mixed legal weights of the reference (self_play.py:147-160) for a slot's
// move list: (1-eps)*softmax [fp32] + eps*dirichlet [fp64], in list order.
// Consumes the slot's numpy stream exactly as np.random.dirichlet does. All
// 256 threads of the slot's workgroup; gam is 4096 doubles of LDS.
__device__ inline void mixed_legal_weights(const DevCfg& cfg, const float* lp, const uint16_t* ml, int n,
                                           double* gam, uint32_t* np_state, uint32_t* mt_ring, int* scratch,
                                           double* vals, int tid, double eps) {
    BlockMT w;
    bmt_load(w, np_state, mt_ring, tid);
    long long att;
    const double acc = block_dirichlet_gamma(w, cfg.alpha, 4096, gam, &att, scratch, tid);
    bmt_store(w, np_state, tid);
    const double invacc = 1 / acc;
    const float keep = (float)(1.0 - eps);
    for (int j = tid; j < n; j += RNG_THREADS) {
        const int mv = ml[j];
        const int idx = (mv & 63) * 64 + ((mv >> 6) & 63);
        const float p32 = keep * lp[idx];
        const double noise = gam[idx] * invacc;
        vals[j] = (double)p32 + eps * noise;
    }
    __syncthreads();
}

// random.choices(population, weights) / random.choice when the total is 0
// (self_play.py:162-167, CPython random.py:506-541). Lane 0 only.
// the pick of random.choices for a non-zero total with r = random() already
// drawn (cum_weights by serial accumulation, bisect_right on r * total)
__device__ inline int choose_from(const double* vals, double* cum, int n, double total, double r) {
    double c = 0.0;
    for (int j = 0; j < n; ++j) {
        c = c + vals[j] / total;
        cum[j] = c;
    }
    const double tot = cum[n - 1] + 0.0;
    const double x = r * tot;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x < cum[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ inline int choose_weighted(const double* vals, double* cum, int n, uint32_t* py) {
    double total = 0.0;
    for (int j = 0; j < n; ++j) total = total + vals[j];
    if (total == 0.0) return mt_randbelow_serial(py, n);
    return choose_from(vals, cum, n, total, mt_random_serial(py));
}

// record the position + move, makeMove, then the reference's termination
// checks in order: isDraw (:180), resign (:185, `value` is the row the move
// was chosen with), max_moves (:196). All lanes of the slot's wave.
__device__ inline unsigned long long commit_move(const DevCfg& cfg, Slot& s, int i, int mv, int8_t* boards,
                                                 kv_record* rec, int8_t* last_board, Ctr* ctr, int lane,
                                                 int flags = 0) {
    // lane = thread index of the slot's workgroup; lanes 0..63 (wave 0) carry
    // the 64 squares, every thread reaches the barriers
    int8_t* board = boards + (size_t)i * 64;
    const bool sqlane = lane < 64;
    const unsigned long long r = lane == 0 ? atomicAdd(&ctr->rec_count, 1ull) : 0ull;
    const unsigned long long ridx = __shfl(r, 0);
    const int8_t sq = sqlane ? board[lane] : 0;
    if (sqlane) last_board[(size_t)i * 64 + lane] = sq;
    if ((long long)ridx < cfg.record_cap) {
        if (sqlane) rec[ridx].board[lane] = sq;
        if (lane == 0) {
            rec[ridx].game_id = s.game_id;
            rec[ridx].ply = s.ply;
            rec[ridx].move = (uint16_t)((mv & 63) * 64 + ((mv >> 6) & 63));
            rec[ridx].pad = (uint16_t)flags;  // bit 0: a fast ply (kv_config.fast_sims)
        }
    } else if (lane == 0) {
        atomicOr(&ctr->error, 2);
    }
    __syncthreads();
    if (lane == 0) {
        make_move_board(board, s.wtm, s.wkr, s.wkc, s.bkr, s.bkc, s.flags, s.ep, mv);
        s.ply += 1;
        s.plies_total += 1;
    }
    __syncthreads();
    const int8_t b2 = sqlane ? board[lane] : 0;
    const bool non_king = b2 != 0 && b2 != 1 && b2 != 7;
    const bool draw = __ballot(non_king) == 0ull;
    if (lane == 0) {
        if (draw) {
            s.end_kind = END_DRAW;
        } else if (s.ply > 15 && (double)s.last_value < -0.7) {
            s.end_kind = END_RESIGN;
            s.outcome = s.wtm ? -1 : 1;
            s.reason = 1;
        } else if (cfg.max_moves > 0 && s.ply >= cfg.max_moves) {
            s.end_kind = END_MAXED;
        }
        if (s.end_kind != END_NONE) s.status = ST_FINISHED;
        s.consumed = 0;
    }
    return ridx;  // the record's index
}

// MCTS launches (kv_mcts.hip), all on `st`
int mcts_root(const DevCfg& cfg, const Tree& t, Slot* slots, const uint16_t* moves, const float* logits,
              const float* values, float* probs_scratch, uint32_t* np_mt, Ctr* ctr, hipStream_t st);
// select / backup for slots [slot0, slot0 + count); reuse: the kernels of kv_config.reuse_tree, in which a
// slot whose root holds sims visits takes no descent and no backup. list (a device array of `count` slot
// indices, the arena's per-net lists) != nullptr: the slots list[0 .. count) instead of the contiguous range
int mcts_select(const DevCfg& cfg, const Tree& t, const Slot* slots, const int8_t* boards, int8_t* nn_boards,
                Ctr* ctr, hipStream_t st, int slot0, int count, bool reuse = false, const int* list = nullptr);
int mcts_backup(const DevCfg& cfg, const Tree& t, const Slot* slots, const float* logits, const float* values,
                float* probs, Ctr* ctr, hipStream_t st, int slot0, int count, bool reuse = false,
                const int* list = nullptr);
// backup of one sim-step fused with the next sim-step's select
int mcts_backup_select(const DevCfg& cfg, const Tree& t, const Slot* slots, const int8_t* boards, const float* logits,
                       const float* values, float* probs, int8_t* nn_boards, Ctr* ctr, hipStream_t st, int slot0,
                       int count, bool reuse = false, const int* list = nullptr);
// reuse_tree: after k_finish, every slot's tree carried (re-rooted on the played edge's child) or dropped
int mcts_carry(const DevCfg& cfg, const Tree& t, const Slot* slots, Ctr* ctr, hipStream_t st);
// fast_sims without reuse_tree: after k_finish, every slot's rem = its next ply's visit target
int mcts_targets(const DevCfg& cfg, const Tree& t, const Slot* slots, hipStream_t st);
int mcts_choose(const DevCfg& cfg, const Tree& t, Slot* slots, int8_t* boards, uint32_t* py_mt, kv_record* rec,
                int8_t* last_board, Ctr* ctr, hipStream_t st);
// negate: the arena's player B under KV_EVAL_HASH (the same rows with the value negated)
int hash_eval(const int8_t* boards, int rows, float* logits, float* values, hipStream_t st, bool negate = false);
int hash_legal(const Tree& t, int rows, hipStream_t st);

// position search launches (kv_search.hip), all on `st`; n trees, L leaves in flight per tree
int search_load(const Tree& t, const SearchWs& w, Slot* slots, int8_t* boards, uint16_t* moves, int8_t* root_rows,
                uint32_t* np_mt, const int8_t* states, unsigned long long seed, int n, int L, Ctr* ctr,
                hipStream_t st);
int search_select(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr, int sims,
                  int n, int L, hipStream_t st);
int search_backup_select(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr,
                         int sims, int n, int L, hipStream_t st);
// session: nn_rows and the counters take this call's rows and backups only (kv_search_continue)
int search_result(const Tree& t, const SearchWs& w, const Slot* slots, Ctr* ctr, int sims, int n, bool session,
                  hipStream_t st);
// self-play / arena with kv_config.leaves > 1: the sim-step of the position search on the slots' own trees (n slots,
// L descents per slot). leaves_backup with select: fused with the next step's select
int leaves_select(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr, int sims,
                  int n, int L, hipStream_t st);
int leaves_backup(const Tree& t, const SearchWs& w, const Slot* slots, const int8_t* boards, Ctr* ctr, int sims,
                  int n, int L, bool select, hipStream_t st);
// kv_config.eval_cache (kv_cache.hip), all on `st`: an empty table; the probe of a sim-step's rows (slots != nullptr:
// the arena's two tables, row r of slot r / L; a row of fewer than nmin moves is not pending) -> hit[rows], the hits'
// payload in w.llogits / w.lvalues, the misses' entries in cidx[rows] and claimed; the store of the missed rows from w
int cache_clear(const CacheTab& t, hipStream_t st);
int cache_reset_claims(const CacheTab& t, hipStream_t st);  // every claim word back to CACHE_NO_CLAIM, the entries kept
int cache_probe(const CacheTab& ta, const CacheTab& tb, const Slot* slots, int L, int nmin, const SearchWs& w, int rows,
                int* hit, int* cidx, CacheCtr* cc, hipStream_t st);
int cache_store(const CacheTab& ta, const CacheTab& tb, const Slot* slots, int L, int nmin, const SearchWs& w, int rows,
                const int* hit, const int* cidx, CacheCtr* cc, hipStream_t st);
// search sessions: play root edge edge[i] in tree i (-1: none), then the per-call reset of a continue
int search_advance(const Tree& t, const SearchWs& w, Slot* slots, int8_t* boards, uint16_t* moves, int8_t* root_rows,
                   const int* edge, int8_t* states, int n, Ctr* ctr, hipStream_t st);
int search_resume(const Tree& t, const SearchWs& w, Slot* slots, uint32_t* np_mt, unsigned long long seed, int n,
                  int L, hipStream_t st);

}  // namespace kv
