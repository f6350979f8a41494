// Self-play engine on MI355X: replaces scripts/self_play.py _run_single_game
// :111-255 / self_play :258-291 for `slots` concurrent games per GPU.
//
// One ply-step of every live game slot is four launches on one stream:
//   k_movegen  one wave per slot, lane = square: reference-exact legal list
//              (kv_movegen.h wave_valid_moves), game-over detection, SELFPLAY_BATCH_SIZE schedule bookkeeping
//   NN         ChessNet over the slots' boards (kv_nn.hip) -- every board is
//              evaluated once, as the reference does (faithful), or only the
//              rows the schedule consumes (lazy)
//   k_sample   one wave per slot: softmax of the consumed row, numpy-legacy
//              Dirichlet noise on the slot's own MT19937 (wave-parallel),
//              0.75/0.25 mix in the reference's fp32/fp64 order, CPython
//              random.choices on the slot's second stream, makeMove, record,
//              termination (draw / resign / max_moves)
//   k_finish   one wave per finished slot: outcome + reward exactly as :210-250, game
//              record, then the slot starts the next game id (recycling)
// The host only launches and, every few steps, reads one counter.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "kv_common.h"
#include "kv_movegen.h"
#include "kv_rng.h"
#include "kv_engine.h"

#pragma clang fp contract(off)

namespace kv {

__constant__ const int8_t kStart[64] = {9, 11, 10, 8, 7, 10, 11, 9, 12, 12, 12, 12, 12, 12, 12, 12,
                                        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        6, 6, 6, 6, 6, 6, 6, 6, 3, 5, 4, 2, 1, 4, 5, 3};

// kv_dev_set_starts: the state vector game gid starts from, nullptr for the initial position
__device__ inline const int8_t* start_vec(const DevCfg& cfg, long long gid) {
    if (!cfg.starts) return nullptr;
    const long long r = gid % cfg.n_starts;
    return cfg.starts + (size_t)(r < 0 ? r + cfg.n_starts : r) * 80;
}

// the position fields of a slot from a state vector (as k_search_load reads one)
__device__ inline void start_pos_fields(Slot& s, const int8_t* v) {
    s.wtm = v[64];
    s.wkr = v[65]; s.wkc = v[66]; s.bkr = v[67]; s.bkc = v[68];
    s.flags = (v[69] ? F_WKM : 0) | (v[70] ? F_BKM : 0) | (v[71] ? F_WRK : 0) | (v[72] ? F_WRQ : 0) |
              (v[73] ? F_BRK : 0) | (v[74] ? F_BRQ : 0);
    s.ep = v[75] < 0 ? -1 : v[75] * 8 + v[76];
}

// GameState() :34-84: the slot fields of a new game (board and streams set by the caller)
__device__ void start_game_fields(const DevCfg& cfg, Slot& s, long long gid) {
    s.game_id = gid;
    s.status = ST_ACTIVE;
    s.ply = 0;
    s.wtm = 1; s.wkr = 7; s.wkc = 4; s.bkr = 0; s.bkc = 4; s.flags = 0; s.ep = -1;
    if (const int8_t* v = start_vec(cfg, gid)) start_pos_fields(s, v);
    s.nmoves = 0;
    s.buf = 0;
    s.consumed = 0;
    s.n_evals = 0;
    s.end_kind = END_NONE;
    s.outcome = 0;
    s.reason = -1;
    if (cfg.seed_mode == KV_SEED_PER_GAME) {
        s.has_last = 0;
        s.need_flush = 0;
    }
}

// GameState() + per-game seeding (_init_worker :81-85 with SEED+g), one thread
__device__ void start_game(const DevCfg& cfg, Slot& s, int8_t* board, uint32_t* np_mt, uint32_t* py_mt,
                           long long k) {
    const long long gid = cfg.id_base + k * cfg.id_stride;
    const int8_t* v = start_vec(cfg, gid);
    for (int i = 0; i < 64; ++i) board[i] = v ? v[i] : kStart[i];
    start_game_fields(cfg, s, gid);
    if (cfg.seed_mode == KV_SEED_PER_GAME) {
        const unsigned long long sd = cfg.seed + (unsigned long long)gid;
        mt_seed_genrand(np_mt, (uint32_t)sd);
        mt_seed_python(py_mt, sd);
    }
}

__global__ void k_init(DevCfg cfg, Slot* slots, int8_t* boards, uint32_t* np_mt, uint32_t* py_mt, Ctr* ctr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cfg.slots) return;
    Slot s;
    memset(&s, 0, sizeof(s));
    s.status = ST_IDLE;
    s.has_last = 0;
    s.need_flush = 0;
    if (cfg.seed_mode == KV_SEED_SEQUENTIAL) {  // one pair of streams seeded SEED (self_play.py:270)
        mt_seed_genrand(np_mt + (size_t)i * MT_WORDS, (uint32_t)cfg.seed);
        mt_seed_python(py_mt + (size_t)i * MT_WORDS, cfg.seed);
    }
    if ((long long)i < cfg.n_games) {
        start_game(cfg, s, boards + (size_t)i * 64, np_mt + (size_t)i * MT_WORDS, py_mt + (size_t)i * MT_WORDS, i);
        atomicAdd(&ctr->active, 1);
    }
    slots[i] = s;
}

// kv_dev_set_starts on a fresh engine: the games k_init started take their start positions (or the initial
// one again); everything else of the slot is as k_init left it
__global__ void k_set_starts(DevCfg cfg, Slot* slots, int8_t* boards) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cfg.slots || (long long)i >= cfg.n_games) return;
    Slot s = slots[i];
    const int8_t* v = start_vec(cfg, s.game_id);
    for (int q = 0; q < 64; ++q) boards[(size_t)i * 64 + q] = v ? v[q] : kStart[q];
    s.wtm = 1; s.wkr = 7; s.wkc = 4; s.bkr = 0; s.bkc = 4; s.flags = 0; s.ep = -1;
    if (v) start_pos_fields(s, v);
    slots[i] = s;
}

// ------------------------------------------------------------- counts ----
// the per-ply counters from the slots themselves, one workgroup: active slots,
// and the running sums of the slots' committed plies and appended network rows
// (per-slot fields instead of one device-scope atomic per slot and kernel on a
// shared counter, which serialised across the XCDs at ~0.1 us each)
__global__ __launch_bounds__(256) void k_count(DevCfg cfg, const Slot* slots, Ctr* ctr) {
    __shared__ unsigned long long red[3][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long a = 0, rows = 0, pl = 0;
    for (int j = tid; j < cfg.slots; j += 256) {
        a += slots[j].status == ST_ACTIVE;
        rows += (unsigned long long)slots[j].rows_total;
        pl += (unsigned long long)slots[j].plies_total;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m);
        rows += __shfl_xor(rows, m);
        pl += __shfl_xor(pl, m);
    }
    if (lane == 0) {
        red[0][wave] = a;
        red[1][wave] = rows;
        red[2][wave] = pl;
    }
    __syncthreads();
    if (tid == 0) {
        ctr->active = (int)(red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        ctr->nn_rows_slots = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        ctr->plies = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    }
}

// ------------------------------------------------------------ movegen ----
__global__ __launch_bounds__(64) void k_movegen(DevCfg cfg, Slot* slots, int8_t* boards, uint16_t* moves,
                                                Ctr* ctr) {
    const int i = blockIdx.x, lane = threadIdx.x;
    Slot s = slots[i];
    if (s.status != ST_ACTIVE) return;
    int8_t* board = boards + (size_t)i * 64;
    const int8_t before = board[lane];
    Pos p = wave_pos(before, s.wtm, s.wkr, s.wkc, s.bkr, s.bkc, s.flags, s.ep);
    const int n = wave_valid_moves(p, moves + (size_t)i * MAXM, MAXM, lane);
    const int8_t after = (int8_t)pos_at(p, lane);
    board[lane] = after;  // the reference may mutate the board (stale king, double check)
    const bool board_same = __ballot(after != before) == 0ull;
    if (lane != 0) return;
    if (n > MAXM) atomicOr(&ctr->error, 1);
    s.movegen_clean = board_same && p.wtm == s.wtm && p.wkr == s.wkr && p.wkc == s.wkc && p.bkr == s.bkr &&
                      p.bkc == s.bkc && p.flags == s.flags && p.ep == s.ep;
    s.wtm = p.wtm;
    s.wkr = p.wkr; s.wkc = p.wkc; s.bkr = p.bkr; s.bkc = p.bkc;
    s.flags = p.flags;
    s.ep = p.ep;
    s.nmoves = n < MAXM ? n : MAXM;
    if (n == 0) {
        s.end_kind = END_NOMOVES;
        s.status = ST_FINISHED;
        s.consumed = 0;
    } else {
        // buffer.append(board); eval when len >= BATCH_SIZE or nothing evaluated yet (:129-145)
        s.buf += 1;
        const bool has = s.has_last || s.need_flush;
        s.consumed = (s.buf >= cfg.batch) || !has;
        s.rows_total += 1;
    }
    if (s.consumed || s.need_flush) ctr->need_eval = 1;  // read by the host in KV_EVAL_LAZY
    slots[i] = s;
}

// ------------------------------------------------------------- sample ----
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_sample(DevCfg cfg, Slot* slots, int8_t* boards, const uint16_t* moves,
                                                const float* logits, const float* values, float* last_probs,
                                                uint32_t* np_mt, uint32_t* py_mt, kv_record* rec, int8_t* last_board,
                                                Ctr* ctr, const int* row_of) {
    __shared__ uint32_t mt3[MT_RW];
    __shared__ double gam[4096];
    __shared__ double vals[MAXM];
    __shared__ double cum[MAXM];
    __shared__ int scratch[RNG_SCRATCH];
    __shared__ int s_pick;
    const int i = blockIdx.x, lane = threadIdx.x;
    Slot s = slots[i];
    if (s.status != ST_ACTIVE) return;
    float* lp = last_probs + (size_t)i * 4096;
    if (s.need_flush) {  // previous game's final flush row (sequential mode)
        if (lane < 64) wave_softmax_4096(logits + (size_t)(cfg.slots + i) * 4096, lp, lane);
        s.last_value = values[cfg.slots + i];
        s.has_last = 1;
        s.need_flush = 0;
    }
    if (s.consumed) {  // policy/value = _last_outputs[...][-1] (:147-150)
        __syncthreads();
        const int row = row_of ? row_of[i] : i;  // the compact lazy batch's row of this slot
        if (lane < 64) wave_softmax_4096(logits + (size_t)row * 4096, lp, lane);
        s.last_value = values[row];
        s.has_last = 1;
        s.buf = 0;
        s.n_evals += 1;
    }
    __syncthreads();
    const int n = s.nmoves;
    const uint16_t* ml = moves + (size_t)i * MAXM;
    mixed_legal_weights(cfg, lp, ml, n, gam, np_mt + (size_t)i * MT_WORDS, mt3, scratch, vals, lane, cfg.eps);
    // random.choices (:162-167): the total, then random() drawn by the whole
    // workgroup (a twist of the CPython state, every 312 plies of a game, runs
    // block-parallel in LDS -- one slot's serial twist would stretch the launch)
    __shared__ double s_total;
    if (lane == 0) {
        double total = 0.0;
        for (int j = 0; j < n; ++j) total = total + vals[j];
        s_total = total;
    }
    __syncthreads();
    uint32_t* py = py_mt + (size_t)i * MT_WORDS;
    if (!isfinite(s_total)) {
        // every gamma draw of the ply was 0 (only a tiny alpha can do this):
        // noise = 0 * (1/0) = NaN, and the reference's random.choices raises
        // ValueError('Total of weights must be finite') -- an error, not a move
        if (lane == 0) atomicOr(&ctr->error, 8);
        return;
    }
    if (s_total == 0.0) {
        if (lane == 0) s_pick = mt_randbelow_serial(py, n);  // random.choice
    } else {
        const double r = block_mt_random(py, mt3, lane);
        if (lane == 0) s_pick = choose_from(vals, cum, n, s_total, r);
    }
    __syncthreads();
    commit_move(cfg, s, i, ml[s_pick], boards, rec, last_board, ctr, lane);
    if (lane == 0) slots[i] = s;
}

// ------------------------------------------------------------- finish ----
// two waves per slot: wave 1 takes the slot's next game and seeds its CPython
// stream (the longer chain) while wave 0 scores the finished game, then sets up
// the next one and seeds its numpy stream
__global__ __launch_bounds__(128) void k_finish(DevCfg cfg, Slot* slots, int8_t* boards, uint16_t* moves,
                                                uint32_t* np_mt, uint32_t* py_mt, kv_game* games, Ctr* ctr) {
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Slot s = slots[i];
    if (s.status != ST_FINISHED) return;
    int8_t* board = boards + (size_t)i * 64;
    // the slot's next game first, so that wave 1 seeds its CPython stream (the
    // longer chain) while wave 0 scores the finished game
    __shared__ long long s_next;
    if (tid == 64) {
        long long next = -1;
        if (cfg.recycle) {
            const unsigned long long k = atomicAdd(&ctr->next_game, 1ull);
            if ((long long)k < cfg.n_games) next = (long long)k;
        }
        s_next = next;
    }
    __syncthreads();
    const long long k = s_next;
    const long long gid = cfg.id_base + k * cfg.id_stride;
    const unsigned long long sd = cfg.seed + (unsigned long long)gid;
    if (wave == 1) {
        if (k >= 0 && cfg.seed_mode == KV_SEED_PER_GAME) wave_seed_python(py_mt + (size_t)i * MT_WORDS, sd, lane);
        return;
    }
    // outcome (:210-238)
    if (s.end_kind == END_MAXED) {
        s.outcome = 0;
        s.reason = 0;
    } else if (s.end_kind == END_NOMOVES && s.movegen_clean) {
        // k_movegen's getValidMoves on this very position found no moves and
        // rewrote nothing, so both getValidMoves calls of the chain below would
        // return none on it: inCheck alone decides mate / stalemate
        const Pos p = wave_pos(board[lane], s.wtm, s.wkr, s.wkc, s.bkr, s.bkc, s.flags, s.ep);
        const bool chk = in_check(p);
        s.outcome = chk ? (p.wtm ? -1 : 1) : 0;
        s.reason = chk ? 2 : 3;
    } else if (s.end_kind != END_RESIGN) {
        Pos p = wave_pos(board[lane], s.wtm, s.wkr, s.wkc, s.bkr, s.bkc, s.flags, s.ep);
        uint16_t* ml = moves + (size_t)i * MAXM;
        const bool chk = in_check(p);
        int n1 = -1;
        if (chk) n1 = wave_valid_moves(p, ml, MAXM, lane);
        if (chk && n1 == 0) {
            s.outcome = p.wtm ? -1 : 1;
            s.reason = 2;
        } else if (wave_valid_moves(p, ml, MAXM, lane) == 0) {
            s.outcome = 0;
            s.reason = 3;
        } else {
            const bool kings_only = (p.w | p.b) == p.K;
            s.outcome = 0;
            s.reason = kings_only ? 4 : 5;  // material branch: always 0 (see oracle/kv_oracle.c)
        }
        board[lane] = (int8_t)pos_at(p, lane);
        s.wtm = p.wtm;
        s.wkr = p.wkr; s.wkc = p.wkc; s.bkr = p.bkr; s.bkc = p.bkc;
        s.flags = p.flags;
        s.ep = p.ep;
    }
    if (tid == 0) {
        // flush of a non-empty buffer (:202-208): one more forward call
        if (cfg.sims == 0 && s.buf > 0) {
            s.n_evals += 1;
            if (cfg.seed_mode == KV_SEED_SEQUENTIAL) s.need_flush = 1;
        }
        const unsigned long long gi = atomicAdd(&ctr->games_count, 1ull);
        kv_game gm;
        gm.game_id = s.game_id;
        gm.plies = s.ply;
        gm.outcome = s.outcome;
        gm.reward = s.outcome == 1 ? 1.0f : (s.outcome == 0 ? 0.2f : -1.0f);
        gm.reason = s.reason;
        gm.n_evals = s.n_evals;
        gm.pad = 0;
        games[gi % (unsigned long long)cfg.games_cap] = gm;
        s.status = ST_IDLE;
    }
    if (k >= 0) {  // the slot starts game k: board + numpy stream by wave 0, fields by thread 0
        const int8_t* v = start_vec(cfg, gid);
        board[lane] = v ? v[lane] : kStart[lane];
        if (cfg.seed_mode == KV_SEED_PER_GAME) wave_seed_genrand(np_mt + (size_t)i * MT_WORDS, (uint32_t)sd, lane);
        if (tid == 0) start_game_fields(cfg, s, gid);
    }
    if (tid == 0) slots[i] = s;
}

// KV_EVAL_LAZY above 16 slots: the boards of the slots whose network row the
// schedule consumes this step (the only rows self_play.py reads: :147-150),
// gathered in slot order into a compact batch; row_of[i] = the slot's row or
// -1. A batch of 1-16 rows is padded to 17 with copies of its first board: the
// network is batch-invariant bit for bit inside its > 16-board class (the
// class of the all-slots batch of faithful mode), so every consumed row equals
// the faithful row and the games are identical (tests/test_engine_gpu.py).
__global__ __launch_bounds__(1024) void k_compact(DevCfg cfg, const Slot* slots, const int8_t* boards,
                                                  int8_t* comp_boards, int* row_of, Ctr* ctr) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < cfg.slots; c0 += 1024) {
        const int i = c0 + tid;
        const bool need = i < cfg.slots && slots[i].status == ST_ACTIVE && slots[i].consumed;
        const unsigned long long bal = __ballot(need);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int k = 0; k < w; ++k) off += wsum[k];
        const int row = off + __popcll(bal & ((1ull << lane) - 1));
        if (i < cfg.slots) row_of[i] = need ? row : -1;
        if (need)
            for (int q = 0; q < 4; ++q)
                ((u32x4*)(comp_boards + (size_t)row * 64))[q] = ((const u32x4*)(boards + (size_t)i * 64))[q];
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < 16; ++k) base += wsum[k];
        __syncthreads();
    }
    const int cnt = base, padded = cnt > 0 && cnt < 17 ? 17 : cnt;
    for (int r = cnt + tid / 4; r < padded; r += 256)  // 4 threads per padding row
        ((u32x4*)(comp_boards + (size_t)r * 64))[tid & 3] = ((const u32x4*)comp_boards)[tid & 3];
    if (tid == 0) ctr->comp_rows = padded;
}

// MCTS with fewer active slots than slots (a finite run whose game queue has
// run dry: its last games, a test's tail): the leaf batches carry only the
// active slots' rows. slot_of[r] = the r-th active slot in slot order, rows
// past the count (padding up to the > 16-board class) repeat row 0; row_of[i]
// = the slot's row or -1. The network is batch-invariant bit for bit inside a
// class, so every active slot's leaf row equals its row in the full batch and
// the searches are unchanged (tests/test_mcts_gpu.py). With kv_config.reuse_tree (node != NULL) the batch is
// that of the slots still searching inside a ply: active and live, the root holding fewer than sims visits
// (kv_config.fast_sims, tgt != NULL: fewer than the ply's own target tgt[i]).
__global__ __launch_bounds__(1024) void k_compact_active(DevCfg cfg, const Slot* slots, int rows, int* slot_of,
                                                         int* row_of, Ctr* ctr, const NodeRec* node, int ncap,
                                                         int sims, const int* tgt) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < cfg.slots; c0 += 1024) {
        const int i = c0 + tid;
        const bool act = i < cfg.slots && slots[i].status == ST_ACTIVE &&
                         (node == nullptr || node[(size_t)i * ncap].N - 1 < (tgt ? tgt[i] : sims));
        const unsigned long long bal = __ballot(act);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int k = 0; k < w; ++k) off += wsum[k];
        const int row = off + __popcll(bal & ((1ull << lane) - 1));
        if (i < cfg.slots) row_of[i] = act && row < rows ? row : -1;
        if (act && row < rows) slot_of[row] = i;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < 16; ++k) base += wsum[k];
        __syncthreads();
    }
    const int cnt = base < rows ? base : rows;
    // more active (and live) slots than the host sized the batch for: some slot would search on stale leaf rows
    if (tid == 0 && base > rows) atomicOr(&ctr->error, 16);
    __syncthreads();
    const int first = cnt > 0 ? slot_of[0] : 0;
    for (int r = cnt + tid; r < rows; r += 1024) slot_of[r] = first;  // padding rows
}

// this sim-step's leaves of the active slots -> the compact batch (one wave per row)
__global__ __launch_bounds__(64) void k_gather_leaves(const int* slot_of, const int8_t* nn_boards,
                                                      const uint16_t* leaf_moves, const int* leaf_cnt, int8_t* cb,
                                                      uint16_t* cm, int* cc) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int s = slot_of[r];
    cb[(size_t)r * 64 + lane] = nn_boards[(size_t)s * 64 + lane];
    const int n = min(leaf_cnt[s], MAXM);
    if (lane == 0) cc[r] = n;
    for (int j = lane; j < n; j += 64) cm[(size_t)r * MAXM + j] = leaf_moves[(size_t)s * MAXM + j];
}

// the compact batch's outputs back to the slots' rows (padding rows dropped)
__global__ __launch_bounds__(64) void k_scatter_leaves(const int* slot_of, const int* row_of, const float* cl,
                                                       const float* cv, const int* cc, float* leaf_logits,
                                                       float* values) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int s = slot_of[r];
    if (row_of[s] != r) return;
    if (lane == 0) values[s] = cv[r];
    const int n = cc[r];
    for (int j = lane; j < n; j += 64) leaf_logits[(size_t)s * MAXM + j] = cl[(size_t)r * MAXM + j];
}

// Arena (kv_config.arena, DESIGN.md "Arena"), once per ply after k_movegen: the active slots partitioned by the
// net of their mover -- player A (list 0) moves in the game with id g when g is even and white is to move, or g is
// odd and black is; player B (list 1) otherwise. k_compact_active's ballot scan with two ballots per wave, so one
// pass writes both lists in slot order: list_x[r] = the r-th slot of player x, row_of[i] = slot i's row in its own
// list or -1, ctr->arena_n = the two counts (read by the host, which sizes the ply's batches from them). pad_to
// (17 above 16 slots, else 0): a list of 1 .. pad_to - 1 slots is padded to pad_to rows that repeat its first slot,
// the network's > 16-board class; the lists hold max(slots, 17) entries. cap: the active slots the host counted
// before k_movegen -- more on the device is a host / device mismatch (error flag 16).
__global__ __launch_bounds__(1024) void k_arena_split(DevCfg cfg, const Slot* slots, int cap, int pad_to, int* list_a,
                                                      int* list_b, int* row_of, Ctr* ctr) {
    __shared__ int wsum[2][16];
    __shared__ int base[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 2) base[tid] = 0;
    __syncthreads();
    for (int c0 = 0; c0 < cfg.slots; c0 += 1024) {
        const int i = c0 + tid;
        bool act = false;
        int x = 0;
        if (i < cfg.slots) {
            const Slot s = slots[i];
            act = s.status == ST_ACTIVE;
            x = (((s.game_id & 1) == 0) == (s.wtm != 0)) ? 0 : 1;
        }
        const unsigned long long bal_a = __ballot(act && x == 0), bal_b = __ballot(act && x == 1);
        if (lane == 0) {
            wsum[0][w] = __popcll(bal_a);
            wsum[1][w] = __popcll(bal_b);
        }
        __syncthreads();
        int off = base[x];
        for (int k = 0; k < w; ++k) off += wsum[x][k];
        const int row = off + __popcll((x ? bal_b : bal_a) & ((1ull << lane) - 1));
        if (i < cfg.slots) row_of[i] = act ? row : -1;
        if (act) (x ? list_b : list_a)[row] = i;  // row < the list's active slots <= cfg.slots
        __syncthreads();
        if (tid < 2)
            for (int k = 0; k < 16; ++k) base[tid] += wsum[tid][k];
        __syncthreads();
    }
    const int na = base[0], nb = base[1];
    if (tid == 0) {
        ctr->arena_n[0] = na;
        ctr->arena_n[1] = nb;
        if (na + nb > cap) atomicOr(&ctr->error, 16);
    }
    if (na > 0 && na < pad_to)
        for (int r = na + tid; r < pad_to; r += 1024) list_a[r] = list_a[0];  // padding rows
    if (nb > 0 && nb < pad_to)
        for (int r = nb + tid; r < pad_to; r += 1024) list_b[r] = list_b[0];
}

// kv_config.leaves > 1 (DESIGN.md "Several leaves per game in self-play"), once per sim-step after the select: the
// dense leaf batch. The select left descent j of slot i at row i * L + j with lcnt[row] = the leaf's moves, 0 for a
// row without a pending leaf (an idle slot, one whose root holds sims backups, a descent that was dropped or ended
// the game). One workgroup strides over the slots x L counts, k_arena_split's ballot scan per 1,024 rows: list_x[r]
// = the r-th pending row of player x in row order (self-play: one list; arena: the player of the slot's mover),
// row_of[row] = its place in its list or -1, a list of 1 .. pad_to - 1 rows padded to pad_to by repeating its first.
// lc->pend = the two counts, lc->stepping / remaining = the slots that took a descent / that go on after this
// step's backups: the host's one readback per step. cap: the entries a list holds (error flag 16 beyond). hit
// (kv_config.eval_cache, else NULL): hit[r] != 0 marks a row the cache answered -- not pending for the lists.
__global__ __launch_bounds__(1024) void k_leaves_compact(DevCfg cfg, const Slot* slots, const SearchSlot* ss,
                                                         const int* lcnt, int L, int sims, int arena, int cap,
                                                         int pad_to, int* list_a, int* list_b, int* row_of,
                                                         LeafCtr* lc, Ctr* ctr, const int* hit, const int* tgt) {
    __shared__ int wsum[2][16];
    __shared__ int base[2];
    __shared__ int s_step, s_rem;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 2) base[tid] = 0;
    if (tid == 0) s_step = s_rem = 0;
    __syncthreads();
    int step = 0, rem = 0;
    for (int i = tid; i < cfg.slots; i += 1024) {
        const SearchSlot q = ss[i];
        step += q.accepted > 0;
        rem += q.accepted > 0 && q.done + q.accepted < (tgt ? tgt[i] : sims);  // (fast_sims: the ply's own target)
    }
    if (step) atomicAdd(&s_step, step);
    if (rem) atomicAdd(&s_rem, rem);
    const int rows = cfg.slots * L;
    for (int c0 = 0; c0 < rows; c0 += 1024) {
        const int r = c0 + tid;
        bool pend = false;
        int x = 0;
        if (r < rows) {
            pend = lcnt[r] > 0 && !(hit && hit[r]);
            if (arena && pend) {
                const Slot s = slots[r / L];
                x = (((s.game_id & 1) == 0) == (s.wtm != 0)) ? 0 : 1;
            }
        }
        const unsigned long long bal_a = __ballot(pend && x == 0), bal_b = __ballot(pend && x == 1);
        if (lane == 0) {
            wsum[0][w] = __popcll(bal_a);
            wsum[1][w] = __popcll(bal_b);
        }
        __syncthreads();
        int off = base[x];
        for (int k = 0; k < w; ++k) off += wsum[x][k];
        const int row = off + __popcll((x ? bal_b : bal_a) & ((1ull << lane) - 1));
        if (r < rows) row_of[r] = pend && row < cap ? row : -1;
        if (pend && row < cap) (x ? list_b : list_a)[row] = r;
        __syncthreads();
        if (tid < 2)
            for (int k = 0; k < 16; ++k) base[tid] += wsum[tid][k];
        __syncthreads();
    }
    const int na = base[0], nb = base[1];
    if (tid == 0) {
        lc->pend[0] = na;
        lc->pend[1] = nb;
        lc->stepping = s_step;
        lc->remaining = s_rem;
        if (na > cap || nb > cap) atomicOr(&ctr->error, 16);
    }
    if (na > 0 && na < pad_to)
        for (int r = na + tid; r < pad_to; r += 1024) list_a[r] = list_a[0];  // padding rows
    if (nb > 0 && nb < pad_to)
        for (int r = nb + tid; r < pad_to; r += 1024) list_b[r] = list_b[0];
}

// arena: the root boards of one player's list -> its compact batch (one wave per row)
__global__ __launch_bounds__(64) void k_arena_gather_roots(const int* list, const int8_t* boards, int8_t* cb) {
    const int r = blockIdx.x, lane = threadIdx.x;
    cb[(size_t)r * 64 + lane] = boards[(size_t)list[r] * 64 + lane];
}

// arena: the batch's full 4,096-logit rows and values back to the slots' rows (padding rows dropped)
__global__ __launch_bounds__(256) void k_arena_scatter_roots(const int* list, const int* row_of, const float* cl,
                                                            const float* cv, float* logits, float* values) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int s = list[r];
    if (row_of[s] != r) return;
    if (tid == 0) values[s] = cv[r];
    const float4* src = (const float4*)(cl + (size_t)r * 4096);
    float4* dst = (float4*)(logits + (size_t)s * 4096);
    for (int j = tid; j < 1024; j += 256) dst[j] = src[j];
}

// the flush rows of sequential mode: boards [slots, 2*slots) = last appended board
__global__ void k_flush_rows(DevCfg cfg, const Slot* slots, const int8_t* last_board, int8_t* nn_boards) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= cfg.slots) return;
    nn_boards[(size_t)(cfg.slots + i) * 64 + lane] = slots[i].need_flush ? last_board[(size_t)i * 64 + lane] : 0;
}

}  // namespace kv

// ---------------------------------------------------------------- host --
struct kv_engine {
    kv_config cfg;
    kv::DevCfg dc;
    kv_net* net = nullptr;
    hipStream_t st = nullptr;
    kv::Slot* slots = nullptr;
    int8_t* boards = nullptr;  // [rows][64]: slot boards, then flush rows
    uint16_t* moves = nullptr;
    float* logits = nullptr;
    float* values = nullptr;
    float* last_probs = nullptr;
    int8_t* comp_boards = nullptr;  // KV_EVAL_LAZY above 16 slots: this step's compact batch
    int* row_of = nullptr;
    long long lazy_rows = 0;        // rows sent through the network by the compact batches
    uint32_t* np_mt = nullptr;
    uint32_t* py_mt = nullptr;
    kv_record* rec = nullptr;
    kv_game* games = nullptr;
    int8_t* last_board = nullptr;
    kv::Ctr* ctr = nullptr;
    kv::Ctr* ctr_host = nullptr;  // pinned
    long long steps = 0;
    double wall_ms = 0;
    std::vector<hipEvent_t> ev;  // residual-conv section start/end per forward
    int n_ev_used = 0;
    double nn_res_ms = 0;
    long long nn_res_launches = 0;
    int dom_algo = KV_ALGO_DIRECT, dom_launches = 10;  // what each event pair brackets
    int dom_path = KV_PATH_DIRECT, dom_split = 0;
    double dom_flop = 0;
    const char* dom_kernel = "";
    bool loaded = false;
    // MCTS (sims > 0)
    kv::Tree tree;
    kv::MctsSlot* ms = nullptr;
    int8_t* nn_boards = nullptr;
    float* probs = nullptr;
    float* sqrt_tab = nullptr;
    // MCTS leaf batches of the active slots only (k_compact_active)
    int* mc_slot_of = nullptr;
    int* mc_row_of = nullptr;
    int8_t* mc_boards = nullptr;
    uint16_t* mc_moves = nullptr;
    int* mc_cnt = nullptr;
    float* mc_logits = nullptr;
    float* mc_values = nullptr;
    long long mc_rows = 0;  // leaf rows the compact batches sent through the network
    long long full_rows = 0;  // leaf rows of the full-slot batches (kv_stats.leaf_batch_rows = mc_rows + full_rows)
    // reuse_tree: tree.rem read back with the per-ply counters (pinned), and the slots per rem value
    int* rem_host = nullptr;
    std::vector<int> rem_hist;
    // kv_records_device / kv_root_visits_device copy out of e->rec / root_visits on the caller's
    // stream; the next write to those buffers (kv_run, kv_reset_records) or their release
    // (kv_destroy) waits for that copy on e->st
    hipEvent_t copy_done = nullptr;
    bool copy_pending = false;
    // slot groups of the MCTS sim loop (kv_config.sim_groups resolved: 1 or 2). Two groups: slots [0, S / 2) on
    // the engine stream with the engine's net, the rest on g_st with g_net, a view of that net (its own
    // workspaces, made at the first kv_run after a weight load); g_fork / g_join order the two streams at the
    // ends of a move's sim loop
    int groups = 1;
    hipStream_t g_st = nullptr;
    hipEvent_t g_fork = nullptr, g_join = nullptr;
    kv_net* g_net = nullptr;
    // arena (kv_config.arena): player B's net, and per player x the slot list of this ply (k_arena_split), the
    // compact batch of its rows (boards, the leaves' moves / counts / legal logits, values) and its root rows'
    // full logits; ar_row_of[slot] = the slot's row in its own list. Player A runs on the engine stream, and with
    // two chains (groups == 2) player B on g_st
    kv_net* net_b = nullptr;
    bool loaded_b = false;
    int* ar_list[2] = {nullptr, nullptr};
    int* ar_row_of = nullptr;
    int8_t* ar_boards[2] = {nullptr, nullptr};
    uint16_t* ar_moves[2] = {nullptr, nullptr};
    int* ar_cnt[2] = {nullptr, nullptr};
    float* ar_llogits[2] = {nullptr, nullptr};
    float* ar_values[2] = {nullptr, nullptr};
    float* ar_rlogits[2] = {nullptr, nullptr};
    long long arena_rows[2] = {0, 0};  // kv_stats.arena_rows
    // kv_config.leaves > 1 (leaves: the resolved count, 1 for 0): the per-(slot, descent) workspaces of the step
    // (lw, rows = slots x leaves), the step's dense batch per player x (self-play: x = 0 only) -- the list of its
    // pending rows, their boards / moves / counts / legal logits / values -- lf_row_of[row] = the row's place in
    // its list, and the step's counters on the device and pinned on the host. big: the run's network class is the
    // > 16-row one (slots x leaves > 16); root_rows: the rows of the self-play root batch (17 for fewer slots in
    // the big class)
    int leaves = 1;
    bool big = false;
    int root_rows = 0;
    kv::SearchWs lw = {};
    int* lf_list[2] = {nullptr, nullptr};
    int* lf_row_of = nullptr;
    int8_t* lf_boards[2] = {nullptr, nullptr};
    uint16_t* lf_moves[2] = {nullptr, nullptr};
    int* lf_cnt[2] = {nullptr, nullptr};
    float* lf_logits[2] = {nullptr, nullptr};
    float* lf_values[2] = {nullptr, nullptr};
    float* lf_hlogits = nullptr;  // KV_EVAL_HASH: the full rows k_hash_eval writes
    kv::LeafCtr* lf_ctr = nullptr;
    kv::LeafCtr* lf_ctr_host = nullptr;  // pinned
    long long sim_steps = 0;             // kv_stats.sim_steps
    // kv_config.eval_cache (kv_cache.hip): the table of player x's net (self-play: x = 0 only; ent == nullptr: off),
    // per workspace row the step's hit flag and the entry a miss claimed, and the device's counters
    kv::CacheTab ec_tab[2] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
    int* ec_hit = nullptr;
    int* ec_idx = nullptr;
    kv::CacheCtr* ec_ctr = nullptr;
    // a sim-step's claims are out: set before the probe, cleared once the step's store has handed them back. A step
    // that returned an error in between leaves it set, and the next ply resets the claim words before it probes
    bool ec_claims_out = false;
    // kv_search: an engine serves either kv_run or kv_search (used: 0 neither yet, 1 kv_run, 2 kv_search)
    int used = 0;
    int8_t* starts = nullptr;  // kv_dev_set_starts: [n_starts][80] on the device (dc.starts), nullptr: none set
    kv::SearchWs sw = {};
    size_t sw_rows = 0;           // rows (positions x leaves) the leaf workspaces hold
    int8_t* s_states = nullptr;   // [slots][80]
    int8_t* s_rboards = nullptr;  // root batch [max(slots, 17)][64], [4096] logits and a value per row
    float* s_rlogits = nullptr;
    float* s_rvalues = nullptr;
    float* s_hlogits = nullptr;   // KV_EVAL_HASH: the full rows k_hash_eval writes for the leaf batch
    size_t s_hrows = 0;
    int* s_rem_host = nullptr;    // pinned: trees with done < sims, read back once per sim-step
    // search session (kv_search_advance / kv_search_continue): the trees of the last kv_search; the host
    // keeps each root's status, move count and visits from the last result or advance
    int sess_n = 0;  // 0: no session
    std::vector<kv::SessionSlot> sess_host;
    std::vector<int> sess_done;
    int* s_edge = nullptr;  // [slots]: the edges of the running advance
};

// order e->st after an outstanding device-to-device copy of the engine's buffers on a caller stream
static int eng_wait_copies(kv_engine* e) {
    if (!e->copy_pending) return KV_OK;
    KV_HIP(hipStreamWaitEvent(e->st, e->copy_done, 0));
    e->copy_pending = false;
    return KV_OK;
}

// The engine stream waits for the copy right away (whatever stream the caller used), so two copies on
// two caller streams are both ordered before the next write to e->rec / root_visits; the event is
// kept for kv_destroy, which waits for the last copy before freeing the buffers.
static int eng_note_copy(kv_engine* e, hipStream_t caller) {
    if (!e->copy_done) KV_HIP(hipEventCreateWithFlags(&e->copy_done, hipEventDisableTiming));
    KV_HIP(hipEventRecord(e->copy_done, caller));
    KV_HIP(hipStreamWaitEvent(e->st, e->copy_done, 0));
    e->copy_pending = true;
    return KV_OK;
}

static int eng_counters(kv_engine* e, bool check_error = true) {
    // active slots / plies / rows are summed from the slots only when the host reads them
    hipLaunchKernelGGL(kv::k_count, dim3(1), dim3(256), 0, e->st, e->dc, e->slots, e->ctr);
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(e->ctr_host, e->ctr, sizeof(kv::Ctr), hipMemcpyDeviceToHost, e->st));
    if (e->rem_host)  // reuse_tree: the sim-steps every slot's next ply runs
        KV_HIP(hipMemcpyAsync(e->rem_host, e->tree.rem, (size_t)e->cfg.slots * sizeof(int), hipMemcpyDeviceToHost,
                              e->st));
    KV_HIP(hipStreamSynchronize(e->st));
    if (check_error && e->ctr_host->error) {
        kv::set_error("engine device error flags 0x%x (1: move list overflow, 2: record buffer full, "
                      "4: MCTS tree pool full, %llu expansions dropped -- raise kv_config.tree_edge_cap; "
                      "8: move weights not finite -- every Dirichlet gamma draw of a ply was 0, where the "
                      "reference's random.choices raises ValueError; 16: more active MCTS slots than the compact "
                      "leaf batch holds -- a host / device count mismatch; 32: a carried tree and the position after "
                      "the move disagree (reuse_tree))",
                      e->ctr_host->error, (unsigned long long)e->ctr_host->tree_overflows);
        if (e->ctr_host->error & 32) return KV_EHIP;
        return (e->ctr_host->error & (8 | 16)) ? KV_EINVAL : KV_EOVERFLOW;
    }
    return KV_OK;
}

static int eng_collect_timing(kv_engine* e) {
    for (int k = 0; k + 1 < e->n_ev_used; k += 2) {
        float ms = 0.f;
        KV_HIP(hipEventSynchronize(e->ev[k + 1]));
        KV_HIP(hipEventElapsedTime(&ms, e->ev[k], e->ev[k + 1]));
        e->nn_res_ms += ms;
        e->nn_res_launches += e->dom_launches;
    }
    e->n_ev_used = 0;
    return KV_OK;
}

// kv_config.sim_groups resolved: 0 (auto) is two groups from 2,048 slots in MCTS mode -- each group then keeps
// the fused R3 stem's 1,024-board floor and the GEMM's one-round grid on half the CUs -- else one
// An arena (kv_config.arena) runs its two players' chains on two streams from KV_ARENA_TWO_CHAINS_MIN slots
// (DESIGN.md "Arena" records the measurement the rule comes from)
static int sim_groups_for(const kv_config* cfg) {
    if (cfg->sim_groups == 0 && cfg->leaves > 1) return 1;  // several leaves per game: one chain
    if (cfg->sim_groups == 0 && cfg->arena) return cfg->sims > 0 && cfg->slots >= KV_ARENA_TWO_CHAINS_MIN ? 2 : 1;
    if (cfg->sim_groups == 0) return cfg->sims > 0 && cfg->slots >= 2048 ? 2 : 1;
    return cfg->sim_groups;
}

extern "C" {

int kv_sim_groups_for(const kv_config* cfg) {
    KV_REQUIRE(cfg, KV_EINVAL, "kv_sim_groups_for: NULL");
    KV_REQUIRE(cfg->sim_groups >= 0 && cfg->sim_groups <= 2, KV_EINVAL, "kv_create: sim_groups %d must be 0 (auto), 1 or 2",
               cfg->sim_groups);
    KV_REQUIRE(cfg->leaves >= 0 && cfg->leaves <= KV_MAX_LEAVES, KV_EINVAL,
               "kv_create: leaves %d out of range [0, %d]", cfg->leaves, KV_MAX_LEAVES);
    KV_REQUIRE(cfg->leaves <= 1 || cfg->sim_groups != 2, KV_EINVAL,
               "kv_create: leaves %d with sim_groups 2: several leaves per game run as one chain (sim_groups 0 or 1)",
               cfg->leaves);
    KV_REQUIRE(cfg->sim_groups != 2 || (cfg->sims >= 1 && cfg->slots / 2 > 16), KV_EINVAL,
               "kv_create: sim_groups 2 needs sims >= 1 and more than 16 slots per group (the network's batch class), "
               "got sims %d, slots %d", cfg->sims, cfg->slots);
    return sim_groups_for(cfg);
}

int kv_create(const kv_config* cfg, kv_engine** out) {
    KV_REQUIRE(cfg && out, KV_EINVAL, "kv_create: NULL argument");
    KV_REQUIRE(cfg->slots > 0 && cfg->n_games >= 0, KV_EINVAL, "kv_create: slots must be > 0");
    // numpy's legacy gamma for shape < 1 (the branch restated on the device); a
    // normal double keeps 1/alpha finite, and kv_libm.h's pow is exact over the
    // whole range, subnormal / zero gamma draws of a small alpha included
    KV_REQUIRE(cfg->alpha >= 2.2250738585072014e-308 && cfg->alpha < 1.0, KV_EINVAL,
               "kv_create: DIR_NOISE_ALPHA must be a normal double in (0,1) (legacy gamma shape<1 branch), got %g",
               cfg->alpha);
    KV_REQUIRE(cfg->batch >= 1, KV_EINVAL, "kv_create: SELFPLAY_BATCH_SIZE must be >= 1");
    KV_REQUIRE(cfg->seed_mode == KV_SEED_PER_GAME || cfg->seed_mode == KV_SEED_SEQUENTIAL, KV_EINVAL,
               "kv_create: bad seed_mode");
    KV_REQUIRE(cfg->seed_mode != KV_SEED_SEQUENTIAL || cfg->slots == 1, KV_EINVAL,
               "kv_create: sequential seeding plays games in order on one slot");
    KV_REQUIRE(cfg->sims >= 0 && cfg->sims <= KV_MAX_SIMS, KV_EINVAL,
               "kv_create: sims %d out of range [0, %d] (16-bit edge visit counts and child ids)", cfg->sims,
               KV_MAX_SIMS);
    KV_REQUIRE(cfg->leaves >= 0 && cfg->leaves <= KV_MAX_LEAVES, KV_EINVAL,
               "kv_create: leaves %d out of range [0, %d]", cfg->leaves, KV_MAX_LEAVES);
    KV_REQUIRE(cfg->leaves <= 1 || cfg->eval_mode != KV_EVAL_LAZY, KV_EINVAL,
               "kv_create: leaves %d with eval_mode KV_EVAL_LAZY (lazy: reference move selection only)", cfg->leaves);
    KV_REQUIRE(cfg->leaves <= 1 || cfg->sims >= 1, KV_EINVAL,
               "kv_create: leaves %d with sims %d: several leaves per game are MCTS descents and need sims >= 1",
               cfg->leaves, cfg->sims);
    KV_REQUIRE(cfg->leaves <= 1 || cfg->reuse_tree == 0, KV_EINVAL,
               "kv_create: leaves %d with reuse_tree 1: a carried tree under virtual loss is not built yet",
               cfg->leaves);
    KV_REQUIRE(cfg->eval_cache == 0 || (cfg->eval_cache >= 64 && cfg->eval_cache <= (1 << 24) &&
                                        (cfg->eval_cache & (cfg->eval_cache - 1)) == 0),
               KV_EINVAL, "kv_create: eval_cache %d must be 0 (off) or a power of two in [64, 2^24] (entries per network)",
               cfg->eval_cache);
    KV_REQUIRE(cfg->eval_cache == 0 || cfg->leaves >= 2, KV_EINVAL,
               "kv_create: eval_cache %d with leaves %d: the cache sits in front of the dense leaf batch and needs "
               "leaves >= 2", cfg->eval_cache, cfg->leaves);
    KV_REQUIRE(cfg->tree_edge_cap <= 0 || cfg->tree_edge_cap >= kv::MAXM, KV_EINVAL,
               "kv_create: tree_edge_cap %d must be 0 (auto) or >= KV_MAXM (the root's list)", cfg->tree_edge_cap);
    KV_REQUIRE(cfg->sims == 0 || cfg->seed_mode == KV_SEED_PER_GAME, KV_EINVAL,
               "kv_create: MCTS mode uses per-game seeding");
    KV_REQUIRE(cfg->eval_mode == KV_EVAL_FAITHFUL || cfg->eval_mode == KV_EVAL_HASH ||
                   (cfg->eval_mode == KV_EVAL_LAZY && cfg->sims == 0),
               KV_EINVAL, "kv_create: eval_mode %d not available (lazy: reference move selection only)",
               cfg->eval_mode);
    KV_REQUIRE(cfg->reuse_tree == 0 || cfg->reuse_tree == 1, KV_EINVAL, "kv_create: reuse_tree %d must be 0 or 1",
               cfg->reuse_tree);
    KV_REQUIRE(cfg->reuse_tree == 0 || cfg->sims >= 1, KV_EINVAL,
               "kv_create: reuse_tree carries MCTS subtrees and needs sims >= 1 (sims 0 is the reference move "
               "selection)");
    KV_REQUIRE(cfg->arena == 0 || cfg->arena == 1, KV_EINVAL, "kv_create: arena %d must be 0 or 1", cfg->arena);
    KV_REQUIRE(cfg->arena == 0 || cfg->sims >= 1, KV_EINVAL,
               "kv_create: arena plays each ply's search on the mover's net and needs sims >= 1 (sims 0 is the "
               "reference move selection)");
    KV_REQUIRE(cfg->arena == 0 || cfg->reuse_tree == 0, KV_EINVAL,
               "kv_create: arena with reuse_tree: a tree grown on one net's rows is not the other player's");
    KV_REQUIRE(cfg->arena == 0 || cfg->eval_mode != KV_EVAL_LAZY, KV_EINVAL,
               "kv_create: arena with eval_mode KV_EVAL_LAZY (lazy: reference move selection only)");
    KV_REQUIRE(cfg->fast_sims >= 0 && (cfg->fast_sims == 0 || cfg->sims == 0 || cfg->fast_sims < cfg->sims), KV_EINVAL,
               "kv_create: fast_sims %d out of range: 0 (off) or 1 <= fast_sims < sims (%d)", cfg->fast_sims, cfg->sims);
    KV_REQUIRE(cfg->fast_sims == 0 || cfg->sims >= 1, KV_EINVAL,
               "kv_create: fast_sims %d with sims 0: the fast search is a PUCT search and needs sims >= 1",
               cfg->fast_sims);
    KV_REQUIRE(cfg->fast_sims != 0 || cfg->full_q16 == 0, KV_EINVAL,
               "kv_create: full_q16 %d with fast_sims 0: it is ignored with the feature off and must be 0",
               cfg->full_q16);
    KV_REQUIRE(cfg->fast_sims == 0 || (cfg->full_q16 >= 1 && cfg->full_q16 <= 65536), KV_EINVAL,
               "kv_create: full_q16 %d out of range [1, 65536] (65536: every ply full)", cfg->full_q16);
    KV_REQUIRE(cfg->fast_sims == 0 || cfg->arena == 0, KV_EINVAL,
               "kv_create: fast_sims %d with arena 1: a match measures strength at the full search", cfg->fast_sims);
    KV_REQUIRE(std::isfinite(cfg->forced_k) && cfg->forced_k >= 0.f && cfg->forced_k <= 16.f, KV_EINVAL,
               "kv_create: forced_k %g out of range: 0 (off) or 0 < forced_k <= 16", (double)cfg->forced_k);
    KV_REQUIRE(!(cfg->forced_k > 0.f) || cfg->sims >= 1, KV_EINVAL,
               "kv_create: forced_k %g with sims 0: forced playouts are PUCT descents and need sims >= 1",
               (double)cfg->forced_k);
    KV_REQUIRE(!(cfg->forced_k > 0.f) || cfg->arena == 0, KV_EINVAL,
               "kv_create: forced_k %g with arena 1: a match measures strength at the plain search",
               (double)cfg->forced_k);
    KV_REQUIRE(cfg->sample_plies >= -1, KV_EINVAL,
               "kv_create: sample_plies %d must be 0 (every ply drawn), k > 0 (first maximum from ply k on) or -1 "
               "(first maximum on every ply)", cfg->sample_plies);
    KV_REQUIRE(cfg->sample_plies == 0 || cfg->sims >= 1, KV_EINVAL,
               "kv_create: sample_plies %d is the MCTS move choice and must be 0 with sims 0", cfg->sample_plies);
    const int groups = kv_sim_groups_for(cfg);
    if (groups < 0) return groups;
    KV_HIP(hipSetDevice(cfg->device));
    kv_engine* e = new kv_engine();
    e->cfg = *cfg;
    e->groups = groups;
    if (e->cfg.game_id_stride <= 0) e->cfg.game_id_stride = 1;
    if (e->cfg.record_cap <= 0) e->cfg.record_cap = 1 << 20;
    kv::DevCfg& d = e->dc;
    d.slots = cfg->slots;
    d.n_games = cfg->n_games;
    d.id_base = cfg->game_id_base;
    d.id_stride = e->cfg.game_id_stride;
    d.seed = cfg->seed;
    d.seed_mode = cfg->seed_mode;
    d.max_moves = cfg->max_moves;
    d.batch = cfg->batch;
    d.eps = cfg->eps;
    d.alpha = cfg->alpha;
    d.record_cap = e->cfg.record_cap;
    d.recycle = cfg->recycle;
    d.rows = cfg->seed_mode == KV_SEED_SEQUENTIAL ? 2 * cfg->slots : cfg->slots;
    d.games_cap = std::max<long long>(1, std::min<long long>(cfg->n_games, 1 << 20));
    d.sims = cfg->sims;
    d.eval_mode = cfg->eval_mode;
    d.sample_plies = cfg->sample_plies;
    d.starts = nullptr;
    d.n_starts = 0;
    d.fast_sims = cfg->fast_sims;
    d.full_q16 = cfg->full_q16;
    e->leaves = std::max(cfg->leaves, 1);
    e->big = e->leaves > 1 ? (long long)cfg->slots * e->leaves > 16 : cfg->slots > 16;
    // several leaves in the > 16-row class: a root batch of fewer than 17 slots is padded to 17 rows (empty boards)
    e->root_rows = e->leaves > 1 && e->big ? std::max(d.rows, 17) : d.rows;
    const size_t S = (size_t)cfg->slots, R = (size_t)e->root_rows;
    int rc = KV_OK;
#define ALLOC(ptr, bytes)                                   \
    do {                                                    \
        hipError_t er_ = hipMalloc(&(ptr), (bytes));        \
        if (er_ != hipSuccess) {                            \
            kv::set_error("kv_create: hipMalloc %s (%zu B): %s", #ptr, (size_t)(bytes), hipGetErrorString(er_)); \
            kv_destroy(e);                                  \
            return KV_ENOMEM;                               \
        }                                                   \
    } while (0)
    ALLOC(e->slots, S * sizeof(kv::Slot));
    ALLOC(e->boards, R * 64);
    ALLOC(e->moves, S * kv::MAXM * sizeof(uint16_t));
    ALLOC(e->logits, R * 4096 * sizeof(float));
    ALLOC(e->values, R * sizeof(float));
    ALLOC(e->last_probs, S * 4096 * sizeof(float));
    if (cfg->eval_mode == KV_EVAL_LAZY && S > 16) {
        ALLOC(e->comp_boards, (S + 17) * 64);
        ALLOC(e->row_of, S * sizeof(int));
    }
    ALLOC(e->np_mt, S * kv::MT_WORDS * sizeof(uint32_t));
    ALLOC(e->py_mt, S * kv::MT_WORDS * sizeof(uint32_t));
    ALLOC(e->rec, (size_t)e->cfg.record_cap * sizeof(kv_record));
    ALLOC(e->games, (size_t)d.games_cap * sizeof(kv_game));
    ALLOC(e->last_board, S * 64);
    ALLOC(e->ctr, sizeof(kv::Ctr));
    if (cfg->sims > 0) {
        kv::Tree& t = e->tree;
        t.ncap = cfg->sims + 2;
        // every expansion adds <= MAXM edges: (sims + 1) x MAXM edges can never
        // overflow (C3: 2,048 slots x 801 x 320 x 14 B = 7.3 GB of the 288 GB);
        // a smaller cap is honoured and an overflow raises KV_EOVERFLOW
        const long long full = (long long)kv::MAXM * (cfg->sims + 1);
        // node edge blocks start on 16-edge boundaries (kv_mcts.hip), so a
        // caller's cap is rounded down to a multiple of 16 (MAXM is one) and
        // every expansion still takes at most MAXM edges
        t.ecap = (int)(cfg->tree_edge_cap > 0 ? std::min<long long>(cfg->tree_edge_cap & ~15, full) : full);
        t.c_puct = cfg->c_puct > 0.f ? cfg->c_puct : 1.5f;
        t.sims = cfg->sims;
        const size_t E = S * (size_t)t.ecap, N = S * (size_t)t.ncap;
        ALLOC(t.e_move, E * sizeof(uint16_t));
        ALLOC(t.e_P, E * sizeof(float));
        ALLOC(t.e_N, E * sizeof(uint16_t));
        ALLOC(t.e_W, E * sizeof(float));
        ALLOC(t.e_child, E * sizeof(uint16_t));
        ALLOC(t.node, N * sizeof(kv::NodeRec));
        ALLOC(t.path, N * sizeof(int));
        ALLOC(t.leaf_moves, S * kv::MAXM * sizeof(uint16_t));
        ALLOC(t.leaf_cnt, S * sizeof(int));
        ALLOC(t.leaf_logits, S * kv::MAXM * sizeof(float));
        (void)hipMemset(t.leaf_cnt, 0, S * sizeof(int));
        ALLOC(e->ms, S * sizeof(kv::MctsSlot));
        ALLOC(e->nn_boards, S * 64);
        ALLOC(e->probs, S * 4096 * sizeof(float));
        ALLOC(e->sqrt_tab, (size_t)(t.ncap + 2) * sizeof(float));
        if (cfg->keep_root_visits) ALLOC(t.root_visits, (size_t)e->cfg.record_cap * kv::MAXM * sizeof(uint16_t));
        if (cfg->keep_root_visits == 2) ALLOC(t.root_moves, (size_t)e->cfg.record_cap * kv::MAXM * sizeof(uint16_t));
        if (cfg->eval_mode != KV_EVAL_HASH && S > 1) {
            ALLOC(e->mc_slot_of, S * sizeof(int));
            ALLOC(e->mc_row_of, S * sizeof(int));
            ALLOC(e->mc_boards, S * 64);
            ALLOC(e->mc_moves, S * kv::MAXM * sizeof(uint16_t));
            ALLOC(e->mc_cnt, S * sizeof(int));
            ALLOC(e->mc_logits, S * kv::MAXM * sizeof(float));
            ALLOC(e->mc_values, S * sizeof(float));
        }
        if (cfg->reuse_tree || cfg->fast_sims > 0) ALLOC(t.rem, S * sizeof(int));
        if (cfg->fast_sims > 0) {
            ALLOC(t.tgt, S * sizeof(int));
            (void)hipMemset(t.tgt, 0, S * sizeof(int));
        }
        t.forced_k = cfg->forced_k;
        if (cfg->forced_k > 0.f) {
            ALLOC(t.forced, S * sizeof(int));
            (void)hipMemset(t.forced, 0, S * sizeof(int));
            if (cfg->keep_root_visits)
                ALLOC(t.root_targets, (size_t)e->cfg.record_cap * kv::MAXM * sizeof(uint16_t));
        }
        if (e->leaves > 1) {
            kv::SearchWs& w = e->lw;
            const size_t rows = S * (size_t)e->leaves, RR = std::max<size_t>(rows, 17);
            ALLOC(t.e_V, E * sizeof(uint16_t));
            ALLOC(w.ss, S * sizeof(kv::SearchSlot));
            ALLOC(w.lf, rows * sizeof(kv::SearchLeaf));
            ALLOC(w.paths, rows * (size_t)t.ncap * sizeof(int));
            ALLOC(w.lboards, rows * 64);
            ALLOC(w.lmoves, rows * kv::MAXM * sizeof(uint16_t));
            ALLOC(w.lcnt, rows * sizeof(int));
            ALLOC(w.llogits, rows * kv::MAXM * sizeof(float));
            ALLOC(w.lvalues, rows * sizeof(float));
            ALLOC(e->lf_row_of, rows * sizeof(int));
            ALLOC(e->lf_ctr, sizeof(kv::LeafCtr));
            (void)hipMemset(t.e_V, 0, E * sizeof(uint16_t));
            (void)hipMemset(w.ss, 0, S * sizeof(kv::SearchSlot));
            (void)hipMemset(w.lcnt, 0, rows * sizeof(int));
            for (int x = 0; x < (cfg->arena ? 2 : 1); ++x) {
                ALLOC(e->lf_list[x], RR * sizeof(int));
                ALLOC(e->lf_boards[x], RR * 64);
                ALLOC(e->lf_moves[x], RR * kv::MAXM * sizeof(uint16_t));
                ALLOC(e->lf_cnt[x], RR * sizeof(int));
                ALLOC(e->lf_logits[x], RR * kv::MAXM * sizeof(float));
                ALLOC(e->lf_values[x], RR * sizeof(float));
            }
            if (cfg->eval_mode == KV_EVAL_HASH) ALLOC(e->lf_hlogits, RR * 4096 * sizeof(float));
            if (cfg->eval_cache) {
                ALLOC(e->ec_hit, rows * sizeof(int));
                ALLOC(e->ec_idx, rows * sizeof(int));
                ALLOC(e->ec_ctr, sizeof(kv::CacheCtr));
                (void)hipMemset(e->ec_hit, 0, rows * sizeof(int));
                (void)hipMemset(e->ec_idx, 0, rows * sizeof(int));
                (void)hipMemset(e->ec_ctr, 0, sizeof(kv::CacheCtr));
                for (int x = 0; x < (cfg->arena ? 2 : 1); ++x) {
                    ALLOC(e->ec_tab[x].claim, (size_t)cfg->eval_cache * sizeof(int));
                    ALLOC(e->ec_tab[x].ent, (size_t)cfg->eval_cache * KV_CACHE_ENTRY_BYTES);
                    e->ec_tab[x].mask = (unsigned)cfg->eval_cache - 1;
                    if (kv::cache_clear(e->ec_tab[x], 0) != KV_OK || hipDeviceSynchronize() != hipSuccess) {
                        kv_destroy(e);
                        return KV_EHIP;
                    }
                }
            }
        }
        if (cfg->arena) {
            const size_t RR = std::max<size_t>(S, 17);  // a list of 1-16 slots is padded to 17 rows above 16 slots
            ALLOC(e->ar_row_of, S * sizeof(int));
            for (int x = 0; x < 2; ++x) {
                ALLOC(e->ar_list[x], RR * sizeof(int));
                ALLOC(e->ar_boards[x], RR * 64);
                ALLOC(e->ar_moves[x], RR * kv::MAXM * sizeof(uint16_t));
                ALLOC(e->ar_cnt[x], RR * sizeof(int));
                ALLOC(e->ar_llogits[x], RR * kv::MAXM * sizeof(float));
                ALLOC(e->ar_values[x], RR * sizeof(float));
                ALLOC(e->ar_rlogits[x], RR * 4096 * sizeof(float));
            }
        }
        t.ms = e->ms;
        std::vector<float> sq(t.ncap + 2);
        for (int k = 0; k < t.ncap + 2; ++k) sq[k] = (float)sqrt((double)k);
        if (hipMemcpy(e->sqrt_tab, sq.data(), sq.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            kv_destroy(e);
            kv::set_error("kv_create: sqrt table copy");
            return KV_EHIP;
        }
        t.sqrt_tab = e->sqrt_tab;
        (void)hipMemset(e->ms, 0, S * sizeof(kv::MctsSlot));
    }
#undef ALLOC
    if (hipHostMalloc(&e->ctr_host, sizeof(kv::Ctr)) != hipSuccess) {
        kv_destroy(e);
        kv::set_error("kv_create: hipHostMalloc failed");
        return KV_ENOMEM;
    }
    if (e->leaves > 1 && hipHostMalloc(&e->lf_ctr_host, sizeof(kv::LeafCtr)) != hipSuccess) {
        e->lf_ctr_host = nullptr;
        kv_destroy(e);
        kv::set_error("kv_create: hipHostMalloc failed");
        return KV_ENOMEM;
    }
    if (e->tree.rem && hipHostMalloc(&e->rem_host, S * sizeof(int)) != hipSuccess) {
        e->rem_host = nullptr;
        kv_destroy(e);
        kv::set_error("kv_create: hipHostMalloc failed");
        return KV_ENOMEM;
    }
    if ((rc = kv_net_create(cfg->device, &e->net)) || (rc = kv_net_set_precision(e->net, cfg->precision)) ||
        (rc = kv_net_set_algo(e->net, cfg->algo))) {
        kv_destroy(e);
        return rc;
    }
    if (cfg->arena && ((rc = kv_net_create(cfg->device, &e->net_b)) ||
                       (rc = kv_net_set_precision(e->net_b, cfg->precision)) ||
                       (rc = kv_net_set_algo(e->net_b, cfg->algo)))) {
        kv_destroy(e);
        return rc;
    }
    if (hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking) != hipSuccess) {
        kv_destroy(e);
        kv::set_error("kv_create: stream");
        return KV_EHIP;
    }
    if (e->groups == 2 && (hipStreamCreateWithFlags(&e->g_st, hipStreamNonBlocking) != hipSuccess ||
                           hipEventCreateWithFlags(&e->g_fork, hipEventDisableTiming) != hipSuccess ||
                           hipEventCreateWithFlags(&e->g_join, hipEventDisableTiming) != hipSuccess)) {
        kv_destroy(e);
        kv::set_error("kv_create: group stream");
        return KV_EHIP;
    }
    (void)hipMemsetAsync(e->boards, 0, R * 64, e->st);
    (void)hipMemsetAsync(e->ctr, 0, sizeof(kv::Ctr), e->st);
    (void)hipMemsetAsync(e->last_probs, 0, S * 4096 * sizeof(float), e->st);
    kv::Ctr c0;
    memset(&c0, 0, sizeof(c0));
    c0.next_game = (unsigned long long)std::min<long long>(cfg->n_games, cfg->slots);
    (void)hipMemcpyAsync(e->ctr, &c0, sizeof(c0), hipMemcpyHostToDevice, e->st);
    hipLaunchKernelGGL(kv::k_init, dim3((cfg->slots + 63) / 64), dim3(64), 0, e->st, d, e->slots, e->boards,
                       e->np_mt, e->py_mt, e->ctr);
    KV_HIP(hipGetLastError());
    // reuse_tree: no slot holds a tree yet -- rem = sims (fast_sims: ply 0's target, with or without reuse_tree) for
    // the slots k_init started, 0 for the idle ones
    if (e->tree.rem && (rc = cfg->reuse_tree ? kv::mcts_carry(d, e->tree, e->slots, e->ctr, e->st)
                                             : kv::mcts_targets(d, e->tree, e->slots, e->st))) {
        kv_destroy(e);
        return rc;
    }
    KV_HIP(hipStreamSynchronize(e->st));
    *out = e;
    return KV_OK;
}

int kv_load_weights(kv_engine* e, const float* packed, size_t n_floats) {
    KV_REQUIRE(e, KV_EINVAL, "kv_load_weights: NULL engine");
    KV_HIP(hipStreamSynchronize(e->st));  // the load (and its calibration) runs on the null stream
    kv::net_view_destroy(e->g_net);  // (idle: the group stream joins the engine stream at every move's end)
    e->g_net = nullptr;
    int rc = kv_net_load(e->net, packed, n_floats);
    if (rc == KV_OK) e->loaded = true;
    if (e->ec_tab[0].ent) {  // kv_config.eval_cache: the rows of the weights before are not this net's
        const int rc2 = kv::cache_clear(e->ec_tab[0], e->st);
        if (rc2) return rc2;
        KV_HIP(hipStreamSynchronize(e->st));
    }
    return rc;
}

int kv_load_weights_b(kv_engine* e, const float* packed, size_t n_floats) {
    KV_REQUIRE(e, KV_EINVAL, "kv_load_weights_b: NULL engine");
    KV_REQUIRE(e->cfg.arena == 1, KV_EINVAL,
               "kv_load_weights_b: the engine was created with arena 0 (self-play has one network)");
    KV_HIP(hipStreamSynchronize(e->st));  // (the group stream joins the engine stream at every ply's end)
    int rc = kv_net_load(e->net_b, packed, n_floats);
    if (rc == KV_OK) e->loaded_b = true;
    if (e->ec_tab[1].ent) {  // kv_config.eval_cache: player B's table
        const int rc2 = kv::cache_clear(e->ec_tab[1], e->st);
        if (rc2) return rc2;
        KV_HIP(hipStreamSynchronize(e->st));
    }
    return rc;
}

int kv_engine_calibration(kv_engine* e, kv_calib* out) {
    KV_REQUIRE(e && out, KV_EINVAL, "kv_engine_calibration: NULL argument");
    return kv_net_calibration(e->net, out);
}

int kv_engine_calibration_b(kv_engine* e, kv_calib* out) {
    KV_REQUIRE(e && out, KV_EINVAL, "kv_engine_calibration_b: NULL argument");
    KV_REQUIRE(e->cfg.arena == 1, KV_EINVAL,
               "kv_engine_calibration_b: the engine was created with arena 0 (self-play has one network)");
    return kv_net_calibration(e->net_b, out);
}

int kv_set_max_moves(kv_engine* e, int max_moves) {
    KV_REQUIRE(e, KV_EINVAL, "kv_set_max_moves: NULL");
    e->cfg.max_moves = max_moves;
    e->dc.max_moves = max_moves;
    return KV_OK;
}

// test-only (kv.h): where the engine's games start. The vectors are checked as kv_search checks its positions
int kv_dev_set_starts(kv_engine* e, const int8_t* states, int n) {
    KV_REQUIRE(e, KV_EINVAL, "kv_dev_set_starts: NULL engine");
    KV_REQUIRE(e->used == 0, KV_EINVAL,
               "kv_dev_set_starts: this engine has %s; the starts are set on a fresh engine only",
               e->used == 1 ? "run self-play (kv_run)" : "searched positions (kv_search)");
    KV_REQUIRE(states ? n >= 1 : n == 0, KV_EINVAL,
               "kv_dev_set_starts: %d states with %s (at least 1 with states; NULL and 0 restore the initial position)",
               n, states ? "a pointer" : "NULL");
    for (int i = 0; i < n; ++i) {
        const int8_t* v = states + (size_t)i * 80;
        bool ok = (v[64] == 0 || v[64] == 1) && v[75] >= -1 && v[75] < 8 && v[76] >= -1 && v[76] < 8 &&
                  (v[75] < 0) == (v[76] < 0);
        for (int q = 0; q < 64; ++q) ok = ok && v[q] >= 0 && v[q] <= 12;
        for (int q = 65; q < 69; ++q) ok = ok && v[q] >= 0 && v[q] < 8;
        KV_REQUIRE(ok, KV_EINVAL, "kv_dev_set_starts: position %d is not a state vector (codes 0..12, wtm 0/1, king "
                   "squares 0..7, ep -1..7)", i);
    }
    KV_HIP(hipSetDevice(e->cfg.device));
    KV_HIP(hipStreamSynchronize(e->st));
    if (e->starts) KV_HIP(hipFree(e->starts));
    e->starts = nullptr;
    e->dc.starts = nullptr;
    e->dc.n_starts = 0;
    if (n > 0) {
        KV_HIP(hipMalloc((void**)&e->starts, (size_t)n * 80));
        KV_HIP(hipMemcpy(e->starts, states, (size_t)n * 80, hipMemcpyHostToDevice));
        e->dc.starts = e->starts;
        e->dc.n_starts = n;
    }
    // the games k_init started are re-seated
    hipLaunchKernelGGL(kv::k_set_starts, dim3((e->cfg.slots + 63) / 64), dim3(64), 0, e->st, e->dc, e->slots,
                       e->boards);
    KV_HIP(hipGetLastError());
    KV_HIP(hipStreamSynchronize(e->st));
    return KV_OK;
}

// one network pass over `rows` boards (or the hash test evaluator), with the
// residual-tower section bracketed by HIP events for the roofline; `leaf`:
// the MCTS leaf batch, whose policy is only the leaves' legal moves
// (kv_net_forward_boards_legal into tree.leaf_logits)
// `comp`: the leaf batch is the compact active-slot batch (e->mc_*) instead of the slots' rows
// slot0 / group (the MCTS leaf batch of slots [slot0, slot0 + rows) only): group 1 runs on the group stream with
// the group's net
static int eng_eval(kv_engine* e, const int8_t* boards, int rows, bool leaf = false, bool comp = false, int slot0 = 0,
                    int group = 0) {
    kv_net* net = group ? e->g_net : e->net;
    hipStream_t st = group ? e->g_st : e->st;
    float* logits = e->logits + (size_t)slot0 * 4096;
    float* values = comp ? e->mc_values : e->values + slot0;
    if (e->dc.eval_mode == KV_EVAL_HASH) {
        int rc = kv::hash_eval(boards, rows, logits, values, st);
        if (rc || !leaf) return rc;
        kv::Tree ts = e->tree;
        ts.leaf_cnt += slot0;
        ts.leaf_logits += (size_t)slot0 * kv::MAXM;
        return kv::hash_legal(ts, rows, st);  // its logits (all 0) in the compact layout
    }
    if ((size_t)e->n_ev_used + 2 > e->ev.size()) {
        for (int k = 0; k < 2; ++k) {
            hipEvent_t x;
            KV_HIP(hipEventCreate(&x));
            e->ev.push_back(x);
        }
    }
    kv::net_set_res_events(net, e->ev[e->n_ev_used], e->ev[e->n_ev_used + 1]);
    e->n_ev_used += 2;
    const int rc = leaf ? kv::net_forward_boards_legal_internal(net, boards, rows,
                                                                comp ? e->mc_moves : e->tree.leaf_moves + (size_t)slot0 * kv::MAXM,
                                                                comp ? e->mc_cnt : e->tree.leaf_cnt + slot0, kv::MAXM,
                                                                comp ? e->mc_logits
                                                                     : e->tree.leaf_logits + (size_t)slot0 * kv::MAXM,
                                                                values, st)
                        : kv::net_forward_boards_internal(net, boards, rows, logits, values, st);
    kv::net_set_res_events(net, nullptr, nullptr);
    kv::net_dom_info(net, &e->dom_algo, &e->dom_launches, &e->dom_flop, &e->dom_path, &e->dom_split,
                     &e->dom_kernel);
    return rc;
}

}  // extern "C"

// Sim-steps [k0, k1) of a move's `steps` on the full-slot leaf batch as two slot groups (kv_config.sim_groups):
// each group's chain -- leaf forward, then backup fused with the next select -- runs on its own stream with its
// own network workspaces, no host sync and no event between the chains inside the loop. The engine stream (group
// 0's) has run the root and the first select for every slot; the group stream forks from it here and joins it
// after the last step. Every board's network row is independent of its batch and every slot's tree and RNG are
// its own, so the results are those of one group bit for bit. While both chains are in flight each net's R3
// GEMM sizes its grid for half the CUs (kv_nn.hip gemm_cus).
static int eng_group_sims(kv_engine* e, int k0, int k1, int steps, bool reuse) {
    const kv::Tree& t = e->tree;
    const int S = e->cfg.slots, h = S / 2;
    int rc = KV_OK;
    if (k0 >= k1) return KV_OK;
    if (!e->g_net && (rc = kv::net_view_create(e->net, &e->g_net))) return rc;
    kv::net_set_cu_share(e->net, 2);
    kv::net_set_cu_share(e->g_net, 2);
    KV_HIP(hipEventRecord(e->g_fork, e->st));
    KV_HIP(hipStreamWaitEvent(e->g_st, e->g_fork, 0));
    for (int k = k0; k < k1 && !rc; ++k) {
        for (int g = 0; g < 2 && !rc; ++g) {
            const int s0 = g ? h : 0, n = g ? S - h : h;
            hipStream_t st = g ? e->g_st : e->st;
            if ((rc = eng_eval(e, e->nn_boards + (size_t)s0 * 64, n, true, false, s0, g))) break;
            rc = k + 1 < steps ? kv::mcts_backup_select(e->dc, t, e->slots, e->boards, e->logits, e->values, e->probs,
                                                        e->nn_boards, e->ctr, st, s0, n, reuse)
                               : kv::mcts_backup(e->dc, t, e->slots, e->logits, e->values, e->probs, e->ctr, st, s0, n,
                                                 reuse);
        }
        e->full_rows += S;
    }
    kv::net_set_cu_share(e->net, 1);
    // the join is enqueued on every exit, so that the engine stream never runs ahead of the group stream
    const hipError_t j0 = hipEventRecord(e->g_join, e->g_st);
    const hipError_t j1 = hipStreamWaitEvent(e->st, e->g_join, 0);
    if (rc) return rc;
    KV_HIP(j0);
    KV_HIP(j1);
    return KV_OK;
}

// One ply's root and sim-steps with kv_config.reuse_tree (DESIGN.md "Carried subtrees in self-play"). The host
// read every slot's rem with the last counters (0 for a slot that was not active), so it knows for every
// sim-step k the live count #{rem > k} and runs max rem steps. While every slot is live the full-slot batch
// runs as without reuse; from the first step with a slot that is not, the leaf batch is the compact batch of
// the active and live slots, rebuilt at every step whose live count is lower than at the last rebuild by at
// least KV_REUSE_COMPACT_STEP. A slot that k_movegen finished this ply only makes the host's counts upper
// bounds (padding rows); more live slots on the device than the batch holds raise error flag 16.
// kv_config.fast_sims takes this path with or without reuse_tree: rem is then each slot's own target less its carried
// visits (k_mcts_carry / k_mcts_targets), 0 for a fast ply whose carried root already holds its target.
static int eng_reuse_sims(kv_engine* e, int act) {
    const kv::Tree& t = e->tree;
    const int S = e->cfg.slots, sims = e->dc.sims;
    int rc = KV_OK;
    std::vector<int>& hist = e->rem_hist;  // hist[r]: slots whose ply runs r sim-steps
    hist.assign((size_t)sims + 2, 0);
    int steps = 0, counted = 0;
    for (int i = 0; i < S; ++i) {
        const int r = std::min(std::max(e->rem_host[i], 0), sims);
        hist[r] += 1;
        steps = std::max(steps, r);
        counted += r > 0;
    }
    // (fast_sims with reuse_tree: a fast ply whose carried root already holds its target runs no step)
    KV_REQUIRE(t.tgt && e->cfg.reuse_tree ? counted <= act : counted == act, KV_EHIP,
               "kv_run: %d active slots, %d with sim-steps to run (reuse_tree / fast_sims)", act, counted);
    e->sim_steps += steps;
    if ((rc = kv::mcts_root(e->dc, t, e->slots, e->moves, e->logits, e->values, e->probs, e->np_mt, e->ctr, e->st)))
        return rc;
    if ((rc = kv::mcts_select(e->dc, t, e->slots, e->boards, e->nn_boards, e->ctr, e->st, 0, S, true))) return rc;
    int live = counted;  // slots with rem > k
    int compacted = -1;  // the live count at the last compaction of this ply (-1: none yet)
    int R = 0;
    // two slot groups: the leading steps at which every slot is live (the full-slot batch) run as groups; from
    // the first compact batch on the ply runs as one group
    int kg = 0;
    if (e->groups == 2 && counted == S) {
        int lv = counted;
        for (; kg < steps; ++kg) {
            if (kg > 0) lv -= hist[kg];
            if (e->mc_slot_of != nullptr && lv < S) break;  // step kg runs the compact batch
        }
        if ((rc = eng_group_sims(e, 0, kg, steps, true))) return rc;
    }
    for (int k = 0; k < steps; ++k) {
        if (k > 0) live -= hist[k];  // the slots whose last step was k - 1
        if (k < kg) continue;
        const bool comp = e->mc_slot_of != nullptr && live < S;
        if (comp) {
            if (compacted < 0 || compacted - live >= KV_REUSE_COMPACT_STEP) {
                R = S > 16 ? std::max(live, 17) : live;
                hipLaunchKernelGGL(kv::k_compact_active, dim3(1), dim3(1024), 0, e->st, e->dc, e->slots, R,
                                   e->mc_slot_of, e->mc_row_of, e->ctr, (const kv::NodeRec*)t.node, t.ncap, sims,
                                   (const int*)t.tgt);
                KV_HIP(hipGetLastError());
                compacted = live;
            }
            hipLaunchKernelGGL(kv::k_gather_leaves, dim3(R), dim3(64), 0, e->st, e->mc_slot_of, e->nn_boards,
                               t.leaf_moves, t.leaf_cnt, e->mc_boards, e->mc_moves, e->mc_cnt);
            KV_HIP(hipGetLastError());
            if ((rc = eng_eval(e, e->mc_boards, R, true, true))) return rc;
            hipLaunchKernelGGL(kv::k_scatter_leaves, dim3(R), dim3(64), 0, e->st, e->mc_slot_of, e->mc_row_of,
                               e->mc_logits, e->mc_values, e->mc_cnt, t.leaf_logits, e->values);
            KV_HIP(hipGetLastError());
            e->mc_rows += R;
        } else {
            if ((rc = eng_eval(e, e->nn_boards, S, true))) return rc;
            e->full_rows += S;
        }
        rc = k + 1 < steps ? kv::mcts_backup_select(e->dc, t, e->slots, e->boards, e->logits, e->values, e->probs,
                                                    e->nn_boards, e->ctr, e->st, 0, S, true)
                           : kv::mcts_backup(e->dc, t, e->slots, e->logits, e->values, e->probs, e->ctr, e->st, 0, S,
                                             true);
        if (rc) return rc;
    }
    return KV_OK;
}

// one network pass of an arena batch: player x's net (or the hash test evaluator, B's value negated) over the R
// rows of its compact batch on `st` -- the root rows' full logits into ar_rlogits, or the leaves' legal logits
static int arena_eval(kv_engine* e, int x, int R, bool leaf, hipStream_t st) {
    kv_net* net = x ? e->net_b : e->net;
    if (e->dc.eval_mode == KV_EVAL_HASH) {
        int rc = kv::hash_eval(e->ar_boards[x], R, e->ar_rlogits[x], e->ar_values[x], st, x == 1);
        if (rc || !leaf) return rc;
        kv::Tree ts = e->tree;  // k_hash_legal reads the batch's counts and writes its logits through the tree
        ts.leaf_cnt = e->ar_cnt[x];
        ts.leaf_logits = e->ar_llogits[x];
        return kv::hash_legal(ts, R, st);
    }
    if ((size_t)e->n_ev_used + 2 > e->ev.size()) {
        for (int k = 0; k < 2; ++k) {
            hipEvent_t ev;
            KV_HIP(hipEventCreate(&ev));
            e->ev.push_back(ev);
        }
    }
    kv::net_set_res_events(net, e->ev[e->n_ev_used], e->ev[e->n_ev_used + 1]);
    e->n_ev_used += 2;
    const int rc = leaf ? kv::net_forward_boards_legal_internal(net, e->ar_boards[x], R, e->ar_moves[x], e->ar_cnt[x],
                                                                kv::MAXM, e->ar_llogits[x], e->ar_values[x], st)
                        : kv::net_forward_boards_internal(net, e->ar_boards[x], R, e->ar_rlogits[x], e->ar_values[x],
                                                          st);
    kv::net_set_res_events(net, nullptr, nullptr);
    kv::net_dom_info(net, &e->dom_algo, &e->dom_launches, &e->dom_flop, &e->dom_path, &e->dom_split, &e->dom_kernel);
    return rc;
}

// One ply's roots and sim-steps of an arena (kv_config.arena, DESIGN.md "Arena"). k_arena_split partitions the
// active slots by the net of their mover; the host reads the two counts (the ply's one readback) and sizes each
// player's batch: n_x rows, padded to 17 above 16 slots. The root rows and every sim-step's leaf rows go through the
// two lists, gathered per list and scattered back to the slots' rows, so root, select, backup and choose are the
// self-play kernels. One group: A's batch, then B's, then one backup + select over all slots. Two groups: A's chain
// (gather, forward, scatter, backup + select over A's list) on the engine stream and B's on the group stream, forked
// and joined once per ply, both nets sizing their GEMM grids for half the CUs; with one list empty the ply runs as
// one group. Every slot's tree, leaf row and value are its own and every row is bit-identical inside its batch
// class, so the two forms give the same bytes.
static int eng_arena_ply(kv_engine* e, int act) {
    const kv::Tree& t = e->tree;
    const int S = e->cfg.slots, sims = e->dc.sims;
    int rc = KV_OK;
    hipLaunchKernelGGL(kv::k_arena_split, dim3(1), dim3(1024), 0, e->st, e->dc, e->slots, act, S > 16 ? 17 : 0,
                       e->ar_list[0], e->ar_list[1], e->ar_row_of, e->ctr);
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(e->ctr_host->arena_n, e->ctr->arena_n, 2 * sizeof(int), hipMemcpyDeviceToHost, e->st));
    KV_HIP(hipStreamSynchronize(e->st));
    int n[2], R[2];
    for (int x = 0; x < 2; ++x) {
        n[x] = e->ctr_host->arena_n[x];
        R[x] = S > 16 && n[x] > 0 && n[x] < 17 ? 17 : n[x];
    }
    KV_REQUIRE(n[0] >= 0 && n[1] >= 0 && n[0] + n[1] <= act, KV_EHIP,
               "kv_run: arena lists of %d + %d slots, %d active", n[0], n[1], act);
    for (int x = 0; x < 2; ++x) {  // the root rows, each on its mover's net
        if (n[x] == 0) continue;
        hipLaunchKernelGGL(kv::k_arena_gather_roots, dim3(R[x]), dim3(64), 0, e->st, e->ar_list[x], e->boards,
                           e->ar_boards[x]);
        KV_HIP(hipGetLastError());
        if ((rc = arena_eval(e, x, R[x], false, e->st))) return rc;
        hipLaunchKernelGGL(kv::k_arena_scatter_roots, dim3(R[x]), dim3(256), 0, e->st, e->ar_list[x], e->ar_row_of,
                           e->ar_rlogits[x], e->ar_values[x], e->logits, e->values);
        KV_HIP(hipGetLastError());
    }
    if ((rc = kv::mcts_root(e->dc, t, e->slots, e->moves, e->logits, e->values, e->probs, e->np_mt, e->ctr, e->st)))
        return rc;
    if ((rc = kv::mcts_select(e->dc, t, e->slots, e->boards, e->nn_boards, e->ctr, e->st, 0, S))) return rc;
    const bool two = e->groups == 2 && n[0] > 0 && n[1] > 0;
    if (two) {
        kv::net_set_cu_share(e->net, 2);
        kv::net_set_cu_share(e->net_b, 2);
        KV_HIP(hipEventRecord(e->g_fork, e->st));
        KV_HIP(hipStreamWaitEvent(e->g_st, e->g_fork, 0));
    }
    for (int k = 0; k < sims && !rc; ++k) {
        for (int x = 0; x < 2 && !rc; ++x) {
            if (n[x] == 0) continue;
            hipStream_t st = two && x ? e->g_st : e->st;
            hipLaunchKernelGGL(kv::k_gather_leaves, dim3(R[x]), dim3(64), 0, st, e->ar_list[x], e->nn_boards,
                               t.leaf_moves, t.leaf_cnt, e->ar_boards[x], e->ar_moves[x], e->ar_cnt[x]);
            if (hipGetLastError() != hipSuccess) rc = KV_EHIP;
            if (!rc) rc = arena_eval(e, x, R[x], true, st);
            if (rc) break;
            hipLaunchKernelGGL(kv::k_scatter_leaves, dim3(R[x]), dim3(64), 0, st, e->ar_list[x], e->ar_row_of,
                               e->ar_llogits[x], e->ar_values[x], e->ar_cnt[x], t.leaf_logits, e->values);
            if (hipGetLastError() != hipSuccess) rc = KV_EHIP;
            if (rc) break;
            e->arena_rows[x] += R[x];
            e->mc_rows += R[x];
            if (two)
                rc = k + 1 < sims ? kv::mcts_backup_select(e->dc, t, e->slots, e->boards, e->logits, e->values, e->probs,
                                                           e->nn_boards, e->ctr, st, 0, n[x], false, e->ar_list[x])
                                  : kv::mcts_backup(e->dc, t, e->slots, e->logits, e->values, e->probs, e->ctr, st, 0,
                                                    n[x], false, e->ar_list[x]);
        }
        if (!two && !rc)
            rc = k + 1 < sims ? kv::mcts_backup_select(e->dc, t, e->slots, e->boards, e->logits, e->values, e->probs,
                                                       e->nn_boards, e->ctr, e->st, 0, S)
                              : kv::mcts_backup(e->dc, t, e->slots, e->logits, e->values, e->probs, e->ctr, e->st, 0, S);
    }
    if (two) {
        kv::net_set_cu_share(e->net, 1);
        kv::net_set_cu_share(e->net_b, 1);
        // the join is enqueued on every exit, so that the engine stream never runs ahead of the group stream
        const hipError_t j0 = hipEventRecord(e->g_join, e->g_st);
        const hipError_t j1 = hipStreamWaitEvent(e->st, e->g_join, 0);
        if (rc) return rc;
        KV_HIP(j0);
        KV_HIP(j1);
    }
    return rc;
}

// one network pass of a dense leaf batch (kv_config.leaves > 1): player x's net (or the hash test evaluator, B's
// value negated) over the R rows of list x, the leaves' legal logits only
static int leaves_eval(kv_engine* e, int x, int R) {
    kv_net* net = x ? e->net_b : e->net;
    if (e->dc.eval_mode == KV_EVAL_HASH) {
        int rc = kv::hash_eval(e->lf_boards[x], R, e->lf_hlogits, e->lf_values[x], e->st, x == 1);
        if (rc) return rc;
        kv::Tree ts = e->tree;  // k_hash_legal reads the batch's counts and writes its logits through the tree
        ts.leaf_cnt = e->lf_cnt[x];
        ts.leaf_logits = e->lf_logits[x];
        return kv::hash_legal(ts, R, e->st);
    }
    if ((size_t)e->n_ev_used + 2 > e->ev.size()) {
        for (int k = 0; k < 2; ++k) {
            hipEvent_t ev;
            KV_HIP(hipEventCreate(&ev));
            e->ev.push_back(ev);
        }
    }
    kv::net_set_res_events(net, e->ev[e->n_ev_used], e->ev[e->n_ev_used + 1]);
    e->n_ev_used += 2;
    const int rc = kv::net_forward_boards_legal_internal(net, e->lf_boards[x], R, e->lf_moves[x], e->lf_cnt[x], kv::MAXM,
                                                         e->lf_logits[x], e->lf_values[x], e->st);
    kv::net_set_res_events(net, nullptr, nullptr);
    kv::net_dom_info(net, &e->dom_algo, &e->dom_launches, &e->dom_flop, &e->dom_path, &e->dom_split, &e->dom_kernel);
    return rc;
}

// One ply's roots and sim-steps with kv_config.leaves > 1 (DESIGN.md "Several leaves per game in self-play"),
// self-play and arena alike, on the engine stream. The roots are the one-leaf engines': the slots' rows (self-play;
// kv_run has run them) or the two players' lists (eng_arena_ply's root section), then k_mcts_root. A sim-step is
// select (fused with the backup before it) -> k_leaves_compact -> the host reads the step's counters -> per
// player gather, forward, scatter of its pending rows, sized from the count and padded to 17 rows in the > 16-row
// class, none for an empty list -> backup. The ply ends when no slot's root holds fewer than sims backups.
// kv_config.eval_cache adds two launches to a step: the probe before k_leaves_compact (a row the cache answers has
// its logits and value and stays out of the lists) and, where a list ran, the store of the missed rows after the
// scatter.
static int eng_leaves_ply(kv_engine* e, int act) {
    const kv::Tree& t = e->tree;
    const kv::SearchWs& w = e->lw;
    const int S = e->cfg.slots, L = e->leaves, sims = e->dc.sims, rows = S * L, np = e->cfg.arena ? 2 : 1;
    const int pad_to = e->big ? 17 : 0;
    const bool cache = e->ec_tab[0].ent != nullptr;
    const kv::CacheTab& ec_b = e->ec_tab[e->cfg.arena ? 1 : 0];
    const kv::Slot* ec_slots = e->cfg.arena ? e->slots : nullptr;
    int rc = KV_OK;
    if (cache && e->ec_claims_out) {  // a sim-step failed between its probe and its store
        for (int x = 0; x < np; ++x)
            if ((rc = kv::cache_reset_claims(e->ec_tab[x], e->st))) return rc;
        e->ec_claims_out = false;
    }
    if (e->cfg.arena) {
        hipLaunchKernelGGL(kv::k_arena_split, dim3(1), dim3(1024), 0, e->st, e->dc, e->slots, act, pad_to,
                           e->ar_list[0], e->ar_list[1], e->ar_row_of, e->ctr);
        KV_HIP(hipGetLastError());
        KV_HIP(hipMemcpyAsync(e->ctr_host->arena_n, e->ctr->arena_n, 2 * sizeof(int), hipMemcpyDeviceToHost, e->st));
        KV_HIP(hipStreamSynchronize(e->st));
        for (int x = 0; x < 2; ++x) {  // the root rows, each on its mover's net
            const int n = e->ctr_host->arena_n[x];
            KV_REQUIRE(n >= 0 && n <= act, KV_EHIP, "kv_run: an arena list of %d slots, %d active", n, act);
            if (n == 0) continue;
            const int R = n < pad_to ? pad_to : n;
            hipLaunchKernelGGL(kv::k_arena_gather_roots, dim3(R), dim3(64), 0, e->st, e->ar_list[x], e->boards,
                               e->ar_boards[x]);
            KV_HIP(hipGetLastError());
            if ((rc = arena_eval(e, x, R, false, e->st))) return rc;
            hipLaunchKernelGGL(kv::k_arena_scatter_roots, dim3(R), dim3(256), 0, e->st, e->ar_list[x], e->ar_row_of,
                               e->ar_rlogits[x], e->ar_values[x], e->logits, e->values);
            KV_HIP(hipGetLastError());
        }
    }
    if ((rc = kv::mcts_root(e->dc, t, e->slots, e->moves, e->logits, e->values, e->probs, e->np_mt, e->ctr, e->st)))
        return rc;
    if ((rc = kv::leaves_select(t, w, e->slots, e->boards, e->ctr, sims, S, L, e->st))) return rc;
    for (int step = 0;; ++step) {
        // every step backs up at least one descent of every slot that is still searching: at most sims steps
        KV_REQUIRE(step < sims, KV_EHIP, "kv_run: %d sim-steps without finishing a ply of %d sims", step, sims);
        if (cache) {
            e->ec_claims_out = true;
            if ((rc = kv::cache_probe(e->ec_tab[0], ec_b, ec_slots, L, 1, w, rows, e->ec_hit, e->ec_idx, e->ec_ctr,
                                      e->st)))
                return rc;
        }
        hipLaunchKernelGGL(kv::k_leaves_compact, dim3(1), dim3(1024), 0, e->st, e->dc, e->slots, w.ss, w.lcnt, L, sims,
                           e->cfg.arena, std::max(rows, 17), pad_to, e->lf_list[0],
                           e->lf_list[1] ? e->lf_list[1] : e->lf_list[0], e->lf_row_of, e->lf_ctr, e->ctr,
                           cache ? e->ec_hit : nullptr, (const int*)t.tgt);
        KV_HIP(hipGetLastError());
        KV_HIP(hipMemcpyAsync(e->lf_ctr_host, e->lf_ctr, sizeof(kv::LeafCtr), hipMemcpyDeviceToHost, e->st));
        KV_HIP(hipStreamSynchronize(e->st));
        const kv::LeafCtr lc = *e->lf_ctr_host;
        if (lc.stepping == 0) {  // (no slot was left to search when the ply began: no row, no claim)
            e->ec_claims_out = false;
            break;
        }
        e->sim_steps += 1;
        for (int x = 0; x < np; ++x) {
            const int n = lc.pend[x];
            KV_REQUIRE(n >= 0 && n <= rows, KV_EHIP, "kv_run: a leaf batch of %d rows, %d slots x %d leaves", n, S, L);
            if (n == 0) continue;  // an empty batch runs no forward
            const int R = n < pad_to ? pad_to : n;
            hipLaunchKernelGGL(kv::k_gather_leaves, dim3(R), dim3(64), 0, e->st, e->lf_list[x], w.lboards, w.lmoves,
                               w.lcnt, e->lf_boards[x], e->lf_moves[x], e->lf_cnt[x]);
            KV_HIP(hipGetLastError());
            if ((rc = leaves_eval(e, x, R))) return rc;
            hipLaunchKernelGGL(kv::k_scatter_leaves, dim3(R), dim3(64), 0, e->st, e->lf_list[x], e->lf_row_of,
                               e->lf_logits[x], e->lf_values[x], e->lf_cnt[x], w.llogits, w.lvalues);
            KV_HIP(hipGetLastError());
            e->mc_rows += R;
            if (e->cfg.arena) e->arena_rows[x] += R;
        }
        if (cache && lc.pend[0] + (np > 1 ? lc.pend[1] : 0) > 0 &&
            (rc = kv::cache_store(e->ec_tab[0], ec_b, ec_slots, L, 1, w, rows, e->ec_hit, e->ec_idx, e->ec_ctr, e->st)))
            return rc;
        e->ec_claims_out = false;  // (a step without a miss took none)
        if ((rc = kv::leaves_backup(t, w, e->slots, e->boards, e->ctr, sims, S, L, lc.remaining > 0, e->st))) return rc;
        if (lc.remaining == 0) break;
    }
    return KV_OK;
}

extern "C" {

int kv_run(kv_engine* e, int64_t max_steps, int64_t stop_after_games) {
    KV_REQUIRE(e && e->loaded, KV_EINVAL, "kv_run: engine has no weights");
    KV_REQUIRE(e->cfg.arena == 0 || e->loaded_b, KV_EINVAL,
               "kv_run: an arena engine needs both weight sets (kv_load_weights_b has not loaded player B's)");
    KV_REQUIRE(e->used != 2, KV_EINVAL,
               "kv_run: this engine has searched positions (kv_search); an engine serves either kv_run or kv_search");
    e->used = 1;
    KV_HIP(hipSetDevice(e->cfg.device));
    const auto t0 = std::chrono::steady_clock::now();
    const int S = e->cfg.slots;
    const bool mcts = e->dc.sims > 0;
    const int check_every = (S >= 64 && stop_after_games < 0 && !mcts) ? 4 : 1;
    int rc = eng_wait_copies(e);
    if (rc) return rc;
    rc = eng_counters(e);
    if (rc) return rc;
    long long done = 0;
    while ((max_steps < 0 || done < max_steps) && e->ctr_host->active > 0 &&
           (stop_after_games < 0 || (int64_t)e->ctr_host->games_count < stop_after_games)) {
        const bool lazy = e->dc.eval_mode == KV_EVAL_LAZY;
        const bool compact = lazy && e->comp_boards != nullptr;  // above 16 slots
        if (lazy && !compact) KV_HIP(hipMemsetAsync(&e->ctr->need_eval, 0, sizeof(int), e->st));
        hipLaunchKernelGGL(kv::k_movegen, dim3(S), dim3(64), 0, e->st, e->dc, e->slots, e->boards,
                           e->moves, e->ctr);
        KV_HIP(hipGetLastError());
        if (e->dc.rows > S)
            hipLaunchKernelGGL(kv::k_flush_rows, dim3(S), dim3(64), 0, e->st, e->dc, e->slots, e->last_board,
                               e->boards);
        bool eval_now = true;
        if (compact) {  // only the consumed rows, as one compact batch (identical outputs)
            hipLaunchKernelGGL(kv::k_compact, dim3(1), dim3(1024), 0, e->st, e->dc, e->slots, e->boards,
                               e->comp_boards, e->row_of, e->ctr);
            KV_HIP(hipGetLastError());
            KV_HIP(hipMemcpyAsync(&e->ctr_host->comp_rows, &e->ctr->comp_rows, sizeof(int), hipMemcpyDeviceToHost,
                                  e->st));
            KV_HIP(hipStreamSynchronize(e->st));
            const int rows = e->ctr_host->comp_rows;
            if (rows > 0 && (rc = eng_eval(e, e->comp_boards, rows))) return rc;
            e->lazy_rows += rows;
            eval_now = false;
        } else if (lazy) {  // evaluate only on the steps whose row the schedule consumes (identical outputs)
            KV_HIP(hipMemcpyAsync(&e->ctr_host->need_eval, &e->ctr->need_eval, sizeof(int), hipMemcpyDeviceToHost,
                                  e->st));
            KV_HIP(hipStreamSynchronize(e->st));
            eval_now = e->ctr_host->need_eval != 0;
        }
        if (e->cfg.arena) eval_now = false;  // the root rows go through the two players' lists (eng_arena_ply)
        if (eval_now && (rc = eng_eval(e, e->boards, e->root_rows))) return rc;
        if (!mcts) {
            hipLaunchKernelGGL(kv::k_sample, dim3(S), dim3(256), 0, e->st, e->dc, e->slots, e->boards, e->moves,
                               e->logits, e->values, e->last_probs, e->np_mt, e->py_mt, e->rec, e->last_board,
                               e->ctr, compact ? (const int*)e->row_of : (const int*)nullptr);
            KV_HIP(hipGetLastError());
        } else {
            const kv::Tree& t = e->tree;
            // fewer active slots than slots (no game left to start): compact leaf batches of the active
            // slots, padded to the network class of the full batch (> 16 boards: at least 17 rows)
            const int act = e->ctr_host->active;
            if (e->leaves > 1) {
                if ((rc = eng_leaves_ply(e, act))) return rc;
            } else if (e->cfg.arena) {
                if ((rc = eng_arena_ply(e, act))) return rc;
                e->sim_steps += e->dc.sims;
            } else if (e->tree.rem) {
                if ((rc = eng_reuse_sims(e, act))) return rc;
            } else {
                const bool comp = e->mc_slot_of != nullptr && act < S;
                const int R = comp ? (S > 16 ? std::max(act, 17) : act) : S;
                e->sim_steps += e->dc.sims;
                if (comp) {
                    hipLaunchKernelGGL(kv::k_compact_active, dim3(1), dim3(1024), 0, e->st, e->dc, e->slots, R,
                                       e->mc_slot_of, e->mc_row_of, e->ctr, (const kv::NodeRec*)nullptr, 0, 0,
                                       (const int*)nullptr);
                    KV_HIP(hipGetLastError());
                }
                if ((rc = kv::mcts_root(e->dc, t, e->slots, e->moves, e->logits, e->values, e->probs, e->np_mt, e->ctr, e->st)))
                    return rc;
                if ((rc = kv::mcts_select(e->dc, t, e->slots, e->boards, e->nn_boards, e->ctr, e->st, 0, S))) return rc;
                const bool grouped = e->groups == 2 && !comp;  // (a compact batch of the active slots: one group)
                if (grouped && (rc = eng_group_sims(e, 0, e->dc.sims, e->dc.sims, false))) return rc;
                for (int k = grouped ? e->dc.sims : 0; k < e->dc.sims; ++k) {
                    if (comp) {
                        hipLaunchKernelGGL(kv::k_gather_leaves, dim3(R), dim3(64), 0, e->st, e->mc_slot_of, e->nn_boards,
                                           t.leaf_moves, t.leaf_cnt, e->mc_boards, e->mc_moves, e->mc_cnt);
                        KV_HIP(hipGetLastError());
                        if ((rc = eng_eval(e, e->mc_boards, R, true, true))) return rc;
                        hipLaunchKernelGGL(kv::k_scatter_leaves, dim3(R), dim3(64), 0, e->st, e->mc_slot_of,
                                           e->mc_row_of, e->mc_logits, e->mc_values, e->mc_cnt, t.leaf_logits,
                                           e->values);
                        KV_HIP(hipGetLastError());
                        e->mc_rows += R;
                    } else if ((rc = eng_eval(e, e->nn_boards, S, true))) {
                        return rc;
                    } else {
                        e->full_rows += S;
                    }
                    rc = k + 1 < e->dc.sims
                             ? kv::mcts_backup_select(e->dc, t, e->slots, e->boards, e->logits, e->values, e->probs,
                                                      e->nn_boards, e->ctr, e->st, 0, S)
                             : kv::mcts_backup(e->dc, t, e->slots, e->logits, e->values, e->probs, e->ctr, e->st, 0, S);
                    if (rc) return rc;
                }
            }
            if ((rc = kv::mcts_choose(e->dc, t, e->slots, e->boards, e->py_mt, e->rec, e->last_board, e->ctr,
                                      e->st)))
                return rc;
        }
        hipLaunchKernelGGL(kv::k_finish, dim3(S), dim3(128), 0, e->st, e->dc, e->slots, e->boards,
                           e->moves, e->np_mt, e->py_mt, e->games, e->ctr);
        KV_HIP(hipGetLastError());
        if (e->tree.rem && (rc = e->cfg.reuse_tree ? kv::mcts_carry(e->dc, e->tree, e->slots, e->ctr, e->st)
                                                   : kv::mcts_targets(e->dc, e->tree, e->slots, e->st)))
            return rc;
        ++done;
        ++e->steps;
        if (done % check_every == 0 || (max_steps >= 0 && done >= max_steps)) {
            if ((rc = eng_counters(e))) return rc;
            if ((rc = eng_collect_timing(e))) return rc;
        }
    }
    if ((rc = eng_counters(e))) return rc;
    if ((rc = eng_collect_timing(e))) return rc;
    e->wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return KV_OK;
}

}  // extern "C"

// ------------------------------------------------------ position search --
// (re)allocate a search buffer; the stream is idle when this runs
template <class T>
static int search_alloc(T*& p, size_t count, bool zero = false) {
    if (p) (void)hipFree(p);
    p = nullptr;
    const hipError_t er = hipMalloc(&p, count * sizeof(T));
    if (er != hipSuccess) {
        p = nullptr;
        kv::set_error("kv_search: hipMalloc (%zu B): %s", count * sizeof(T), hipGetErrorString(er));
        return KV_ENOMEM;
    }
    if (zero) KV_HIP(hipMemset(p, 0, count * sizeof(T)));
    return KV_OK;
}

// the workspaces of a search over n positions with L leaves in flight: reserved at the first search that asks
// for them, only grown
static int search_reserve(kv_engine* e, int n, int L) {
    const size_t S = (size_t)e->cfg.slots, RR = std::max<size_t>(S, 17), rows = (size_t)n * L;
    const bool hash = e->dc.eval_mode == KV_EVAL_HASH;
    kv::SearchWs& w = e->sw;
    kv::Tree& t = e->tree;
    int rc = KV_OK;
    const bool grow = rows > e->sw_rows, grow_h = hash && rows > e->s_hrows;
    if (w.ss && !grow && !grow_h && (L == 1 || t.e_V)) return KV_OK;
    KV_HIP(hipStreamSynchronize(e->st));
    if (!w.ss) {
        if ((rc = search_alloc(w.ss, S)) || (rc = search_alloc(w.remaining, 1)) || (rc = search_alloc(w.res, S)) ||
            (rc = search_alloc(e->s_states, S * 80)) || (rc = search_alloc(e->s_rboards, RR * 64, true)) ||
            (rc = search_alloc(e->s_rlogits, RR * 4096)) || (rc = search_alloc(e->s_rvalues, RR)) ||
            (rc = search_alloc(w.sess, S, true)) || (rc = search_alloc(e->s_edge, S)))
            return rc;
        if (hipHostMalloc(&e->s_rem_host, sizeof(int)) != hipSuccess) {
            e->s_rem_host = nullptr;
            kv::set_error("kv_search: hipHostMalloc failed");
            return KV_ENOMEM;
        }
    }
    if (grow) {
        e->sw_rows = 0;
        // lboards zeroed: a row no leaf was written to yet is still a board the network can read
        if ((rc = search_alloc(w.lf, rows)) || (rc = search_alloc(w.paths, rows * (size_t)t.ncap)) ||
            (rc = search_alloc(w.lboards, rows * 64, true)) || (rc = search_alloc(w.lmoves, rows * kv::MAXM)) ||
            (rc = search_alloc(w.lcnt, rows, true)) || (rc = search_alloc(w.llogits, rows * kv::MAXM)) ||
            (rc = search_alloc(w.lvalues, rows)))
            return rc;
        e->sw_rows = rows;
    }
    if (grow_h) {
        e->s_hrows = 0;
        if ((rc = search_alloc(e->s_hlogits, rows * 4096))) return rc;
        e->s_hrows = rows;
    }
    if (L > 1 && !t.e_V && (rc = search_alloc(t.e_V, S * (size_t)t.ecap, true))) return rc;
    return KV_OK;
}

// the session of a finished kv_search / kv_search_continue: what the host keeps of every root
static void session_note(kv_engine* e, const kv_search_result* out, int n) {
    e->sess_host.assign(n, kv::SessionSlot{});
    e->sess_done.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        e->sess_host[i].status = out[i].status;
        e->sess_host[i].n_moves = out[i].n_moves;
        e->sess_done[i] = out[i].status == kv::SR_SEARCHED ? out[i].sims : 0;
    }
    e->sess_n = n;
}

// one network pass of a search (or the hash test evaluator): the root rows, or the step's leaf batch with
// only the leaves' legal logits (kv_net_forward_boards_legal)
static int search_eval(kv_engine* e, const int8_t* boards, int rows, bool leaf) {
    const kv::SearchWs& w = e->sw;
    if (e->dc.eval_mode == KV_EVAL_HASH) {
        int rc = kv::hash_eval(boards, rows, leaf ? e->s_hlogits : e->s_rlogits, leaf ? w.lvalues : e->s_rvalues,
                               e->st);
        if (rc || !leaf) return rc;
        kv::Tree lt = e->tree;  // k_hash_legal reads the batch's counts and writes its logits through the tree
        lt.leaf_cnt = w.lcnt;
        lt.leaf_logits = w.llogits;
        return kv::hash_legal(lt, rows, e->st);
    }
    return leaf ? kv::net_forward_boards_legal_internal(e->net, boards, rows, w.lmoves, w.lcnt, kv::MAXM, w.llogits,
                                                        w.lvalues, e->st)
                : kv::net_forward_boards_internal(e->net, boards, rows, e->s_rlogits, e->s_rvalues, e->st);
}

extern "C" {

int kv_search(kv_engine* e, const int8_t* states, int n, const kv_search_params* p, kv_search_result* out) {
    KV_REQUIRE(e && states && p && out, KV_EINVAL, "kv_search: NULL argument");
    KV_REQUIRE(n > 0 && n <= e->cfg.slots, KV_EINVAL, "kv_search: %d positions, the engine holds 1..%d (slots)", n,
               e->cfg.slots);
    KV_REQUIRE(p->leaves >= 1 && p->leaves <= KV_MAX_LEAVES, KV_EINVAL, "kv_search: leaves %d out of range [1, %d]",
               p->leaves, KV_MAX_LEAVES);
    KV_REQUIRE(e->cfg.arena == 0, KV_EINVAL,
               "kv_search: an arena engine plays matches (kv_run); a position search has one network");
    KV_REQUIRE(e->cfg.sims >= 1, KV_EINVAL, "kv_search: the engine was created without tree pools (sims 0)");
    KV_REQUIRE(p->sims >= 1 && p->sims <= e->cfg.sims, KV_EINVAL,
               "kv_search: sims %d out of range [1, %d] (the engine's sims size its tree pools)", p->sims,
               e->cfg.sims);
    KV_REQUIRE(p->alpha >= 2.2250738585072014e-308 && p->alpha < 1.0, KV_EINVAL,
               "kv_search: alpha must be a normal double in (0,1), got %g", p->alpha);
    KV_REQUIRE(p->eps >= 0.0 && p->eps <= 1.0, KV_EINVAL, "kv_search: eps %g out of range [0, 1]", p->eps);
    KV_REQUIRE(e->used != 1, KV_EINVAL,
               "kv_search: this engine has run self-play (kv_run); an engine serves either kv_run or kv_search");
    KV_REQUIRE(e->loaded, KV_EINVAL, "kv_search: engine has no weights");
    for (int i = 0; i < n; ++i) {
        const int8_t* v = states + (size_t)i * 80;
        bool ok = (v[64] == 0 || v[64] == 1) && v[75] >= -1 && v[75] < 8 && v[76] >= -1 && v[76] < 8 &&
                  (v[75] < 0) == (v[76] < 0);
        for (int q = 0; q < 64; ++q) ok = ok && v[q] >= 0 && v[q] <= 12;
        for (int q = 65; q < 69; ++q) ok = ok && v[q] >= 0 && v[q] < 8;
        KV_REQUIRE(ok, KV_EINVAL, "kv_search: position %d is not a state vector (codes 0..12, wtm 0/1, king "
                   "squares 0..7, ep -1..7)", i);
    }
    e->used = 2;
    e->sess_n = 0;  // a new session begins when this search has succeeded
    KV_HIP(hipSetDevice(e->cfg.device));
    const auto t0 = std::chrono::steady_clock::now();
    const int L = p->leaves, rows = n * L;
    int rc = search_reserve(e, n, L);
    if (rc) return rc;
    const kv::SearchWs& w = e->sw;
    kv::Tree ts = e->tree;  // (kv_config.fast_sims is self-play's: a search has one target, its own sims)
    ts.tgt = nullptr;
    if (!e->cfg.reuse_tree) ts.rem = nullptr;
    const kv::Tree& t = ts;
    hipStream_t st = e->st;
    // a search that overflowed a shrunk pool leaves the engine usable: the flag is this search's own
    KV_HIP(hipMemsetAsync(&e->ctr->error, 0, sizeof(int), st));
    KV_HIP(hipMemsetAsync(w.sess, 0, (size_t)n * sizeof(kv::SessionSlot), st));
    KV_HIP(hipMemcpyAsync(e->s_states, states, (size_t)n * 80, hipMemcpyHostToDevice, st));
    if ((rc = kv::search_load(t, w, e->slots, e->boards, e->moves, e->s_rboards, e->np_mt, e->s_states, p->seed, n,
                              L, e->ctr, st)))
        return rc;
    // the network class (<= 16 boards or above) is that of positions x leaves for the whole search: the
    // root batch of a larger class is padded to 17 rows (empty boards past n)
    const int root_rows = rows > 16 ? std::max(n, 17) : n;
    if ((rc = search_eval(e, e->s_rboards, root_rows, false))) return rc;
    kv::DevCfg dc = e->dc;
    dc.slots = n;
    dc.eps = p->eps;
    dc.alpha = p->alpha;
    if ((rc = kv::mcts_root(dc, t, e->slots, e->moves, e->s_rlogits, e->s_rvalues, e->probs, e->np_mt, e->ctr, st)))
        return rc;
    if ((rc = kv::search_select(t, w, e->slots, e->boards, e->ctr, p->sims, n, L, st))) return rc;
    // every step accepts at least one descent per unfinished tree: at most sims steps. With one leaf in
    // flight it accepts exactly one, so the step count is known and the host reads nothing back (kv_run's
    // loop); with more, collisions decide it: one counter per step, trees with done < sims
    const bool counted = L > 1;
    for (int step = 0;; ++step) {
        KV_REQUIRE(step < p->sims, KV_EHIP, "kv_search: %d sim-steps without finishing %d sims", step, p->sims);
        if ((rc = search_eval(e, w.lboards, rows, true))) return rc;
        if (counted) KV_HIP(hipMemsetAsync(w.remaining, 0, sizeof(int), st));
        if ((rc = kv::search_backup_select(t, w, e->slots, e->boards, e->ctr, p->sims, n, L, st))) return rc;
        if (!counted) {
            if (step + 1 == p->sims) break;
            continue;
        }
        KV_HIP(hipMemcpyAsync(e->s_rem_host, w.remaining, sizeof(int), hipMemcpyDeviceToHost, st));
        KV_HIP(hipStreamSynchronize(st));
        if (*e->s_rem_host == 0) break;
    }
    if ((rc = kv::search_result(t, w, e->slots, e->ctr, p->sims, n, false, st))) return rc;
    KV_HIP(hipMemcpyAsync(out, w.res, (size_t)n * sizeof(kv_search_result), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    e->steps += 1;
    e->wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((rc = eng_counters(e))) return rc;
    session_note(e, out, n);
    return KV_OK;
}

int kv_search_advance(kv_engine* e, int n, const int32_t* edge, int8_t* states_out) {
    KV_REQUIRE(e, KV_EINVAL, "kv_search_advance: NULL argument");
    KV_REQUIRE(e->sess_n > 0, KV_EINVAL, "kv_search_advance: no session (kv_search starts one)");
    KV_REQUIRE(edge, KV_EINVAL, "kv_search_advance: NULL argument");
    KV_REQUIRE(n == e->sess_n, KV_EINVAL, "kv_search_advance: %d trees, the session holds %d", n, e->sess_n);
    // checked against the roots the host knows, so that a bad edge changes no tree
    for (int i = 0; i < n; ++i) {
        if (edge[i] < 0) continue;
        const kv::SessionSlot& se = e->sess_host[i];
        KV_REQUIRE(se.status == kv::SR_SEARCHED, KV_EINVAL,
                   "kv_search_advance: edge %d at tree %d, whose root is not searched (status %d)", edge[i], i,
                   se.status);
        KV_REQUIRE(edge[i] < se.n_moves, KV_EINVAL, "kv_search_advance: edge %d at tree %d, whose root has %d moves",
                   edge[i], i, se.n_moves);
    }
    KV_HIP(hipSetDevice(e->cfg.device));
    const kv::SearchWs& w = e->sw;
    hipStream_t st = e->st;
    const int sess_n = e->sess_n;
    e->sess_n = 0;  // back when the advance has succeeded
    KV_HIP(hipMemsetAsync(&e->ctr->error, 0, sizeof(int), st));
    KV_HIP(hipMemcpyAsync(e->s_edge, edge, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    int rc = kv::search_advance(e->tree, w, e->slots, e->boards, e->moves, e->s_rboards, e->s_edge, e->s_states, n,
                                e->ctr, st);
    if (rc) return rc;
    std::vector<kv::SessionSlot> got(n);
    KV_HIP(hipMemcpyAsync(got.data(), w.sess, (size_t)n * sizeof(kv::SessionSlot), hipMemcpyDeviceToHost, st));
    if (states_out) KV_HIP(hipMemcpyAsync(states_out, e->s_states, (size_t)n * 80, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(e->ctr_host, e->ctr, sizeof(kv::Ctr), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    if (e->ctr_host->error) {
        kv::set_error("kv_search_advance: device error flags 0x%x (1: move list overflow; 32: the tree and the "
                      "position after the move disagree)", e->ctr_host->error);
        return e->ctr_host->error & 32 ? KV_EHIP : KV_EOVERFLOW;
    }
    for (int i = 0; i < n; ++i) {
        if (edge[i] < 0) continue;
        e->sess_host[i] = got[i];
        e->sess_done[i] = got[i].kept;
    }
    e->sess_n = sess_n;
    return KV_OK;
}

int kv_search_continue(kv_engine* e, int n, const kv_search_params* p, kv_search_result* out, int32_t* kept) {
    KV_REQUIRE(e, KV_EINVAL, "kv_search_continue: NULL argument");
    KV_REQUIRE(e->sess_n > 0, KV_EINVAL, "kv_search_continue: no session (kv_search starts one)");
    KV_REQUIRE(p && out, KV_EINVAL, "kv_search_continue: NULL argument");
    KV_REQUIRE(n == e->sess_n, KV_EINVAL, "kv_search_continue: %d trees, the session holds %d", n, e->sess_n);
    KV_REQUIRE(p->leaves >= 1 && p->leaves <= KV_MAX_LEAVES, KV_EINVAL,
               "kv_search_continue: leaves %d out of range [1, %d]", p->leaves, KV_MAX_LEAVES);
    KV_REQUIRE(p->sims >= 1 && p->sims <= e->cfg.sims, KV_EINVAL,
               "kv_search_continue: sims %d out of range [1, %d] (the engine's sims size its tree pools)", p->sims,
               e->cfg.sims);
    KV_REQUIRE(p->alpha >= 2.2250738585072014e-308 && p->alpha < 1.0, KV_EINVAL,
               "kv_search_continue: alpha must be a normal double in (0,1), got %g", p->alpha);
    KV_REQUIRE(p->eps == 0.0, KV_EINVAL,
               "kv_search_continue: eps %g, a session's roots take no Dirichlet noise (eps must be 0)", p->eps);
    KV_HIP(hipSetDevice(e->cfg.device));
    const auto t0 = std::chrono::steady_clock::now();
    const int L = p->leaves, rows = n * L;
    const int sess_n = e->sess_n;
    e->sess_n = 0;  // back when the call has succeeded
    int rc = search_reserve(e, n, L);
    if (rc) return rc;
    const kv::SearchWs& w = e->sw;
    kv::Tree ts = e->tree;  // (kv_config.fast_sims is self-play's: a search has one target, its own sims)
    ts.tgt = nullptr;
    if (!e->cfg.reuse_tree) ts.rem = nullptr;
    const kv::Tree& t = ts;
    hipStream_t st = e->st;
    // what the host knows of the roots: the dropped trees take a root row, the longest top-up bounds the steps
    bool any_fresh = false;
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        const kv::SessionSlot& se = e->sess_host[i];
        if (se.status != kv::SR_SEARCHED) continue;
        any_fresh = any_fresh || se.fresh;
        longest = std::max(longest, p->sims - (se.fresh ? 0 : e->sess_done[i]));
        if (kept) kept[i] = se.fresh ? 0 : e->sess_done[i];
    }
    if (kept)
        for (int i = 0; i < n; ++i)
            if (e->sess_host[i].status != kv::SR_SEARCHED) kept[i] = 0;
    KV_HIP(hipMemsetAsync(&e->ctr->error, 0, sizeof(int), st));
    if ((rc = kv::search_resume(t, w, e->slots, e->np_mt, p->seed, n, L, st))) return rc;
    if (any_fresh) {
        // k_mcts_root on the dropped trees' rows, in the batch class of the whole call (kv_search)
        const int root_rows = rows > 16 ? std::max(n, 17) : n;
        if ((rc = search_eval(e, e->s_rboards, root_rows, false))) return rc;
        kv::DevCfg dc = e->dc;
        dc.slots = n;
        dc.eps = 0.0;
        dc.alpha = p->alpha;
        if ((rc = kv::mcts_root(dc, t, e->slots, e->moves, e->s_rlogits, e->s_rvalues, e->probs, e->np_mt, e->ctr,
                                st)))
            return rc;
    }
    if (longest > 0) {
        if ((rc = kv::search_select(t, w, e->slots, e->boards, e->ctr, p->sims, n, L, st))) return rc;
        const bool counted = L > 1;  // kv_search's loop; with one leaf the longest top-up is the step count
        for (int step = 0;; ++step) {
            KV_REQUIRE(step < longest, KV_EHIP, "kv_search_continue: %d sim-steps without finishing %d sims", step,
                       p->sims);
            if ((rc = search_eval(e, w.lboards, rows, true))) return rc;
            if (counted) KV_HIP(hipMemsetAsync(w.remaining, 0, sizeof(int), st));
            if ((rc = kv::search_backup_select(t, w, e->slots, e->boards, e->ctr, p->sims, n, L, st))) return rc;
            if (!counted) {
                if (step + 1 == longest) break;
                continue;
            }
            KV_HIP(hipMemcpyAsync(e->s_rem_host, w.remaining, sizeof(int), hipMemcpyDeviceToHost, st));
            KV_HIP(hipStreamSynchronize(st));
            if (*e->s_rem_host == 0) break;
        }
    }
    if ((rc = kv::search_result(t, w, e->slots, e->ctr, p->sims, n, true, st))) return rc;
    KV_HIP(hipMemcpyAsync(out, w.res, (size_t)n * sizeof(kv_search_result), hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    e->steps += 1;
    e->wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((rc = eng_counters(e))) return rc;
    session_note(e, out, sess_n);
    return KV_OK;
}

int kv_search_tree_size(kv_engine* e, int i, int32_t* nodes, int32_t* edges) {
    KV_REQUIRE(e && nodes && edges, KV_EINVAL, "kv_search_tree_size: NULL argument");
    KV_REQUIRE(e->sess_n > 0, KV_EINVAL, "kv_search_tree_size: no session (kv_search starts one)");
    KV_REQUIRE(i >= 0 && i < e->sess_n, KV_EINVAL, "kv_search_tree_size: tree %d, the session holds %d", i,
               e->sess_n);
    *nodes = *edges = 0;
    const kv::SessionSlot& se = e->sess_host[i];
    if (se.status != kv::SR_SEARCHED || se.fresh) return KV_OK;  // no tree (yet)
    KV_HIP(hipSetDevice(e->cfg.device));
    kv::MctsSlot m;
    KV_HIP(hipMemcpyAsync(&m, e->ms + i, sizeof(m), hipMemcpyDeviceToHost, e->st));
    KV_HIP(hipStreamSynchronize(e->st));
    *nodes = m.node_count;
    *edges = (m.edge_count + 15) & ~15;  // every block counted to its 16-edge boundary
    return KV_OK;
}

size_t kv_sizeof_search_result(void) { return sizeof(kv_search_result); }

int kv_reset_records(kv_engine* e) {
    KV_REQUIRE(e, KV_EINVAL, "kv_reset_records: NULL");
    const int rc = eng_wait_copies(e);
    if (rc) return rc;
    KV_HIP(hipMemsetAsync(&e->ctr->rec_count, 0, sizeof(unsigned long long), e->st));
    KV_HIP(hipStreamSynchronize(e->st));
    return KV_OK;
}

int kv_sync(kv_engine* e) {
    KV_REQUIRE(e, KV_EINVAL, "kv_sync: NULL");
    KV_HIP(hipStreamSynchronize(e->st));
    return KV_OK;
}

int kv_records(kv_engine* e, kv_record* out, size_t cap, size_t* n) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_records: NULL argument");
    int rc = eng_counters(e);
    if (rc) return rc;
    size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_records: buffer holds %zu, need %zu", cap, cnt);
    KV_HIP(hipMemcpy(out, e->rec, cnt * sizeof(kv_record), hipMemcpyDeviceToHost));
    std::stable_sort(out, out + cnt, [](const kv_record& a, const kv_record& b) {
        return a.game_id != b.game_id ? a.game_id < b.game_id : a.ply < b.ply;
    });
    return KV_OK;
}

int kv_records_device(kv_engine* e, kv_record* out_dev, size_t cap, size_t* n, void* stream) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_records_device: NULL argument");
    int rc = eng_counters(e);
    if (rc) return rc;
    const size_t cnt =
        (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out_dev) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_records_device: buffer holds %zu, need %zu", cap, cnt);
    // the engine stream is idle after eng_counters; the copy runs on the caller's stream, and the
    // engine's next write to e->rec waits for it (eng_wait_copies)
    KV_HIP(hipMemcpyAsync(out_dev, e->rec, cnt * sizeof(kv_record), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return eng_note_copy(e, (hipStream_t)stream);
}

int kv_games(kv_engine* e, kv_game* out, size_t cap, size_t* n) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_games: NULL argument");
    int rc = eng_counters(e);
    if (rc) return rc;
    size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->games_count, (unsigned long long)e->dc.games_cap);
    *n = cnt;
    if (!out) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_games: buffer holds %zu, need %zu", cap, cnt);
    KV_HIP(hipMemcpy(out, e->games, cnt * sizeof(kv_game), hipMemcpyDeviceToHost));
    std::sort(out, out + cnt, [](const kv_game& a, const kv_game& b) { return a.game_id < b.game_id; });
    return KV_OK;
}

int kv_stats_get(kv_engine* e, kv_stats* out) {
    KV_REQUIRE(e && out, KV_EINVAL, "kv_stats_get: NULL argument");
    int rc = eng_counters(e, false);  // readable after an error too (tree_overflows)
    if (rc) return rc;
    out->steps = e->steps;
    out->plies = (int64_t)e->ctr_host->plies;
    out->games_done = (int64_t)e->ctr_host->games_count;
    out->nn_rows = (int64_t)(e->ctr_host->nn_rows + e->ctr_host->nn_rows_slots);
    out->sims = (int64_t)e->ctr_host->sims;
    out->records = (int64_t)e->ctr_host->rec_count;
    out->res_conv_ms = e->nn_res_ms;
    out->res_conv_launches = e->nn_res_launches;
    out->step_ms = e->wall_ms;
    out->dom_flop = e->dom_flop;
    out->dom_algo = e->dom_algo;
    out->dom_path = e->dom_path;
    out->dom_split = e->dom_split;
    snprintf(out->dom_kernel, sizeof(out->dom_kernel), "%s", e->dom_kernel ? e->dom_kernel : "");
    out->tree_overflows = (int64_t)e->ctr_host->tree_overflows;
    out->nn_rows_lazy = e->lazy_rows;
    out->sim_steps = e->sim_steps;
    // the MCTS leaf rows k_mcts_choose counted (Ctr::nn_rows; a search engine's are kv_search's own)
    out->leaf_rows_pending = e->used == 1 && e->dc.sims > 0 ? (int64_t)e->ctr_host->nn_rows : 0;
    out->sims_kept = (int64_t)e->ctr_host->sims_kept;
    out->roots_carried = (int64_t)e->ctr_host->roots_carried;
    out->leaf_batch_rows = e->mc_rows + e->full_rows;
    out->plies_fast = (int64_t)e->ctr_host->plies_fast;
    out->plies_full = out->plies - out->plies_fast;
    out->forced_descents = (int64_t)e->ctr_host->forced_descents;
    out->visits_pruned = (int64_t)e->ctr_host->visits_pruned;
    out->arena_rows[0] = e->arena_rows[0];
    out->arena_rows[1] = e->arena_rows[1];
    kv::CacheCtr cc = {0, 0, 0};
    if (e->ec_ctr) KV_HIP(hipMemcpy(&cc, e->ec_ctr, sizeof(cc), hipMemcpyDeviceToHost));  // (eng_counters has synced)
    out->cache_probes = (int64_t)cc.probes;
    out->cache_hits = (int64_t)cc.hits;
    out->cache_stores = (int64_t)cc.stores;
    return KV_OK;
}

size_t kv_sizeof_config(void) { return sizeof(kv_config); }
size_t kv_sizeof_stats(void) { return sizeof(kv_stats); }

// kv_root_visits / kv_root_targets: the per-record count rows of `buf` in kv_records' order, -1 padded
static int root_counts(kv_engine* e, const uint16_t* buf, const char* what, int32_t* out, size_t cap, size_t* n) {
    int rc = eng_counters(e);
    if (rc) return rc;
    const size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "%s: buffer holds %zu records, need %zu", what, cap, cnt);
    std::vector<kv_record> rec(cnt);
    std::vector<uint16_t> vis(cnt * kv::MAXM);
    KV_HIP(hipMemcpy(rec.data(), e->rec, cnt * sizeof(kv_record), hipMemcpyDeviceToHost));
    KV_HIP(hipMemcpy(vis.data(), buf, vis.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    std::vector<size_t> ord(cnt);
    for (size_t k = 0; k < cnt; ++k) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {  // kv_records' order
        return rec[a].game_id != rec[b].game_id ? rec[a].game_id < rec[b].game_id : rec[a].ply < rec[b].ply;
    });
    for (size_t k = 0; k < cnt; ++k)
        for (int j = 0; j < kv::MAXM; ++j) {
            const uint16_t v = vis[ord[k] * kv::MAXM + j];
            out[k * kv::MAXM + j] = v == 0xffff ? -1 : (int32_t)v;
        }
    return KV_OK;
}

int kv_root_visits(kv_engine* e, int32_t* out, size_t cap, size_t* n) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_root_visits: NULL argument");
    KV_REQUIRE(e->tree.root_visits, KV_EINVAL, "kv_root_visits: engine was created without keep_root_visits");
    return root_counts(e, e->tree.root_visits, "kv_root_visits", out, cap, n);
}

int kv_root_targets(kv_engine* e, int32_t* out, size_t cap, size_t* n) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_root_targets: NULL argument");
    KV_REQUIRE(e->tree.root_targets, KV_EINVAL,
               "kv_root_targets: engine was created without forced_k > 0 and keep_root_visits");
    return root_counts(e, e->tree.root_targets, "kv_root_targets", out, cap, n);
}

int kv_root_targets_device(kv_engine* e, uint16_t* out_dev, size_t cap, size_t* n, void* stream) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_root_targets_device: NULL argument");
    KV_REQUIRE(e->tree.root_targets, KV_EINVAL,
               "kv_root_targets_device: engine was created without forced_k > 0 and keep_root_visits");
    int rc = eng_counters(e);
    if (rc) return rc;
    const size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out_dev) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_root_targets_device: buffer holds %zu records, need %zu", cap, cnt);
    KV_HIP(hipMemcpyAsync(out_dev, e->tree.root_targets, cnt * kv::MAXM * sizeof(uint16_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return eng_note_copy(e, (hipStream_t)stream);
}

int kv_root_visits_device(kv_engine* e, uint16_t* out_dev, size_t cap, size_t* n, void* stream) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_root_visits_device: NULL argument");
    KV_REQUIRE(e->tree.root_visits, KV_EINVAL, "kv_root_visits_device: engine was created without keep_root_visits");
    int rc = eng_counters(e);
    if (rc) return rc;
    const size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out_dev) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_root_visits_device: buffer holds %zu records, need %zu", cap, cnt);
    KV_HIP(hipMemcpyAsync(out_dev, e->tree.root_visits, cnt * kv::MAXM * sizeof(uint16_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return eng_note_copy(e, (hipStream_t)stream);
}

int kv_root_moves(kv_engine* e, uint16_t* out, size_t cap, size_t* n) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_root_moves: NULL argument");
    KV_REQUIRE(e->tree.root_moves, KV_EINVAL, "kv_root_moves: engine was created without keep_root_visits = 2");
    int rc = eng_counters(e);
    if (rc) return rc;
    const size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_root_moves: buffer holds %zu records, need %zu", cap, cnt);
    std::vector<kv_record> rec(cnt);
    std::vector<uint16_t> mv(cnt * kv::MAXM);
    KV_HIP(hipMemcpy(rec.data(), e->rec, cnt * sizeof(kv_record), hipMemcpyDeviceToHost));
    KV_HIP(hipMemcpy(mv.data(), e->tree.root_moves, mv.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    std::vector<size_t> ord(cnt);
    for (size_t k = 0; k < cnt; ++k) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {  // kv_records' order, as kv_root_visits
        return rec[a].game_id != rec[b].game_id ? rec[a].game_id < rec[b].game_id : rec[a].ply < rec[b].ply;
    });
    for (size_t k = 0; k < cnt; ++k)
        memcpy(out + k * kv::MAXM, mv.data() + ord[k] * kv::MAXM, kv::MAXM * sizeof(uint16_t));
    return KV_OK;
}

int kv_root_moves_device(kv_engine* e, uint16_t* out_dev, size_t cap, size_t* n, void* stream) {
    KV_REQUIRE(e && n, KV_EINVAL, "kv_root_moves_device: NULL argument");
    KV_REQUIRE(e->tree.root_moves, KV_EINVAL,
               "kv_root_moves_device: engine was created without keep_root_visits = 2");
    int rc = eng_counters(e);
    if (rc) return rc;
    const size_t cnt = (size_t)std::min<unsigned long long>(e->ctr_host->rec_count, (unsigned long long)e->cfg.record_cap);
    *n = cnt;
    if (!out_dev) return KV_OK;
    KV_REQUIRE(cap >= cnt, KV_EINVAL, "kv_root_moves_device: buffer holds %zu records, need %zu", cap, cnt);
    KV_HIP(hipMemcpyAsync(out_dev, e->tree.root_moves, cnt * kv::MAXM * sizeof(uint16_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return eng_note_copy(e, (hipStream_t)stream);
}

void kv_destroy(kv_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    if (e->copy_pending) (void)hipEventSynchronize(e->copy_done);  // a caller-stream copy out of e->rec
    if (e->st) (void)hipStreamSynchronize(e->st);
    kv::Tree& t = e->tree;
    void* bufs[] = {e->slots, e->boards, e->moves, e->logits, e->values, e->last_probs, e->comp_boards, e->row_of,
                    e->np_mt, e->py_mt, e->rec, e->games, e->last_board, e->ctr,
                    t.e_move, t.e_P, t.e_N, t.e_W, t.e_child, t.node, t.path,
                    t.leaf_moves, e->ms, e->nn_boards, e->probs, e->sqrt_tab, t.root_visits, t.leaf_cnt,
                    t.leaf_logits, e->mc_slot_of, e->mc_row_of, e->mc_boards, e->mc_moves, e->mc_cnt,
                    e->mc_logits, e->mc_values,
                    t.e_V, e->sw.ss, e->sw.lf, e->sw.paths, e->sw.lboards, e->sw.lmoves, e->sw.lcnt, e->sw.llogits,
                    e->sw.lvalues, e->sw.remaining, e->sw.res, e->s_states, e->s_rboards, e->s_rlogits,
                    e->s_rvalues, e->s_hlogits, e->sw.sess, e->s_edge, t.root_moves, t.rem, t.tgt, t.forced, t.root_targets,
                    e->ar_row_of, e->ar_list[0], e->ar_list[1], e->ar_boards[0], e->ar_boards[1], e->ar_moves[0],
                    e->ar_moves[1], e->ar_cnt[0], e->ar_cnt[1], e->ar_llogits[0], e->ar_llogits[1], e->ar_values[0],
                    e->ar_values[1], e->ar_rlogits[0], e->ar_rlogits[1],
                    e->lw.ss, e->lw.lf, e->lw.paths, e->lw.lboards, e->lw.lmoves, e->lw.lcnt, e->lw.llogits,
                    e->lw.lvalues, e->lf_list[0], e->lf_list[1], e->lf_row_of, e->lf_boards[0], e->lf_boards[1],
                    e->lf_moves[0], e->lf_moves[1], e->lf_cnt[0], e->lf_cnt[1], e->lf_logits[0], e->lf_logits[1],
                    e->lf_values[0], e->lf_values[1], e->lf_hlogits, e->lf_ctr,
                    e->ec_tab[0].ent, e->ec_tab[0].claim, e->ec_tab[1].ent, e->ec_tab[1].claim, e->ec_hit, e->ec_idx,
                    e->ec_ctr, e->starts};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (e->ctr_host) (void)hipHostFree(e->ctr_host);
    if (e->s_rem_host) (void)hipHostFree(e->s_rem_host);
    if (e->rem_host) (void)hipHostFree(e->rem_host);
    if (e->lf_ctr_host) (void)hipHostFree(e->lf_ctr_host);
    for (auto x : e->ev) (void)hipEventDestroy(x);
    if (e->copy_done) (void)hipEventDestroy(e->copy_done);
    if (e->g_st) (void)hipStreamSynchronize(e->g_st);
    kv::net_view_destroy(e->g_net);
    if (e->net_b) kv_net_destroy(e->net_b);
    if (e->net) kv_net_destroy(e->net);
    if (e->g_fork) (void)hipEventDestroy(e->g_fork);
    if (e->g_join) (void)hipEventDestroy(e->g_join);
    if (e->g_st) (void)hipStreamDestroy(e->g_st);
    if (e->st) (void)hipStreamDestroy(e->st);
    delete e;
}

}  // extern "C"
