/*
 * kv.h -- C ABI of libkv.so, the MI355X-native self-play engine that drops in
 * under the reference's self-play data-generation path.
 *
 * The reference has no native boundary: its callers bind Python names
 * (SURVEY.md 8b). Each entry point below replaces one of those names; the
 * Python mirror in knightvision_amd/ (same names, argument meaning and error
 * behaviour) binds them with ctypes, see INTEGRATION.md.
 *
 * Conventions: every call returns int status (0 ok, negative KV_E*); the text
 * of the last error is kv_last_error(). Pointers named *_dev are HIP device
 * pointers, everything else is host memory owned by the caller. `stream` is a
 * hipStream_t passed as void* (NULL = the default stream). An engine or net
 * is not re-entrant: one host thread per object / GPU.
 */
#ifndef KV_H
#define KV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KV_OK 0
#define KV_EINVAL -1
#define KV_ENOMEM -2
#define KV_EHIP -3
#define KV_EOVERFLOW -4

const char* kv_last_error(void);
int kv_version(void);

/* ------------------------------------------------------------------ NN ---
 * ChessNet forward (replaces ai/model.py:51-77 ChessNet.forward).
 * Packed weights: BN folded into per-channel scale/shift; layout produced by
 * knightvision_amd/weights.py:pack_weights and re-derived by kv_net_packed_size
 * (each tensor padded to a multiple of 16 floats):
 *   12 convs, each: w[Cout][9][CinPad], scale[Cout], shift[Cout]
 *     (conv1 12->256 CinPad 16, conv2 256->512, 10 residual convs 512->512)
 *   head.w[3][512] head.scale[3] head.shift[3]   (policy_conv x2, value_conv)
 *   pfc.w[4096][128] pfc.b[4096] vfc1.w[512][64] vfc1.b[512] vfc2.w[512] vfc2.b[1]
 */
typedef struct kv_net kv_net;

size_t kv_net_packed_size(void);
int kv_net_create(int device, kv_net** out);
int kv_net_load(kv_net* net, const float* packed, size_t n_floats);
/* planes_dev: [B][12][8][8] fp32 (encode_board layout, ai/ai.py:17-30);
 * policy_dev: [B][4096] logits; value_dev: [B] tanh value. Any B >= 1: a batch of more than 16,384
 * boards (the tower's 32-bit workspace offsets) runs as equal slices of at most 16,384, each in the same
 * size class (> 16 boards) as the whole batch, so every output is the one a single pass would give. The same
 * holds for the two board-code forwards below. */
int kv_net_forward(kv_net* net, const float* planes_dev, int B, float* policy_dev, float* value_dev, void* stream);
/* boards_dev: [B][64] int8 piece codes (0 empty, 1..6 wK wQ wR wB wN wp,
 * 7..12 bK bQ bR bB bN bp; square r*8+c, row 0 = rank 8). */
int kv_net_forward_boards(kv_net* net, const int8_t* boards_dev, int B, float* policy_dev, float* value_dev,
                          void* stream);
/* The same forward with only the listed moves' logits (the MCTS leaves' legal
 * moves): moves_dev [B][maxm] move words (from | to << 6, as kv_dev_valid_moves),
 * n_moves_dev [B] (0: no logits for that board; values above maxm are read as
 * maxm -- a row holds maxm moves); legal_dev [B][maxm] receives
 * policy logit (from*64 + to) of each listed move, bit-identical to the
 * corresponding entry of kv_net_forward_boards; value_dev [B]. */
int kv_net_forward_boards_legal(kv_net* net, const int8_t* boards_dev, int B, const uint16_t* moves_dev,
                                const int* n_moves_dev, int maxm, float* legal_dev, float* value_dev, void* stream);
/* per-launch timing of the last forward (HIP events on `stream`): ms of the
 * residual conv launches summed, and count of those launches. */
int kv_net_last_timing(kv_net* net, float* conv_ms, int* n_conv);
/* Arithmetic of the 3x3 convs with Cin 256/512 (the stem conv, the heads and
 * the activations between layers are fp32 in every mode):
 * KV_PREC_FP32   fp32 (default; the parity mode). Under KV_ALGO_AUTO the net
 *                picks its conv path per weight load by measuring the
 *                candidates against an fp64 forward (kv_net_calibration).
 * KV_PREC_F64W   Winograd F(8x8) with every Winograd-domain quantity (U, V, M,
 *                transforms) in fp64, on v_mfma_f64_16x16x4_f64, at every batch
 *                size: logits within ~3e-6 of an fp64 forward on every weight set
 *                measured.
 * KV_PREC_I8X5   the same fp64 Winograd domain with the GEMMs on the int8
 *                matrix cores: every V / U row scaled by a power of two and
 *                split into 5 int8 digits, the 15 digit products of weight
 *                >= 2^-28 accumulated exactly in int32 and combined in fp64
 *                (per-row 35-bit block fixed point, 15 of 25 digit pairs: within
 *                ~2^-36 of the fp64 product per element); logits
 *                as close to fp64 as KV_PREC_F64W's, at every batch size (the
 *                fp32 AUTO fallback for trained weights before F64W).
 * KV_PREC_I8R4   the same fp64 domain with 4 radix-256 digits per value
 *                (31-bit block fixed point: N = rint(a 2^(31-e)) split into
 *                balanced bytes) and the 13 digit pairs i + j <= 4 of 16:
 *                13 int8 GEMMs instead of 15 over 4 digit planes instead of
 *                5 (AUTO's candidate before KV_PREC_I8X5).
 * Values 1 and 2 (bf16x3 / bf16x6) were retired in round 4, 3 (f16x3: F(4x8) GEMMs on fp16 MFMA with both
 * operands split in two fp16 pieces) in round 6 -- no configuration chose them: KV_EINVAL. */
#define KV_PREC_FP32 0
#define KV_PREC_F64W 4
#define KV_PREC_I8X5 5
#define KV_PREC_I8R4 6
int kv_net_set_precision(kv_net* net, int precision);
/* Algorithm of the fp32 3x3 convs with Cin 256/512:
 * KV_ALGO_AUTO      per weight load, the fastest path whose logits / values are
 *                   within 4e-5 / 4e-6 of an fp64 forward on 64 calibration
 *                   boards (the initial position, 16 positions of reference
 *                   self-play, 47 seeded random ones): > 16 boards F(8x8) fp32
 *                   on 3 radix-256 int8 digits (KV_ALGO_WINOGRAD88_I8R3),
 *                   else on 4 radix-128 ones (KV_ALGO_WINOGRAD88_I8), else the
 *                   same with fp64 input transforms (KV_ALGO_WINOGRAD88_I8V),
 *                   else the fp64 Winograd domain on 4 radix-256 int8
 *                   digits (KV_PREC_I8R4), else on fp64 MFMA; <= 16 boards
 *                   direct (split-K), else F(8x8)
 *                   fp64 (kv_net_calibration reports it)
 * KV_ALGO_DIRECT    implicit GEMM over the 9 taps (exact fp32 products)
 * KV_ALGO_WINOGRAD88 F(8x8,3x3): 100 GEMMs of 1 tile x Cin x Cout per board,
 *                   5.76x fewer FLOPs than direct (fp32 MFMA)
 * KV_ALGO_WINOGRAD88_I8 the F(8x8) fp32 tower (fp32 U, V, M, transforms) with
 *                   each GEMM on 4 int8 digits per value: per-row 28-bit
 *                   block fixed point, the 10 digit pairs i + j <= 3, exact
 *                   int32 levels, one rounding to fp32, on
 *                   v_mfma_i32_32x32x32_i8
 * KV_ALGO_WINOGRAD88_I8V the same tower with each conv's V the fp64 input
 *                   transform of its fp32 input, cut to 4 digits from fp64
 *                   (M, the output transform and the activations stay fp32)
 * KV_ALGO_WINOGRAD88_I8R3 the fp32 tower of KV_ALGO_WINOGRAD88_I8 with each
 *                   GEMM on 3 radix-256 int8 digits per value: per-row 24-bit
 *                   block fixed point (N = rint(a 2^(23-e)) as balanced
 *                   bytes), the 6 digit pairs i + j <= 2 of 9, exact int32
 *                   levels, one rounding to fp32 -- 6 int8 GEMMs per point
 *                   instead of 10 (AUTO's first candidate)
 * Values 2 (F(4x4)) and 3 (F(4x8)) were retired in rounds 4 and 6: KV_EINVAL. Setting the precision or
 * the algorithm of a loaded net re-prepares it (synchronous).
 * Results are batch-invariant inside a class (<= 16 boards, > 16 boards). */
#define KV_ALGO_AUTO 0
#define KV_ALGO_DIRECT 1
#define KV_ALGO_WINOGRAD88 4
#define KV_ALGO_WINOGRAD88_I8 5
#define KV_ALGO_WINOGRAD88_I8V 6
#define KV_ALGO_WINOGRAD88_I8R3 7
int kv_net_set_algo(kv_net* net, int algo);
/* conv paths (what a forward runs) */
#define KV_PATH_DIRECT 0
#define KV_PATH_WINO88 2
#define KV_PATH_WINO88_F64 3
#define KV_PATH_WINO88_I8 5     /* (1 and 4, the retired F(4x8) towers, stay unused indices) */
#define KV_PATH_WINO88_I8F32 6
#define KV_PATH_WINO88_I8F32V 7
#define KV_PATH_WINO88_I8R 8
#define KV_PATH_WINO88_I8F32R3 9
#define KV_NPATH 10
typedef struct {
    int calibrated;      /* 1: the last load / setting ran the fp32 AUTO calibration */
    int path_large;      /* KV_PATH_* of batches > 16 boards (also without calibration) */
    int path_small;      /* KV_PATH_* of batches <= 16 boards */
    int n_boards;        /* calibration boards */
    double tol_logit;    /* budget: max |logit - fp64| */
    double tol_value;    /* budget: max |value - fp64| */
    double err_logit[KV_NPATH]; /* > 16-board candidates measured, per path (-1: not run) */
    double err_value[KV_NPATH];
    double err_small_logit;     /* the <= 16-board direct path on 16 of the boards */
    double err_small_value;
    double ms;                  /* wall time of the calibration */
} kv_calib;
int kv_net_calibration(kv_net* net, kv_calib* out);
int kv_net_set_timing(kv_net* net, int enable);
void kv_net_destroy(kv_net* net);

/* ------------------------------------------------------------- engine ---
 * Self-play engine (replaces scripts/self_play.py self_play :258-291 /
 * _run_single_game :111-255 / _init_worker :52-85 state).
 */
#define KV_SEED_PER_GAME 0   /* game g seeded SEED+g in both streams, no carried eval */
#define KV_SEED_SEQUENTIAL 1 /* one numpy + one CPython stream seeded SEED, games in order */

#define KV_EVAL_FAITHFUL 0 /* every board evaluated once, as the reference does */
#define KV_EVAL_LAZY 1     /* the network runs only on the rows the schedule consumes (reference move
                              selection): <= 16 slots, all slots' rows on the steps where one is
                              consumed (the sequential drop-in path); above, the consumed rows as one
                              compact batch. Identical outputs, ~1/SELFPLAY_BATCH_SIZE of the network
                              work -- the reference evaluates every board and reads one row in 16 */
#define KV_EVAL_HASH 2     /* TEST ONLY: uniform logits + hash value instead of the network */

typedef struct {
    int device;
    int slots;            /* concurrent games on this GPU */
    int64_t n_games;      /* games to play (global ids game_id_base + k*game_id_stride) */
    int64_t game_id_base; /* first global game id on this rank */
    int64_t game_id_stride;
    uint64_t seed;        /* SEED (self_play.py:24) */
    int seed_mode;        /* KV_SEED_* */
    int max_moves;        /* <= 0: None */
    int batch;            /* SELFPLAY_BATCH_SIZE (self_play.py:34) */
    double eps;           /* DIR_NOISE_EPS */
    double alpha;         /* DIR_NOISE_ALPHA, a normal double in (0,1) (numpy's legacy gamma shape < 1
                             branch, restated exactly down to subnormal / zero draws; a ply whose 4096
                             draws are all 0 fails kv_run with KV_EINVAL, as the reference's
                             random.choices raises ValueError on the NaN weights) */
    int sims;             /* 0: reference move selection; 1..KV_MAX_SIMS: PUCT MCTS sims/move */
    float c_puct;
    int eval_mode;        /* KV_EVAL_* */
    int64_t record_cap;   /* record buffer capacity (records, one per committed ply; <= 0: 2^20); a run that
                             fills it fails with KV_EOVERFLOW ("record buffer full"), never a silent drop */
    int recycle;          /* 1: a finished slot starts the next game id */
    int precision;        /* KV_PREC_* of the network convs */
    int algo;             /* KV_ALGO_* of the network convs */
    int tree_edge_cap;    /* MCTS edges per slot; <= 0: KV_MAXM x (sims + 1), which cannot overflow. An
                             expansion that does not fit raises KV_EOVERFLOW (kv_stats.tree_overflows) */
    float forced_k;       /* Forced playouts and policy target pruning (MCTS self-play, DESIGN.md "Forced playouts and
                             policy target pruning"). 0: off (no kernel takes another path, no byte changes). Else
                             0 < forced_k <= 16 (KataGo: 2): on a full ply a root edge with n > 0 visits is taken
                             before any PUCT score while n * n < forced_k * P * S (S the root's visit sum); at the move
                             choice the forced visits PUCT would not have made are taken out again, the move is drawn
                             from the pruned counts T (sample_plies: their first maximum), and T is kept beside the
                             raw counts for kv_root_targets[_device] when keep_root_visits is set. kv_root_visits, the
                             carried subtree and every counter keep the raw counts; a fast ply (fast_sims) has no
                             forcing and T = N. Needs sims >= 1 and arena 0; negative, non-finite or above 16:
                             KV_EINVAL. (forced_k stands before keep_root_visits) */
    int keep_root_visits; /* 1: keep each MCTS move's root visit counts (pi) for kv_root_visits[_device];
                             2: as 1, and also each committed move's root move words for kv_root_moves[_device] */
    int fast_sims;        /* Playout cap randomization (MCTS self-play, DESIGN.md "Playout cap randomization"). 0: off,
                             every ply is searched to sims root visits (no kernel takes another path). Else
                             1 <= fast_sims < sims: each ply is searched either full (sims visits) or fast (fast_sims
                             visits, the root's Dirichlet noise drawn and weighted by 0); the kind is a pure function
                             of cfg.seed + game id and the ply (full_q16). kv_record.pad bit 0 marks a fast ply.
                             Needs sims >= 1 and arena 0; any other value: KV_EINVAL */
    int full_q16;         /* fast_sims > 0: a ply is full when the top 16 bits of its 64-bit hash are below this,
                             1..65536 (65536: every ply full). Must be 0 with fast_sims 0. (The two stand before
                             eval_cache: the struct's last six fields stay eval_cache, leaves, arena, sample_plies,
                             sim_groups, reuse_tree) */
    int eval_cache;      /* Evaluation cache (DESIGN.md "Evaluation cache"): entries per network of an exact memo of the
                             leaf rows in HBM -- one table in self-play, two in an arena -- that kv_run's sim-step
                             probes before it builds the dense leaf batch and fills after the forward. 0: off (no launch,
                             argument or byte of the engine changes). Else a power of two in [64, 2^24], with leaves >= 2;
                             any other value: KV_EINVAL. The key is the row's network inputs (64 board codes, the move
                             count n, the n move words), compared whole; the payload the n legal logits and the value as
                             bits, so play is byte for byte the play with it off. Direct-mapped, KV_CACHE_ENTRY_BYTES per
                             entry; a row of more than KV_CACHE_MAXM moves is never stored. A table lives as long as the
                             engine; kv_load_weights empties player A's, kv_load_weights_b player B's. kv_search* on
                             such an engine runs without it. (eval_cache stands before leaves: the struct's last five
                             fields stay leaves, arena, sample_plies, sim_groups, reuse_tree) */
    int leaves;           /* MCTS self-play and arena (kv_run): descents in flight per game and sim-step (DESIGN.md
                             "Several leaves per game in self-play"). 0 or 1: one leaf, the k_mcts_* kernels and host
                             loops. 2..KV_MAX_LEAVES: every ply's search is the sim-step loop of "Position search" on
                             the self-play root -- up to `leaves` descents per game and step under virtual loss, the
                             collision rule, backups in descent order -- and a step's network batch is the dense list
                             of the pending leaves of all games (per player in an arena), so a ply takes between
                             ceil(sims / leaves) and sims steps. Needs sims >= 1; refused (KV_EINVAL) with
                             reuse_tree 1, eval_mode KV_EVAL_LAZY or sim_groups 2; sim_groups 0 resolves to 1. The
                             network batch class of the whole run is that of slots x leaves (<= 16 rows, or above):
                             in the larger class the root batch and every non-empty leaf batch carry at least 17
                             rows, short ones padded by repeating their first row. Any other value: KV_EINVAL.
                             kv_search* keeps its own `leaves` parameter and ignores this one. (leaves stands before
                             arena: the struct's last four fields stay arena, sample_plies, sim_groups, reuse_tree) */
    int arena;            /* 0: self-play. 1: a match between two networks (DESIGN.md "Arena"): player A is the net of
                             kv_load_weights, player B the net of kv_load_weights_b; in the game with global id g A
                             plays white iff g is even, and a ply's whole search (the root row and every leaf row) runs
                             on the net of the side to move at the root. Everything else is the self-play search.
                             kv_game.outcome stays white-perspective. With KV_EVAL_HASH B's rows are A's with the value
                             negated. Needs sims >= 1, reuse_tree 0 and eval_mode != KV_EVAL_LAZY; sim_groups 2 needs
                             34 slots; kv_search* is refused. Any other value: KV_EINVAL. (arena and sample_plies stand
                             before sim_groups: sim_groups and reuse_tree stay the struct's last two fields) */
    int sample_plies;     /* MCTS move choice (sims >= 1; must be 0 with sims 0). 0: every ply draws random.choices over
                             the root visit counts. k > 0: plies 0..k-1 draw, from ply k on the move is the first
                             maximum of the root visit counts in list order and the CPython stream is not advanced.
                             -1: every ply takes the first maximum. Any other negative value: KV_EINVAL */
    int sim_groups;       /* MCTS self-play: the slot groups a move's sim loop runs as, each group's chain (leaf forward,
                             backup + select) on a stream of its own with its own network workspaces, so that one
                             group's GEMM runs beside the other's output kernels (DESIGN.md "MCTS semantics"). 0: auto
                             (kv_sim_groups_for), 1: one group, 2: two groups of slots / 2 (needs sims >= 1 and more
                             than 16 slots per group, else KV_EINVAL). Records, root visits and stats are the same bit
                             for bit. kv_search* always runs as one group */
    int reuse_tree;       /* MCTS self-play (sims >= 1): 0: every ply's tree is built from nothing; 1: the subtree
                             under the move just played is carried into the next ply (DESIGN.md "MCTS semantics",
                             "Carried subtrees in self-play"): its visits count toward sims, the root takes the
                             fresh root's mixed priors from the same numpy stream. Any other value, or 1 with
                             sims 0: KV_EINVAL */
} kv_config;

#define KV_MAXM 320 /* move-list capacity per position */
/* Evaluation cache (kv_config.eval_cache): the moves an entry holds, and an entry's bytes -- 64 board codes, a
 * 16-byte header (n, the value's bits, 8 reserved), KV_CACHE_MAXM move words, KV_CACHE_MAXM logits' bits = 656,
 * rounded up to whole 64-byte lines. A table of E entries takes E x (KV_CACHE_ENTRY_BYTES + 4) bytes. */
#define KV_CACHE_MAXM 96
#define KV_CACHE_ENTRY_BYTES 704
/* arena with sim_groups 0 (auto): the two players' chains run on two streams from this many slots (DESIGN.md
 * "Arena" records the measurement) */
#ifndef KV_ARENA_TWO_CHAINS_MIN
#define KV_ARENA_TWO_CHAINS_MIN 256
#endif
#define KV_MAX_SIMS 65000 /* MCTS edges keep 16-bit visit counts and child node ids */
/* reuse_tree: inside a ply the compact leaf batch of the slots still searching is rebuilt at every sim-step
 * whose live count is lower than at the last rebuild by at least this many slots (1: every change; DESIGN.md
 * "Carried subtrees in self-play" records the measurement) */
#ifndef KV_REUSE_COMPACT_STEP /* (a build may set another value to measure it) */
#define KV_REUSE_COMPACT_STEP 1
#endif

typedef struct {
    int64_t game_id;
    int32_t ply;
    uint16_t move;       /* encode_move index (ai/ai.py:51-57) */
    uint16_t pad;        /* bit 0: a fast ply of kv_config.fast_sims (not a policy target); else 0 */
    int8_t board[64];   /* position before the move (encode_board input) */
} kv_record;             /* 80 bytes */

typedef struct {
    int64_t game_id;
    int32_t plies;
    int32_t outcome;     /* +1 white win, 0 draw, -1 black win (self_play.py:211-238) */
    float reward;        /* 1.0 / 0.2 / -1.0 (self_play.py:245-250) */
    int32_t reason;      /* 0 max_moves 1 resign 2 mate 3 stalemate 4 draw 5 material */
    int32_t n_evals;     /* network rows consumed by this game's schedule */
    int32_t pad;
} kv_game;               /* 32 bytes */

typedef struct {
    int64_t steps;        /* ply-steps executed */
    int64_t plies;        /* moves committed */
    int64_t games_done;
    int64_t nn_rows;      /* boards evaluated by the network (with kv_config.eval_cache: the rows the search consumed;
                             nn_rows - cache_hits are the rows the network ran, padding aside) */
    int64_t sims;         /* MCTS backups completed (reuse_tree: a ply adds its new backups, not cfg.sims) */
    int64_t records;
    double res_conv_ms;   /* device time of the measured dominant-kernel launches (HIP events):
                             direct: the 10 residual convs of each forward; Winograd: one
                             residual GEMM launch per forward */
    int64_t res_conv_launches;
    double step_ms;       /* wall time inside kv_run */
    double dom_flop;      /* MFMA FLOPs of one measured launch (padded rows included) */
    int64_t dom_algo;     /* KV_ALGO_DIRECT or _WINOGRAD88 for those launches */
    int64_t tree_overflows; /* MCTS expansions dropped for a full edge pool (each also fails kv_run) */
    int64_t nn_rows_lazy;   /* KV_EVAL_LAZY above 16 slots: rows the compact batches sent through the
                               network (nn_rows counts the rows the reference's schedule evaluates) */
    int64_t dom_path;       /* KV_PATH_* of those launches (F(8x8) fp32 or fp64 for KV_ALGO_WINOGRAD88) */
    int64_t dom_split;      /* fp32 F(8x8): points of the GEMM layer run as 128x128 tiles in its first launch
                               (the rest as 64x128 tiles in a second one; 100: one launch); 0 otherwise */
    char dom_kernel[96];    /* the name of the kernel those launches ran, as the library chose it (template
                               arguments included, e.g. "wino88i32_gemm_lagt_kernel<512,5>") */
    int64_t forced_descents; /* kv_config.forced_k: descents at whose root an edge was under its forced count, so
                               that the forced rule and not PUCT chose the root edge, and */
    int64_t visits_pruned;  /* the root visits the pruning took out of the policy targets, the sum over the committed
                               plies of (the raw counts' sum - the pruned counts' sum). Both counted at the move
                               choice; 0 with forced_k 0. (The two stand before plies_full) */
    int64_t plies_full;    /* committed plies searched to cfg.sims (== plies with kv_config.fast_sims 0) and */
    int64_t plies_fast;     /* to cfg.fast_sims, counted at the move choice. reuse_tree 0: sims == plies_full x
                               cfg.sims + plies_fast x cfg.fast_sims; reuse_tree 1: sims + sims_kept == the sum of
                               the committed plies' root visit sums, each max(the ply's target, the visits carried
                               in). (The two stand before arena_rows) */
    int64_t arena_rows[2];  /* arena: the leaf-batch rows player A's / player B's net ran, padding included
                               (arena_rows[0] + arena_rows[1] == leaf_batch_rows); 0, 0 on a self-play engine */
    int64_t cache_probes;   /* kv_config.eval_cache: pending leaf rows probed (== leaf_rows_pending when kv_run returns), */
    int64_t cache_hits;     /* of those the rows an entry answered and the network did not run, */
    int64_t cache_stores;   /* and the entries written (the sum over both tables of an arena); 0 with the cache off.
                               (The three stand before sim_steps: the struct's last five fields stay sim_steps,
                               leaf_rows_pending, sims_kept, roots_carried, leaf_batch_rows) */
    int64_t sim_steps;      /* MCTS sim-steps kv_run ran (select, leaf batch, backup), summed over the ply-steps:
                               plies' steps x sims with kv_config.leaves <= 1; with more leaves a ply-step runs as many
                               as its slowest game needs (collisions decide it) */
    int64_t leaf_rows_pending; /* leaf-batch rows that carried a live game's pending leaf: leaf_batch_rows -
                               leaf_rows_pending is padding (rows of idle slots, of leaves that ended the game, and the
                               rows that fill a batch up to its class). Counted per committed ply at its move choice,
                               so nn_rows == the root rows + leaf_rows_pending when kv_run returns */
    int64_t sims_kept;      /* reuse_tree: root visits carried into plies, summed over the committed plies
                               (sims + sims_kept == plies x cfg.sims) */
    int64_t roots_carried;  /* reuse_tree: committed plies whose root was a carried tree */
    int64_t leaf_batch_rows; /* rows of every MCTS leaf batch the network ran in kv_run, padding included, full
                               and compact batches alike (with reuse_tree 0 too). With kv_config.eval_cache it and
                               arena_rows fall with the hits: only the missed rows' (padded) lists run */
} kv_stats;

typedef struct kv_engine kv_engine;

int kv_create(const kv_config* cfg, kv_engine** out);
/* the slot groups an engine created from cfg runs (kv_config.sim_groups with 0 resolved; no GPU is touched), or
 * KV_EINVAL for a sim_groups kv_create refuses */
int kv_sim_groups_for(const kv_config* cfg);
/* Loads the network weights; under fp32 + KV_ALGO_AUTO this runs the conv-path
 * calibration (kv_net_calibration), reported by kv_engine_calibration. */
int kv_load_weights(kv_engine* e, const float* packed, size_t n_floats);
int kv_engine_calibration(kv_engine* e, kv_calib* out);
/* Arena (kv_config.arena = 1): player B's weights, prepared with the engine's precision / algo -- under AUTO B gets
 * a calibration of its own (kv_engine_calibration_b) and may choose another conv path than A's. Both are KV_EINVAL
 * on an engine created with arena = 0; kv_run on an arena engine needs both weight sets. */
int kv_load_weights_b(kv_engine* e, const float* packed, size_t n_floats);
int kv_engine_calibration_b(kv_engine* e, kv_calib* out);
/* Run ply-steps until every game is finished, or max_steps steps (>= 0), or
 * stop_after_games games have finished in total (>= 0), whichever is first. */
int kv_run(kv_engine* e, int64_t max_steps, int64_t stop_after_games);
/* max_moves for games from now on (_run_single_game's max_moves argument) */
int kv_set_max_moves(kv_engine* e, int max_moves);
int kv_records(kv_engine* e, kv_record* out, size_t cap, size_t* n);
/* The same records, unsorted (allocation order), copied device-to-device into
 * out_dev (a device buffer of cap records on the engine's GPU) on `stream`:
 * the experience stays in HBM for the RCCL gather. out_dev
 * NULL: only *n. The engine's next kv_run / kv_reset_records waits for the
 * copy on its own stream (an event recorded on `stream`), and kv_destroy
 * waits for it before freeing the buffer. */
int kv_records_device(kv_engine* e, kv_record* out_dev, size_t cap, size_t* n, void* stream);
/* finished games (the last 2^20 at most), ordered by game id */
int kv_games(kv_engine* e, kv_game* out, size_t cap, size_t* n);
/* drop the records collected so far (between kv_run calls) */
int kv_reset_records(kv_engine* e);
int kv_stats_get(kv_engine* e, kv_stats* out);
/* sizeof(kv_config) / sizeof(kv_stats) as the library was built, for a binding to check its mirror against */
size_t kv_sizeof_config(void);
size_t kv_sizeof_stats(void);
/* MCTS root visit counts of every committed move (keep_root_visits = 1):
 * out [n][KV_MAXM] in root move-list order, -1 padded, rows in kv_records'
 * order. No reference counterpart (the reference has no search); used by the
 * parity tests against the oracle's PUCT restatement. */
int kv_root_visits(kv_engine* e, int32_t* out, size_t cap, size_t* n);
/* the same visit counts (pi of the (s, pi, z) training triple, BASELINE config C4) device to device, uint16
 * [n][KV_MAXM] in the engine's record order -- row k belongs to record k of kv_records_device (0xffff past the
 * position's move list); stream as in kv_records_device */
int kv_root_visits_device(kv_engine* e, uint16_t* out_dev, size_t cap, size_t* n, void* stream);
/* The root move list those counts are indexed by (keep_root_visits = 2): out uint16 [n][KV_MAXM], entry j the
 * move word (from | to << 6 | flags << 12, as kv_search_result.moves) of count j, 0xffff past the list; rows in
 * kv_records' order, the same permutation as kv_root_visits. The policy logit of a word w is
 * (w & 63) * 64 + ((w >> 6) & 63) (kv_net_forward_boards_legal). On an engine created with keep_root_visits 0
 * or 1: KV_EINVAL. */
int kv_root_moves(kv_engine* e, uint16_t* out, size_t cap, size_t* n);
/* the same words device to device in the engine's record order (row k belongs to record k of kv_records_device
 * and row k of kv_root_visits_device); stream as in kv_records_device */
int kv_root_moves_device(kv_engine* e, uint16_t* out_dev, size_t cap, size_t* n, void* stream);
/* The pruned root counts T of every committed move (kv_config.forced_k > 0 with keep_root_visits set; DESIGN.md
 * "Forced playouts and policy target pruning"): the policy target, kv_root_visits' layout, order and padding -- out
 * [n][KV_MAXM], -1 padded, rows in kv_records' order. A fast ply's row is its raw counts. On an engine created with
 * forced_k 0 or keep_root_visits 0: KV_EINVAL. */
int kv_root_targets(kv_engine* e, int32_t* out, size_t cap, size_t* n);
/* the same counts device to device, kv_root_visits_device's layout (uint16, 0xffff padded, the engine's record
 * order); stream as in kv_records_device */
int kv_root_targets_device(kv_engine* e, uint16_t* out_dev, size_t cap, size_t* n, void* stream);
int kv_sync(kv_engine* e);
void kv_destroy(kv_engine* e);

/* ------------------------------------------------------ position search ---
 * PUCT search of n given positions (DESIGN.md "MCTS semantics": the self-play
 * search from any root, with `leaves` descents in flight per tree and sim-step
 * under virtual loss, so one position fills a network batch of `leaves` rows;
 * leaves = 1 is the self-play search bit for bit). No reference counterpart.
 *
 * The engine comes from kv_create with slots >= n and sims >= p->sims >= 1 (the
 * tree pools); c_puct, eval_mode, precision, algo and tree_edge_cap are its
 * config's, n_games may be 0. An engine serves either kv_run or kv_search:
 * calling one after the other has been used is KV_EINVAL. states: n 80-byte
 * state vectors (64 board codes, wtm, king squares, moved flags, ep, as
 * kv_dev_valid_moves reads them). Position i's numpy stream (the root's
 * Dirichlet draw) is seeded p->seed + i; with eps = 0 the result does not
 * depend on it. A shrunk tree_edge_cap that overflows raises KV_EOVERFLOW. */
#define KV_MAX_LEAVES 64
typedef struct { int sims; int leaves; double eps, alpha; uint64_t seed; } kv_search_params;
typedef struct {
    int32_t status;   /* 0 searched, 1 checkmated root, 2 stalemate, 3 draw (kings only) */
    int32_t n_moves, sims, best, pv_len, steps, nn_rows, pad; /* best: first maximum of visits (-1: not
                         searched); steps: sim-steps run; nn_rows: the root's row + the leaves evaluated */
    float root_value; /* network value of the root, white perspective; terminal: that value */
    float best_q;
    uint16_t pv[16];  /* first-max-visit edges from the root through expanded children, as move words */
    uint16_t moves[KV_MAXM];  /* from | to<<6 | flags<<12, root list order (kv_dev_valid_moves' words) */
    int32_t  visits[KV_MAXM]; /* -1 past n_moves */
    float    q[KV_MAXM], prior[KV_MAXM]; /* q = W/N from the root mover's side, 0 where unvisited */
} kv_search_result;
int kv_search(kv_engine* e, const int8_t* states /*[n][80]*/, int n,
              const kv_search_params* p, kv_search_result* out /*[n]*/);
size_t kv_sizeof_search_result(void);

/* Search sessions (DESIGN.md "Search sessions"): the trees of the last kv_search follow a game, so that the
 * subtree under a played move is searched on instead of rebuilt. A kv_search starts a new session; n must be
 * the session's; both calls are KV_EINVAL before any kv_search. A call that fails on the device (KV_EHIP,
 * KV_EOVERFLOW) ends the session.
 *
 * kv_search_advance plays root move edge[i] (root list index; -1: tree i stays as it is) in every tree: the
 * child's subtree becomes the tree, its visits, values, priors and move words carried bit for bit; an edge
 * without an expanded child (never visited, or a move into mate, stalemate or kings only) drops the tree. An
 * edge >= the root's n_moves, or >= 0 at a root that was not searched, is KV_EINVAL and changes no tree.
 * states_out (or NULL): the state vectors after the moves (the current ones where edge is -1).
 *
 * kv_search_continue searches the current roots up to p->sims root visits, the carried ones counting:
 * a tree that already holds them runs no step. A dropped tree is searched as kv_search searches a given
 * position. p->eps must be 0 (no noise at a carried root). out as kv_search, with sims = the root's visits
 * (carried + new), steps and nn_rows of this call only (no root row for a carried tree); kept (or NULL):
 * the visits each root held when the call began, 0 for a dropped tree. leaves may differ from call to call.
 *
 * kv_search_tree_size: the nodes of tree i and the edges of its pool it occupies (every node's block counted
 * to its 16-edge boundary); 0, 0 for a root that is not searched or a dropped tree not yet continued. */
int kv_search_advance(kv_engine* e, int n, const int32_t* edge /*[n]*/, int8_t* states_out /*[n][80] or NULL*/);
int kv_search_continue(kv_engine* e, int n, const kv_search_params* p, kv_search_result* out /*[n]*/,
                       int32_t* kept /*[n] or NULL*/);
int kv_search_tree_size(kv_engine* e, int i, int32_t* nodes, int32_t* edges);

/* ------------------------------------------------- device test entry points ---
 * Run one device kernel over host-provided inputs (copies in and out). They
 * exist so parity tests can call the product kernels through the C ABI. */

/* getValidMoves (core/chessEngine.py:277-321) for n states (80-byte vectors,
 * see oracle/kv_oracle.c); moves_out [n][cap] as uint16 from|to<<6|flags<<12
 * (flags bit0 ep, bit1 castle, bit2 promotion); n_moves [n]; states_after
 * [n][80] (the reference may mutate the board); in_check [n]. */
int kv_dev_valid_moves(int device, const int8_t* states, int n, uint16_t* moves_out, int cap, int* n_moves,
                       int8_t* states_after, uint8_t* in_check);
/* squareUnderAttack (chessEngine.py:400-415) for all 64 squares: bit r*8+c of
 * attacked[i] is set when an opponent pseudo-move of state i ends on (r, c);
 * inCheck (:388-394) is the bit of the mover's stored king location. */
int kv_dev_attacks(int device, const int8_t* states, int n, uint64_t* attacked);
/* kv_dev_attacks' attack set computed on the host CPU: the same source (targets(), csrc/kv_movegen.h)
 * compiled for the host, so tests can pin it against the reference's recorded sets without a GPU. */
int kv_host_attacks(const int8_t* states, int n, uint64_t* attacked);
/* makeMove (chessEngine.py:127-197) of move index[i] of each state's list. */
int kv_dev_make_move(int device, int8_t* states, const int* index, int n);
/* Where the engine's games start (tests only: self-play and the arena have no opening book). states: n >= 1
 * 80-byte state vectors as kv_search takes them, checked as kv_search checks them (KV_EINVAL and a reason in
 * kv_last_error()). The game with global id g starts from states[g % n], at ply 0 with a fresh slot, whether
 * it is one of the first wave of games or starts in a recycled slot, in both seed modes -- so which position a
 * game gets depends on its id alone, not on slots, recycling order, game_id_base or game_id_stride. NULL with
 * n 0 restores the initial position. Only on an engine that has neither run nor searched (later: KV_EINVAL);
 * the games the engine's creation already started are re-seated. A start without a legal move is a game of 0
 * plies (no record, no root-visit row, reason 2 or 3); a kings-only start plays one move and is then a
 * reason-4 draw, as the reference tests isDraw only after a move. With no starts set nothing of the engine
 * changes. */
int kv_dev_set_starts(kv_engine* e, const int8_t* states /*[n][80]*/, int n);
/* numpy RandomState(seed[i]).dirichlet([alpha]*k) `draws` times per stream:
 * out [n][draws][k] fp64, attempts [n][draws] gamma attempts consumed,
 * tail [n] = the stream's next random_sample() after the draws. */
int kv_dev_dirichlet(int device, const uint64_t* seeds, int n, double alpha, int k, int draws, double* out,
                     int64_t* attempts, double* tail);
/* The evaluation cache's probe and store kernels (kv_config.eval_cache) on a fresh table of `entries` entries (a
 * power of two in [64, 2^24]) over n_rows given rows: boards [n_rows][64], moves [n_rows][KV_MAXM] move words,
 * counts [n_rows] (0 .. KV_MAXM; here a row of 0 moves is probed like any other), and the payload the network
 * would give: logits [n_rows][KV_MAXM] and values [n_rows] as bits. step_len [n_steps] cuts the rows into
 * consecutive sim-steps (their sum is n_rows): per step the product's probe over the step's rows, then its store
 * of the missed ones. hit [n_rows]: 1 where the probe found the row's key; out_logits [n_rows][KV_MAXM] /
 * out_values [n_rows]: what the probe wrote for a hit (the row's first n logits; everything else stays 0xff
 * bytes). counters [3] (or NULL): probes, hits, stores as the device counted them. */
int kv_dev_eval_cache(int device, int entries, const int8_t* boards, const uint16_t* moves, const int* counts,
                      const uint32_t* logits, const uint32_t* values, int n_rows, const int* step_len, int n_steps,
                      int32_t* hit, uint32_t* out_logits, uint32_t* out_values, int64_t* counters);
/* The device's restatement of glibc log (op 0: out = log(x)) / pow (op 1:
 * out = pow(x, y)) (csrc/kv_libm.h, used by the Dirichlet draw), run on the
 * host CPU: the same source compiled for the host, so tests can pin it against
 * libm itself without a GPU. */
int kv_host_libm(int op, const double* x, const double* y, int n, double* out);
/* CPython random.Random(seed[i]): count random() values -> out [n][count]. */
int kv_dev_py_random(int device, const uint64_t* seeds, int n, int count, double* out);
/* The int8-digit Winograd GEMM of one conv layer (csrc/kv_wino88i.h): V [100][rows][K]
 * and U [100][512][K] fp64 (K 256 or 512, rows a multiple of 128) are split into
 * `digits` int8 digits by the product's slice kernel and multiplied by its GEMM
 * kernel: M [100][rows][512] (digits 5: KV_PREC_I8X5's fp64 M; 4: the fp32
 * domain's (KV_ALGO_WINOGRAD88_I8) fp32 M, widened); v_digits (5 digits: planes
 * [100][K/32][5][rows][32]; 4 digits: row lines [100][K/32][rows][4][32]) and
 * v_exp [100][rows] (either may be NULL) return V's digits and row exponents. seg 2 (4 digits):
 * KV_PREC_I8R4's 4 radix-256 digits in row lines [100][K/32][rows][4][32], its GEMM and fp64 M. seg 3
 * (4 digits): KV_ALGO_WINOGRAD88_I8R3's 3 radix-256 digits in 96-byte row lines [100][K/32][rows][3][32] (the
 * first 3/4 of v_digits, the rest zero), the product's 6-pair GEMM and fp32 M. seg 1 (exponents per
 * 256-channel segment, a removed form) and any other value: KV_EINVAL, checked before any device call. */
int kv_dev_wino88i(int device, const double* V, int rows, const double* U, int K, int digits, int seg, double* M,
                   int8_t* v_digits, int* v_exp);
/* The fp32 tower's residual output kernel on int8 digits (KV_ALGO_WINOGRAD88_I8): M [100][rows][512] fp32
 * (rows a multiple of 128), folded BN scale / shift [512], resid [rows][64][512] or NULL -> Y
 * [rows][64][512] (= ReLU(A^T M A * scale + shift (+ resid))) and the next conv's V as row-line digits
 * [100][16][rows][4][32] with row exponents [100][rows]. fused bit 0 set: the product's one-kernel form
 * (wino88i32_out_kernel), clear: wino88_out_kernel's fp32 V then the slice kernel (bit-identical); bit 4: 3
 * radix-256 digits, KV_ALGO_WINOGRAD88_I8R3's, in 96-byte lines [100][16][rows][3][32] in the first 3/4 of
 * v_digits, the rest zero; bit 2 (KV_ALGO_WINOGRAD88_I8V's V, not with bit 4): with bit 0 the one-kernel
 * wino88i32v_out_kernel, without it wino88_out_kernel's Y, then wino88d_in_kernel's fp64 V and the slice kernel
 * (bit-identical). Bits 1, 3 and 5 (removed forms) and higher: KV_EINVAL, checked before any device call. */
int kv_dev_wino88i32_out(int device, const float* M, int rows, const float* scale, const float* shift,
                         const float* resid, int fused, float* Y, int8_t* v_digits, int* v_exp);
/* The front of the R3 tower (KV_ALGO_WINOGRAD88_I8R3): boards [nb][64] int8 piece codes (0 empty, 1-12), `rows`
 * >= nb a multiple of 32 (the rows past nb are empty boards), conv1 as wT [9][12][256] ([tap][piece][cout]),
 * folded BN scale / shift [256] -> conv2's V as 3 radix-256 digits in 96-byte row lines [100][8][rows][3][32] in
 * the first 3/4 of v_digits ([100][8][rows][4][32] bytes; the rest comes back as the byte 0x55) and row exponents
 * [100][rows]. fused 1: the product's one-kernel form (stem_r3_kernel); 0: stem_kernel<4>'s fp32 V256, then the
 * slice kernel (bit-identical). */
int kv_dev_tower_front(int device, const int8_t* boards, int nb, int rows, const float* wT, const float* scale,
                       const float* shift, int fused, int8_t* v_digits, int* v_exp);
/* The back end of the fp32 tower on int8 digits: the last residual block's output step and the heads. M
 * [100][rows][512] fp32 (rows a multiple of 32), folded BN scale / shift [512], resid [rows][64][512], heads =
 * head conv weights [3][512] (policy 0, policy 1, value) | their BN scale [3] | shift [3] | value_fc1 weight
 * [512][64] | bias [512] | value_fc2 weight [512] | bias [1] -> pfeat [rows][128] (channel-major policy
 * features) and value [rows]. fused bit 0: the product's one-kernel form (wino88_out_heads_kernel: the activation
 * goes from the output transform to the heads through LDS, no X; with bit 1 the residual read non-temporally,
 * as the tower runs it at 1,024+ boards); clear: wino88_out_kernel's X, then heads_kernel (bit-identical). */
int kv_dev_tower_back(int device, const float* M, int rows, const float* scale, const float* shift,
                      const float* resid, const float* heads, int fused, float* pfeat, float* value);
/* KV_PREC_I8R4's output step: M [100][rows][512] fp64 (rows a multiple of 128), folded BN scale / shift,
 * resid or NULL -> Y [rows][64][512] and the next conv's V as 4 radix-256 digits in row lines
 * [100][16][rows][4][32] with row exponents [100][rows]. fused 1: the product's wino88i64r_out_kernel; 0:
 * wino88d_out_half_kernel's Y, wino88d_in_kernel's fp64 V, the radix-256 slice kernel (bit-identical). */
int kv_dev_wino88r_out(int device, const double* M, int rows, const float* scale, const float* shift,
                       const float* resid, int fused, float* Y, int8_t* v_digits, int* v_exp);
/* Two nets with the same weights run side by side, each forward on a stream of its own (the probe of a two-group
 * sim-step, tools/two_stream_forward_probe.py). cu_share 2: the R3 GEMM of either net sizes its grid for half the
 * CUs (the one-round form when its tiles fill whole rounds of them), so two GEMMs in flight fill the chip once and
 * a GEMM leaves half of it to the other net's output kernel; 1: the whole chip, as a net alone. follow 1: b's GEMM
 * of every conv waits (stream-side, no host sync) for a's GEMM of the same conv in the forward enqueued before it,
 * so b runs half a layer behind a; the caller enqueues a's forward first, then b's. Outputs are unchanged. A
 * destroyed `a` must not stay b's leader: pair again (follow 0) or destroy b first. */
int kv_dev_net_pair(kv_net* a, kv_net* b, int cu_share, int follow);
/* The clock the chip holds under the headline GEMM (a diagnostic; MI355X_MICROARCH.md "DVFS give-back" item 6):
 * the product's fp32-tower GEMM (K 512, `rows` boards, `digits` 4 or 3 (KV_ALGO_WINOGRAD88_I8R3), seeded random
 * digits) back to back for `seconds`, then
 * one launch of its stamped build: out[0] = median over workgroups of (s_memtime delta / s_memrealtime delta)
 * x 100 MHz, out[1] = the back-to-back launches' mean time (us), out[2] = their count, out[3] = tiles per
 * workgroup of the stamped kernel, which runs on the product launch's grid. */
int kv_dev_gemm_clock(int device, int rows, int digits, double seconds, double* out);
/* kv_dev_gemm_clock for KV_ALGO_WINOGRAD88_I8R3's GEMM with the tower's CU share (`share` 2: the grid sized for
 * half the CUs, as with two slot groups side by side; 1: the whole chip) and, abl 16, the timing ablation that
 * compiles the tile epilogue out (no conversion, no M stores; M is not written), which only this entry reaches.
 * out[0..3] as kv_dev_gemm_clock, out[4] = workgroups of the launch (the product's one-round grid). */
int kv_dev_r3gemm_clock(int device, int rows, int abl, int share, double seconds, double* out);
/* KV_ALGO_WINOGRAD88_I8R3's slice kernel and GEMM on a slice of a longer buffer: V [100][rows][K] and U
 * [100][512][K] fp64 (K 256 or 512); the digits, exponents and M occupy rows [row0, row0 + rows) of buffers
 * `stride` rows long (all multiples of 128, stride at most 16,384), as a forward's slices do. tpw 0: the
 * product's kernel and grid for `rows`; 1, 4 or 5: that many tiles per workgroup in nwg workgroups (0: the
 * launcher's grid; else a multiple of 8 with 400 rows / 128 = tpw x nwg x groups). M [100][rows][512] returns
 * those rows (fp32, widened); *outside = how many elements of M's other rows the launch changed. */
int kv_dev_wino88i_r3(int device, const double* V, int rows, const double* U, int K, int tpw, int nwg, int stride,
                      int row0, double* M, long long* outside);
/* Phase timing of the fp32 tower's output kernel (a diagnostic build of wino88i32_out_kernel with shader-clock
 * stamps) at `rows` boards on seeded M (resid: the residual + Y variant; r3: 3 radix-256 digits): stamps
 * [min(rows, 4096)][2][6] = s_memtime of waves 0 and 15 of each board's workgroup at start, V ready, after the
 * maxima barrier, after the exponent barrier, digit stores issued, stores drained; us = that launch's time. */
int kv_dev_out_phases(int device, int rows, int resid, int r3, unsigned long long* stamps, float* us);

/* ------------------------------------------------------- data pipeline ---
 * Full-rules chess (python-chess 1.999 semantics, csrc/kv_chess.cpp) for the
 * reference's PGN -> JSONL ingestion and its JSONL datasets. Host code: no
 * GPU is touched. Squares here are python-chess's (a1 = 0, h8 = 63).
 *
 * kv_pgn_extract replaces data_utils/parser_pgn.py:81-118
 * extract_data_from_pgn's loop (chess.pgn.read_game + board.fen() /
 * board.san(move) / board.push(move) per mainline move): one record per
 * mainline move of every game in `text`, in file order. Stops before a game
 * whose records would not fit in `cap` and reports in *consumed the bytes of
 * `text` processed (whole games), so callers loop over large inputs;
 * KV_EOVERFLOW if a single game does not fit (*n_out = its move count). */
#define KV_PGN_OUTCOME_NONE (-128) /* Result "*" or unknown: the reference's `outcome = None` */
typedef struct kv_pgn_record {
    char fen[100];   /* board.fen() before the move, NUL-terminated */
    char san[12];    /* board.san(move) */
    int32_t outcome; /* 1 ("1-0"), -1 ("0-1"), 0 ("1/2-1/2"), KV_PGN_OUTCOME_NONE */
    int32_t game;    /* index of the game within this call */
} kv_pgn_record;
int kv_pgn_extract(const char* text, size_t len, kv_pgn_record* out, size_t cap, size_t* n_out, size_t* consumed,
                   int64_t* n_games);
/* fen_to_tensor's piece scan (data_utils/dataset.py:59-68, scripts/train.py:531-545):
 * n FENs, `stride` bytes apart (NUL-terminated) -> codes[n][64] int8, 0 empty,
 * 1..12 = P N B R Q K p n b r q k (the PGN plane order + 1), index row*8+col
 * with row 0 = rank 8. */
int kv_fen_codes(const char* fens, size_t stride, int n, int8_t* codes);
/* ChessPGNDataset.default_move_encoder (scripts/train.py:553-558):
 * board.parse_san(san) -> from_square*64 + to_square. */
int kv_san_move_index(const char* fens, size_t fen_stride, const char* sans, size_t san_stride, int n,
                      int32_t* out);
/* test / tooling entry points: perft node count, SAN round trip (parse_san ->
 * san, fen after push), Board(fen).fen() */
int kv_chess_perft(const char* fen, int depth, uint64_t* nodes);
int kv_chess_san(const char* fen, const char* san_in, char* san_out, size_t san_cap, char* fen_after, size_t fen_cap);
int kv_chess_fen(const char* fen_in, char* fen_out, size_t cap);

/* --------------------------------------------------------------- train ---
 * Update-step kernels of the learn loop. The reference
 * trains ChessNet under torch.cuda.amp.autocast (scripts/train.py:161-184):
 * its 3x3 convolutions (ai/model.py:34-40, :8-25) run on fp16 operands with
 * fp32 accumulation and fp16 outputs, its BatchNorms in training mode (fp32
 * batch statistics, fp16 output). These entry points restate those units for
 * the tower (conv1, conv2, the 5 residual blocks), replacing the MIOpen
 * convolutions / BatchNorms torch calls there (knightvision_amd/train_ops.py
 * wraps them as autograd functions). Activations are NHWC fp16 device arrays
 * [n boards][64 squares][C]; weights fp16 [co][9][ci] (tap = 3 * row + col of
 * the 3x3 kernel); every call is asynchronous on `stream`.
 */
/* y = bias + conv3x3(x, w), pad 1 on the 8x8 board; ci % 16 == 0, co % 128 == 0;
 * bias_dev fp32 [co] or NULL. Also the data gradient: x = dy, w = the flipped
 * image of kv_tr_conv_weights_f16, co = the conv's input channels. */
int kv_tr_conv3x3_f16(const void* x_dev, int n, int ci, const void* w_dev, const float* bias_dev, int co,
                      void* y_dev, void* stream);
/* the same with a fused fp16 addend: y = fp16(float(fp16(bias + conv3x3(x, w))) + float(add)) -- the data
 * gradient of a residual block's first conv plus the residual branch's gradient, rounded as autograd's
 * fp16 gradient accumulation rounds it; add_dev [n][64][co] (not y_dev) or NULL */
int kv_tr_conv3x3_add_f16(const void* x_dev, int n, int ci, const void* w_dev, const float* bias_dev, int co,
                          const void* add_dev, void* y_dev, void* stream);
/* fp32 torch weight [co][ci_real][3][3] -> fp16 forward image [co][9][ci] (channels >= ci_real zero) and,
 * if wt_dev != NULL, the data-gradient image [ci][9][co] (taps flipped) */
int kv_tr_conv_weights_f16(const float* w_dev, int co, int ci_real, int ci, void* wf_dev, void* wt_dev, void* stream);
/* bytes of workspace kv_tr_conv3x3_wgrad_f16 needs (and the board splits it uses) */
size_t kv_tr_wgrad_workspace(int n, int ci, int co, int* splits);
/* dw fp32 [co][ci_real][3][3] = fp16-rounded sum over boards and squares of dy (x) shifted x;
 * ci % 64 == 0, co % 64 == 0; deterministic (fixed split order) */
int kv_tr_conv3x3_wgrad_f16(const void* dy_dev, const void* x_dev, int n, int ci, int ci_real, int co, float* dw_dev,
                            void* ws_dev, size_t ws_bytes, void* stream);
/* bytes of workspace the BatchNorm / channel-sum calls need for rows x C */
size_t kv_tr_bn_workspace(int rows, int C);
/* training BatchNorm statistics over rows (= boards x 64) of fp16 x: mean, biased var, 1/sqrt(var + eps) */
int kv_tr_bn_stats_f16(const void* x_dev, int rows, int C, float eps, float* mean_dev, float* var_dev,
                       float* invstd_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* y = fp16((x - mean) * invstd * gamma + beta); res_dev != NULL: y = fp16(y + res); relu: max(y, 0) */
int kv_tr_bn_apply_f16(const void* x_dev, int rows, int C, const float* mean_dev, const float* invstd_dev,
                       const float* gamma_dev, const float* beta_dev, const void* res_dev, int relu, void* y_dev,
                       void* stream);
/* backward of kv_tr_bn_apply_f16 (y_dev = its output, for the ReLU mask): dgamma, dbeta fp32 [C], dx fp16 and,
 * if dres_dev != NULL, the residual's gradient (the masked dy); if dxsum_dev != NULL, the channel sums of dx
 * fp32 [C] (the bias gradient of the conv that produced x, without a second pass over dx) */
int kv_tr_bn_backward_f16(const void* x_dev, const void* dy_dev, const void* y_dev, int rows, int C, int relu,
                          const float* mean_dev, const float* invstd_dev, const float* gamma_dev, float* dgamma_dev,
                          float* dbeta_dev, void* dx_dev, void* dres_dev, float* dxsum_dev, void* ws_dev,
                          size_t ws_bytes, void* stream);
/* per-channel sum of fp16 rows x C (a conv bias gradient) */
int kv_tr_channel_sum_f16(const void* x_dev, int rows, int C, float* sum_dev, void* ws_dev, size_t ws_bytes,
                          void* stream);
/* the heads' 1x1 convolutions (policy 512 -> 2, value 512 -> 1; ai/model.py:42-49) over rows = boards x 64 of
 * the tower output h fp16 [rows][512]: w fp16 [3][512] (policy rows 0-1, value row 2), b fp32 [3] (fp16 values);
 * out fp16 [rows][4] (column 3 unused) */
int kv_tr_head1x1_f16(const void* h_dev, int rows, const void* w_dev, const float* b_dev, void* out_dev,
                      void* stream);
size_t kv_tr_head1x1_workspace(int rows);
/* its backward from dout fp16 [rows][4]: dh fp16 [rows][512], dw fp32 [3][512], db fp32 [3] (fp16-rounded) */
int kv_tr_head1x1_backward_f16(const void* h_dev, const void* dout_dev, int rows, const void* w_dev, void* dh_dev,
                               float* dw_dev, float* db_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* encode_board planes fp32 [n][12][8][8] (ai/ai.py:17-30) -> NHWC fp16 [n][64][cpad], channels >= 12 zero */
int kv_tr_planes_to_nhwc(const float* planes_dev, int n, int cpad, void* out_dev, void* stream);
/* Soft-target policy loss on MCTS root visit distributions (no reference counterpart: the reference trains on
 * the move played). logits fp16 [B][4096], 16-byte aligned; the targets are a CSR over the whole dataset:
 * off int64 [N + 1], idx / cnt uint16 [nnz], one entry per legal root move (policy index (w & 63) * 64 +
 * ((w >> 6) & 63) of its move word w, visit count), and row [B] names the dataset row of each batch row
 * (0 <= row[i] < N and idx < 4096 are the caller's to guarantee; an entry with idx >= 4096 is skipped). Per batch
 * row, with z the logits widened to fp32, p = softmax(z) and pi_k = (sum of cnt with idx k) / (sum of the row's
 * cnt), 0 for a row whose counts are all 0:
 *   lse = max + log sum exp(z - max), ce = -sum_k pi_k (z_k - lse), ent = lse - sum_k p_k z_k.
 * Every output is bit-reproducible and independent of B and of the row's place in the batch. */
int kv_tr_policy_loss_f16(const void* logits_dev, const int64_t* row_dev, const int64_t* off_dev,
                          const uint16_t* idx_dev, const uint16_t* cnt_dev, int B, float* ce_dev, float* ent_dev,
                          float* lse_dev, void* stream);
/* its backward from the forward's lse / ent and the per-row gradients gce / gent of ce / ent (they carry the
 * means, the entropy coefficient and the loss scale), s = sum_k pi_k (1 or 0):
 *   dlogits_k = fp16(gce (s p_k - pi_k) - gent p_k ((z_k - lse) + ent)), computed in fp32, rounded once */
int kv_tr_policy_loss_backward_f16(const void* logits_dev, const int64_t* row_dev, const int64_t* off_dev,
                                   const uint16_t* idx_dev, const uint16_t* cnt_dev, int B, const float* lse_dev,
                                   const float* ent_dev, const float* gce_dev, const float* gent_dev,
                                   void* dlogits_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KV_H */
