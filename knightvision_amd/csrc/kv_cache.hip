// Evaluation cache (kv_config.eval_cache, DESIGN.md "Evaluation cache"): an exact, direct-mapped memo of the dense
// leaf batch's network rows in HBM, one table per network.
//
// An entry is KV_CACHE_ENTRY_BYTES = 44 16-byte words:
//   [0, 4)    the 64 board codes
//   [4]       n, the value's bits, 0, 0
//   [5, 17)   KV_CACHE_MAXM move words (0 past n)
//   [17, 41)  KV_CACHE_MAXM logits as bits (0 past n)
//   [41, 44)  unused (an entry is whole 64-byte lines)
// An empty table is 0xff bytes: n = -1 matches no row. The index is the low bits of cache_hash over the key (the
// board's 32 byte pairs, n, the n move words); a hit needs every key byte equal.
//
// A sim-step runs two launches, one wave per workspace row, and nothing inside a launch depends on another
// workgroup of it. k_cache_probe reads the table only: a hit copies the payload into the row's logits / value and
// raises its flag (k_leaves_compact leaves a flagged row out of the list), a miss takes the entry's claim word down
// to its row index (device-scope atomicMin). k_cache_store, after the forward and the scatter, lets the row that
// holds an entry's claim -- the earliest miss of the step in list order, the lists being in row order -- write the
// entry and hand the claim back. So the rows of one step never see each other's stores, and the table after a step
// does not depend on the order the waves ran in.
#include <hip/hip_runtime.h>

#include "kv_engine.h"

namespace kv {

constexpr int CACHE_ENTRY_U4 = KV_CACHE_ENTRY_BYTES / 16;
static_assert(KV_CACHE_ENTRY_BYTES % 64 == 0 && KV_CACHE_MAXM % 8 == 0 && KV_CACHE_MAXM <= MAXM &&
                  64 + 16 + KV_CACHE_MAXM * 6 <= KV_CACHE_ENTRY_BYTES,
              "an entry is whole lines and holds KV_CACHE_MAXM moves");
constexpr int CE_HDR = 4, CE_MOVES = 5, CE_LOGITS = CE_MOVES + KV_CACHE_MAXM / 8, CE_END = CE_LOGITS + KV_CACHE_MAXM / 4;
static_assert(CE_END <= 64, "one lane per 16-byte word of an entry");

__device__ inline unsigned long long cache_mix64(unsigned long long z) {  // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// h = XOR_k mix64((k + 1) * 0x9E3779B97F4A7C15 ^ w_k) over the key's 16-bit words: k < 32 the board's byte pairs
// (little endian), k = 32 the count n, k = 33 + j move word j. Lane l takes the words l, l + 64, ..; every lane
// returns the wave's XOR.
__device__ inline unsigned long long cache_hash(const int8_t* board, const uint16_t* mw, int n, int lane) {
    const uint16_t* bw = (const uint16_t*)board;
    unsigned long long h = 0;
    for (int k = lane; k < 33 + n; k += 64) {
        const unsigned w = k < 32 ? bw[k] : k == 32 ? (unsigned)n : mw[k - 33];
        h ^= cache_mix64(((unsigned long long)(k + 1) * 0x9E3779B97F4A7C15ull) ^ (unsigned long long)w);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)h, m), hi = __shfl_xor((unsigned)(h >> 32), m);
        h ^= ((unsigned long long)hi << 32) | lo;
    }
    return h;
}

// the bits of a 32-bit pair of move words (first word index j) that lie below n
__device__ inline unsigned cache_pair_mask(int j, int n) {
    return (j < n ? 0xffffu : 0u) | (j + 1 < n ? 0xffff0000u : 0u);
}

// the table of the row's network: the arena's player of the slot's mover (k_leaves_compact's rule), else A's
__device__ inline const CacheTab& cache_tab_of(const CacheTab& ta, const CacheTab& tb, const Slot* slots, int slot) {
    if (!slots) return ta;
    const Slot& s = slots[slot];
    return (((s.game_id & 1) == 0) == (s.wtm != 0)) ? ta : tb;
}

// One wave per row. A row of fewer than nmin moves is not pending (the engine: 1). hit[r] = 1 and the payload in
// llogits / lvalues where the row's key is in its table; a miss of at most KV_CACHE_MAXM moves leaves its entry
// index in cidx[r] and claims the entry.
__global__ __launch_bounds__(64) void k_cache_probe(CacheTab ta, CacheTab tb, const Slot* slots, int L, int nmin,
                                                    const int8_t* lboards, const uint16_t* lmoves, const int* lcnt,
                                                    float* llogits, float* lvalues, int* hit, int* cidx,
                                                    CacheCtr* cc) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int n = min(lcnt[r], MAXM);
    if (n < nmin) {
        if (lane == 0) hit[r] = 0;
        return;
    }
    if (n > KV_CACHE_MAXM) {  // more moves than an entry holds: a miss, never stored
        if (lane == 0) {
            hit[r] = 0;
            atomicAdd(&cc->probes, 1ull);
        }
        return;
    }
    const CacheTab& t = cache_tab_of(ta, tb, slots, r / L);
    const int8_t* board = lboards + (size_t)r * 64;
    const uint16_t* mw = lmoves + (size_t)r * MAXM;
    const unsigned idx = (unsigned)cache_hash(board, mw, n, lane) & t.mask;
    const uint4* e = t.ent + (size_t)idx * CACHE_ENTRY_U4;
    bool same = true;
    if (lane < CE_HDR) {
        const uint4 a = e[lane], b = ((const uint4*)board)[lane];
        same = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
    } else if (lane == CE_HDR) {
        same = (int)e[CE_HDR].x == n;
    } else if (lane < CE_LOGITS) {
        const int j = (lane - CE_MOVES) * 8;
        if (j < n) {
            const uint4 a = e[lane], b = ((const uint4*)mw)[lane - CE_MOVES];
            same = (((a.x ^ b.x) & cache_pair_mask(j, n)) | ((a.y ^ b.y) & cache_pair_mask(j + 2, n)) |
                    ((a.z ^ b.z) & cache_pair_mask(j + 4, n)) | ((a.w ^ b.w) & cache_pair_mask(j + 6, n))) == 0;
        }
    }
    const bool found = __all(same);
    if (found) {
        unsigned* lg = (unsigned*)llogits + (size_t)r * MAXM;
        if (lane >= CE_LOGITS && lane < CE_END) {
            const int j = (lane - CE_LOGITS) * 4;
            if (j < n) {
                const uint4 a = e[lane];
                lg[j] = a.x;
                if (j + 1 < n) lg[j + 1] = a.y;
                if (j + 2 < n) lg[j + 2] = a.z;
                if (j + 3 < n) lg[j + 3] = a.w;
            }
        }
        if (lane == 0) {
            ((unsigned*)lvalues)[r] = e[CE_HDR].y;
            hit[r] = 1;
            atomicAdd(&cc->probes, 1ull);
            atomicAdd(&cc->hits, 1ull);
        }
    } else if (lane == 0) {
        hit[r] = 0;
        cidx[r] = (int)idx;
        atomicMin(&t.claim[idx], r);
        atomicAdd(&cc->probes, 1ull);
    }
}

// One wave per row, after the step's forward and scatter: the missed row that holds its entry's claim writes the
// entry from the row's inputs and outputs and hands the claim back.
__global__ __launch_bounds__(64) void k_cache_store(CacheTab ta, CacheTab tb, const Slot* slots, int L, int nmin,
                                                    const int8_t* lboards, const uint16_t* lmoves, const int* lcnt,
                                                    const float* llogits, const float* lvalues, const int* hit,
                                                    const int* cidx, CacheCtr* cc) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int n = min(lcnt[r], MAXM);
    if (n < nmin || n > KV_CACHE_MAXM || hit[r]) return;
    const CacheTab& t = cache_tab_of(ta, tb, slots, r / L);
    const unsigned idx = (unsigned)cidx[r] & t.mask;
    if (t.claim[idx] != r) return;
    uint4* e = t.ent + (size_t)idx * CACHE_ENTRY_U4;
    if (lane < CE_HDR) {
        e[lane] = ((const uint4*)(lboards + (size_t)r * 64))[lane];
    } else if (lane == CE_HDR) {
        e[CE_HDR] = make_uint4((unsigned)n, ((const unsigned*)lvalues)[r], 0u, 0u);
    } else if (lane < CE_LOGITS) {
        const int j = (lane - CE_MOVES) * 8;
        uint4 b = make_uint4(0u, 0u, 0u, 0u);
        if (j < n) {
            b = ((const uint4*)(lmoves + (size_t)r * MAXM))[lane - CE_MOVES];
            b.x &= cache_pair_mask(j, n);
            b.y &= cache_pair_mask(j + 2, n);
            b.z &= cache_pair_mask(j + 4, n);
            b.w &= cache_pair_mask(j + 6, n);
        }
        e[lane] = b;
    } else if (lane < CE_END) {
        const int j = (lane - CE_LOGITS) * 4;
        uint4 b = make_uint4(0u, 0u, 0u, 0u);
        if (j < n) {
            b = ((const uint4*)(llogits + (size_t)r * MAXM))[lane - CE_LOGITS];
            if (j + 1 >= n) b.y = 0u;
            if (j + 2 >= n) b.z = 0u;
            if (j + 3 >= n) b.w = 0u;
        }
        e[lane] = b;
    }
    if (lane == 0) {
        t.claim[idx] = CACHE_NO_CLAIM;
        atomicAdd(&cc->stores, 1ull);
    }
}

int cache_reset_claims(const CacheTab& t, hipStream_t st) {
    KV_HIP(hipMemsetAsync(t.claim, CACHE_NO_CLAIM & 0xff, ((size_t)t.mask + 1) * sizeof(int), st));
    return KV_OK;
}

int cache_clear(const CacheTab& t, hipStream_t st) {
    KV_HIP(hipMemsetAsync(t.ent, 0xff, ((size_t)t.mask + 1) * KV_CACHE_ENTRY_BYTES, st));
    return cache_reset_claims(t, st);
}

int cache_probe(const CacheTab& ta, const CacheTab& tb, const Slot* slots, int L, int nmin, const SearchWs& w, int rows,
                int* hit, int* cidx, CacheCtr* cc, hipStream_t st) {
    hipLaunchKernelGGL(k_cache_probe, dim3(rows), dim3(64), 0, st, ta, tb, slots, L, nmin, w.lboards, w.lmoves, w.lcnt,
                       w.llogits, w.lvalues, hit, cidx, cc);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

int cache_store(const CacheTab& ta, const CacheTab& tb, const Slot* slots, int L, int nmin, const SearchWs& w, int rows,
                const int* hit, const int* cidx, CacheCtr* cc, hipStream_t st) {
    hipLaunchKernelGGL(k_cache_store, dim3(rows), dim3(64), 0, st, ta, tb, slots, L, nmin, w.lboards, w.lmoves, w.lcnt,
                       w.llogits, w.lvalues, hit, cidx, cc);
    KV_HIP(hipGetLastError());
    return KV_OK;
}

}  // namespace kv

extern "C" {

int kv_dev_eval_cache(int device, int entries, const int8_t* boards, const uint16_t* moves, const int* counts,
                      const uint32_t* logits, const uint32_t* values, int n_rows, const int* step_len, int n_steps,
                      int32_t* hit, uint32_t* out_logits, uint32_t* out_values, int64_t* counters) {
    KV_REQUIRE(boards && moves && counts && logits && values && step_len && hit && out_logits && out_values &&
                   n_rows > 0 && n_steps > 0,
               KV_EINVAL, "kv_dev_eval_cache: bad arguments");
    KV_REQUIRE(entries >= 64 && entries <= (1 << 24) && (entries & (entries - 1)) == 0, KV_EINVAL,
               "kv_dev_eval_cache: entries %d must be a power of two in [64, 2^24]", entries);
    long long total = 0;
    for (int s = 0; s < n_steps; ++s) {
        KV_REQUIRE(step_len[s] > 0, KV_EINVAL, "kv_dev_eval_cache: step %d of %d rows", s, step_len[s]);
        total += step_len[s];
    }
    KV_REQUIRE(total == n_rows, KV_EINVAL, "kv_dev_eval_cache: the steps hold %lld rows, n_rows is %d", total, n_rows);
    for (int r = 0; r < n_rows; ++r)
        KV_REQUIRE(counts[r] >= 0 && counts[r] <= kv::MAXM, KV_EINVAL, "kv_dev_eval_cache: row %d has %d moves", r,
                   counts[r]);
    KV_HIP(hipSetDevice(device));
    const size_t R = (size_t)n_rows;
    kv::DevBuf<int8_t> b;
    kv::DevBuf<uint16_t> m;
    kv::DevBuf<int> c, h, ci, claim;
    kv::DevBuf<float> pl, pv, ol, ov;
    kv::DevBuf<uint4> ent;
    kv::DevBuf<kv::CacheCtr> cc;
    KV_HIP(b.alloc(R * 64));
    KV_HIP(m.alloc(R * kv::MAXM));
    KV_HIP(c.alloc(R));
    KV_HIP(h.alloc(R));
    KV_HIP(ci.alloc(R));
    KV_HIP(pl.alloc(R * kv::MAXM));
    KV_HIP(pv.alloc(R));
    KV_HIP(ol.alloc(R * kv::MAXM));
    KV_HIP(ov.alloc(R));
    KV_HIP(ent.alloc((size_t)entries * kv::CACHE_ENTRY_U4));
    KV_HIP(claim.alloc(entries));
    KV_HIP(cc.alloc(1));
    KV_HIP(hipMemcpy(b.p, boards, R * 64, hipMemcpyHostToDevice));
    KV_HIP(hipMemcpy(m.p, moves, R * kv::MAXM * sizeof(uint16_t), hipMemcpyHostToDevice));
    KV_HIP(hipMemcpy(c.p, counts, R * sizeof(int), hipMemcpyHostToDevice));
    KV_HIP(hipMemcpy(pl.p, logits, R * kv::MAXM * sizeof(float), hipMemcpyHostToDevice));
    KV_HIP(hipMemcpy(pv.p, values, R * sizeof(float), hipMemcpyHostToDevice));
    KV_HIP(hipMemset(ol.p, 0xff, R * kv::MAXM * sizeof(float)));
    KV_HIP(hipMemset(ov.p, 0xff, R * sizeof(float)));
    KV_HIP(hipMemset(h.p, 0, R * sizeof(int)));
    KV_HIP(hipMemset(ci.p, 0, R * sizeof(int)));
    KV_HIP(hipMemset(cc.p, 0, sizeof(kv::CacheCtr)));
    kv::CacheTab t;
    t.ent = ent.p;
    t.claim = claim.p;
    t.mask = (unsigned)entries - 1;
    int rc = kv::cache_clear(t, 0);
    if (rc) return rc;
    size_t r0 = 0;
    for (int s = 0; s < n_steps; ++s) {
        const int n = step_len[s];
        kv::SearchWs probe = {}, store = {};  // the probe writes the outputs, the store reads the given payload
        probe.lboards = store.lboards = b.p + r0 * 64;
        probe.lmoves = store.lmoves = m.p + r0 * kv::MAXM;
        probe.lcnt = store.lcnt = c.p + r0;
        probe.llogits = ol.p + r0 * kv::MAXM;
        probe.lvalues = ov.p + r0;
        store.llogits = pl.p + r0 * kv::MAXM;
        store.lvalues = pv.p + r0;
        if ((rc = kv::cache_probe(t, t, nullptr, 1, 0, probe, n, h.p + r0, ci.p + r0, cc.p, 0))) return rc;
        if ((rc = kv::cache_store(t, t, nullptr, 1, 0, store, n, h.p + r0, ci.p + r0, cc.p, 0))) return rc;
        r0 += (size_t)n;
    }
    KV_HIP(hipDeviceSynchronize());
    KV_HIP(hipMemcpy(hit, h.p, R * sizeof(int), hipMemcpyDeviceToHost));
    KV_HIP(hipMemcpy(out_logits, ol.p, R * kv::MAXM * sizeof(float), hipMemcpyDeviceToHost));
    KV_HIP(hipMemcpy(out_values, ov.p, R * sizeof(float), hipMemcpyDeviceToHost));
    if (counters) {
        kv::CacheCtr host;
        KV_HIP(hipMemcpy(&host, cc.p, sizeof(host), hipMemcpyDeviceToHost));
        counters[0] = (int64_t)host.probes;
        counters[1] = (int64_t)host.hits;
        counters[2] = (int64_t)host.stores;
    }
    return KV_OK;
}

}  // extern "C"
