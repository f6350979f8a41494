// F(8x8) Winograd GEMMs on the int8 matrix cores with exact integer
// accumulation (KV_PATH_WINO88_I8): the fp64 Winograd domain of kv_wino88d.h
// (U, V, M and both transforms in fp64) with the GEMM's products taken from
// int8 digits instead of v_mfma_f64.
//
// Every row of V (point xi, board) and of U (xi, output channel) -- K input
// channels -- is scaled by a power of two 2^-e to |a| < 255/256 (e from the
// row's largest magnitude, i8_row_exponent) and split into 5 signed int8 digits,
//     a * 2^-e = sum_i d_i * 2^(-7(i+1)) + rest,  |d_0| <= 127, |d_i| <= 64,
//     |rest| <= 2^-36,
// d_i = rint(t_i), t_{i+1} = 128 (t_i - d_i), t_0 = 128 a 2^-e (each step exact
// in fp64). The product keeps the digit pairs with i + j <= S - 1, S = 5:
//     M = 2^(e_v + e_u - 14) * sum_{l < S} 2^(-7l) * sum_{i+j=l} (D_i . E_j)
// where each D_i . E_j is one v_mfma_i32_32x32x32_i8 chain over K (exact in
// int32: |level l| <= 5 * 512 * 127^2 < 2^31), and the five level sums are
// combined in fp64 exactly (at most 51 significant bits). What it computes:
// per-row 35-bit block fixed point (each value cut to the multiples of
// 2^(e-36) of its row's exponent), the 15 digit pairs i + j <= 4 of the 25
// (the 10 dropped pairs weigh < 2^-42 of the row maxima's product each), exact
// int32 levels, one exact fp64 combine. Nothing in the GEMM rounds, so M is
// independent of k order, tile shape and batch by construction. Its distance
// from the fp64 product of the unsplit rows is bounded per element by the
// truncation (|rest| <= 2^-36 per value) plus the dropped pairs:
// tests/test_wino_i8_gpu.py::test_i8_gemm_within_derived_bound_of_fp64_product.
// 15 int8 products at 32x the fp32 MFMA rate (the int8 rate is 2x bf16's)
// against v_mfma_f64 at half the fp32 rate: a ~4x higher ceiling than the fp64
// GEMM it replaces, at the same accuracy (host emulation on the stress weights:
// max |dlogit| 3.0e-6 against the fp64 path's 2.9e-6, profiles/r04_ozaki_emulation.log).
//
// Layouts: digit planes [slab xi][K / 32][digit 5][row][32] int8 (plane (xi, kc,
// d): digit d of channels 32 kc .. 32 kc + 31 of every row), exponents
// [xi][row] int32.
#pragma once
#include <hip/hip_runtime.h>

#include "kv_common.h"
#include "kv_wino88.h"   // w88_bt, wino88_out_plane
#include "kv_wino88d.h"  // f64x2

namespace kv {

constexpr int kI8Digits = 5;    // digits per value in the fp64 domain (KV_PATH_WINO88_I8); the GEMM keeps
                                // the digit pairs i + j < digits
constexpr int kI8DigitsF32 = 4; // in the fp32 domain (KV_PATH_WINO88_I8F32): 28 bits, an fp32 value exactly
                                // when it is within 2^-4 of its row's max

typedef int i8x16_t __attribute__((ext_vector_type(4)));   // 16 int8 in 4 dwords (MFMA A / B)
typedef int i32x16_t __attribute__((ext_vector_type(16)));  // 32x32 int32 accumulator block

// Row exponent from the high word m of the row's largest |value| (biased exponent E in bits 20-30):
// 2^(e-1) <= max < 2^e, e = E - 1022, plus one when the max's top 7 fraction bits are all ones (max >=
// 255/256 * 2^e): then every t = a 2^-e < 255/256, so the first digit rint(128 t) <= 127 and every later
// remainder is within 1/2 -- no digit needs a clamp (35 bits kept on all but ~0.8 % of rows, 34 on
// those). An all-zero row gets e = 0 (digits 0).
__device__ inline int i8_row_exponent(unsigned m) {
    if (!m) return 0;
    return (int)(m >> 20) - 1022 + ((m & 0xFE000u) == 0xFE000u ? 1 : 0);
}

// fp32 form: m = the bits of the row's largest |float| (exponent in bits 23-30, top 7 fraction bits 16-22)
__device__ inline int i8_row_exponent_f32(unsigned m) {
    if (!m) return 0;
    return (int)(m >> 23) - 126 + ((m & 0x7F0000u) == 0x7F0000u ? 1 : 0);
}

// Radix-256 form (KV_PATH_WINO88_I8R: 4 digits of 8 bits): e with max < 127/128 2^e (one more than the
// plain rule when the max's top 7 fraction bits are >= 126), so every N = rint(v 2^(31-e)) has |N| < 127/128
// 2^31 and its balanced base-256 digits d_0 (most significant) .. d_3, N = sum_i d_i 2^(8 (3 - i)), are all
// in [-128, 127] with |d_0| <= 127: v ~ 2^(e-7) sum_i d_i 2^(-8 i), 31-bit block fixed point.
__device__ inline int i8_row_exponent_r8(unsigned m) {
    if (!m) return 0;
    return (int)(m >> 20) - 1022 + ((m & 0xFE000u) >= 0xFC000u ? 1 : 0);
}

// fp32 form of the radix-256 rule (KV_PATH_WINO88_I8F32R3): m = the bits of the row's largest |float|; one more
// when its top 6 fraction bits are all ones (max >= 127/128 2^e)
__device__ inline int i8_row_exponent_f32r(unsigned m) {
    if (!m) return 0;
    return (int)(m >> 23) - 126 + ((m & 0x7E0000u) == 0x7E0000u ? 1 : 0);
}

// The 3 radix-256 digits of v under e (KV_PATH_WINO88_I8F32R3: the fp32 tower's 24-bit block fixed point), in
// the row lines' 4 digit slots: N = rint(v 2^(23-e)) by an fp64 magic-number add (ties to even; exact for
// |N| < 2^31 -- the fp32 magic add would round at |t| >= 2^22), |N| < 127/128 2^23 under the radix-256 rule, so
// the balanced digits d_0 (most significant) .. d_2, N = d_0 2^16 + d_1 2^8 + d_2, are the bytes of
// N + 0x808080 with their top bits flipped; packed byte d = d_d (slot 3 zero): v ~ 2^(e-7) sum_d d_d 2^(-8 d).
__device__ inline unsigned i8_digits_r3(double v, int e) {
#pragma clang fp contract(off)
    constexpr double kMagic = 6755399441055744.0;  // 1.5 * 2^52
    const unsigned n = (unsigned)__double_as_longlong(ldexp(v, 23 - e) + kMagic);
    return __builtin_amdgcn_perm(0u, (n + 0x808080u) ^ 0x808080u, 0x0c000102u);
}

// the 4 radix-256 digits of v under e, packed: byte k = d_(3-k) (two's complement). N by a magic-number add
// (rint, ties to even; the low word of t + 1.5 2^52 is N's two's complement for |t| < 2^31); then the balanced
// digits are the bytes of N + 0x80808080 (each d + 128 in [0, 255], no carry out) with their top bits flipped.
__device__ inline unsigned i8_digits_r8(double v, int e) {
#pragma clang fp contract(off)
    constexpr double kMagic = 6755399441055744.0;  // 1.5 * 2^52
    const unsigned n = (unsigned)__double_as_longlong(ldexp(v, 31 - e) + kMagic);
    return (n + 0x80808080u) ^ 0x80808080u;
}

// D digits of v under exponent e: t = 128 v 2^-e, d = rint(t), t = 128 (t - d), each step exact (in fp32
// too: t never has more significant bits than v)
template <int D, class T>
__device__ inline void i8_digits(T v, int e, int (&d)[D]) {
    T t = ldexp(v, 7 - e);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const T q = rint(t);
        d[i] = (int)q;
        t = (t - q) * (T)128;
    }
}

// max over the 32 lanes of each half-wave of v, by DPP-modified max operations (no selects, no LDS-pipe
// shuffle): xor 1 and xor 2 within quads, the half-row and row mirrors (every lane then holds its 16-lane
// row's max), then row_bcast:15 into rows 1 and 3 -- lanes 16-31 end with the max of lanes 0-31, lanes
// 48-63 with the max of lanes 32-63.
__device__ inline unsigned i8_half_max_dpp(unsigned v) {
    // old = 0 (the identity of an unsigned max) so the compiler folds each DPP move into its max
    unsigned t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);  // quad_perm 1,0,3,2
    v = v > t ? v : t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);  // quad_perm 2,3,0,1
    v = v > t ? v : t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v = v > t ? v : t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    v = v > t ? v : t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    return v > t ? v : t;
}

// i8_digits<D> of an fp64 v with each rint(t) as t + 1.5 * 2^52 (|t| <= 128: the add rounds to the integer,
// ties to even, as rint) -- q[i]'s low byte is digit i's two's complement; q - 1.5 * 2^52 is rint(t) exactly, so
// the remainders are i8_digits's: the same digits with full-rate fp64 adds instead of v_rndne_f64 +
// v_cvt_i32_f64
template <int D>
__device__ inline void i8_digits_magic(double v, int e, unsigned (&q)[D]) {
#pragma clang fp contract(off)
    constexpr double kMagic = 6755399441055744.0;  // 1.5 * 2^52
    double t = ldexp(v, 7 - e);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double qf = t + kMagic;
        q[i] = (unsigned)__double_as_longlong(qf);
        if (i + 1 < D) t = (t - (qf - kMagic)) * 128.0;
    }
}

// The 4 digits of an fp32 v under exponent e (i8_digits<4>) packed into one dword, digit d in byte d: each
// rint(t) as t + 1.5 * 2^23 (|t| <= 128: the add rounds to the integer, ties to even, as rintf) whose low byte
// is the digit's two's complement; q - 1.5 * 2^23 is rint(t) exactly, so t - rint(t) and the x128 are the
// same operations as i8_digits's -- the same digits, without the float -> int conversions.
__device__ inline unsigned i8_digits4_packed(float v, int e) {
#pragma clang fp contract(off)
    constexpr float kMagic = 12582912.0f;  // 1.5 * 2^23
    float t = ldexpf(v, 7 - e);
    unsigned q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float qf = t + kMagic;
        q[i] = __float_as_uint(qf);
        if (i < 3) t = (t - (qf - kMagic)) * 128.0f;
    }
    const unsigned lo = __builtin_amdgcn_perm(q[1], q[0], 0x0c0c0400u);  // [q0.b0, q1.b0, 0, 0]
    const unsigned hi = __builtin_amdgcn_perm(q[3], q[2], 0x0c0c0400u);
    return lo | hi << 16;
}

// lane quad q = lane & 3 holds P = digits 0..3 of its channel (byte d = digit d); returns digit q of the
// quad's 4 channels (byte j = channel 4 (lane / 4) + j)
__device__ inline unsigned i8_quad_transpose(unsigned P, int lane) {
    const unsigned q1 = (unsigned)__builtin_amdgcn_mov_dpp((int)P, 0xB1, 0xF, 0xF, false);  // quad_perm 1,0,3,2
    // even lane: [P.0 q1.0 P.2 q1.2], odd: [q1.1 P.1 q1.3 P.3]
    const unsigned R = __builtin_amdgcn_perm(q1, P, (lane & 1) ? 0x03070105u : 0x06020400u);
    const unsigned r2 = (unsigned)__builtin_amdgcn_mov_dpp((int)R, 0x4E, 0xF, 0xF, false);  // quad_perm 2,3,0,1
    // lanes 0, 1 of the quad: [R.0 R.1 r2.0 r2.1], lanes 2, 3: [r2.2 r2.3 R.2 R.3]
    return __builtin_amdgcn_perm(r2, R, (lane & 2) ? 0x03020706u : 0x05040100u);
}

// The digits and exponent of `nslab` slabs of n rows of K fp64 values: row r of
// slab x is src[(x * slab_rows + r) * K ...]; digit d of its channels
// [32 kc, 32 kc + 32) goes to plane (x, kc, d) of dst -- 32 bytes at
// (((x * K/32 + kc) * 5 + d) * slab_rows + r) * 32 -- and the exponent to
// ex[x * slab_rows + r]. One wave per row; lane l holds channels
// [l * K/64, (l + 1) * K/64). RL (row lines, 4 digits only): digit d of the
// 32 channels goes to (((x * K/32 + kc) * slab_rows + r) * 4 + d) * 32 instead
// -- the 4 digits of one row's chunk are one 128-byte line.
// R3 (KV_PATH_WINO88_I8F32R3; row lines): 3 radix-256 digits (i8_digits_r3) under the radix-256 exponent rule of
// the fp32 or fp64 rows, in 96-byte lines (((x * K/32 + kc) * slab_rows + r) * 3 + d) * 32
template <int K, class T, int D, bool RL = false, bool R8 = false, bool R3 = false>
__global__ __launch_bounds__(256) void wino88i_slice_kernel(const T* __restrict__ src, int n, int slab_rows,
                                                            int nslab, int8_t* __restrict__ dst,
                                                            int* __restrict__ ex) {
    static_assert(K == 256 || K == 512, "rows of 256 or 512 channels");
    static_assert(!RL || D == 4, "row lines hold 4 digits");
    static_assert(!R8 || (D == 4 && sizeof(T) == 8), "radix 256: 4 digits of fp64 rows");
    static_assert(!R3 || (D == 4 && RL && !R8), "3 radix-256 digits in 96-byte row lines");
    constexpr int CPL = K / 64;  // 4 or 8 channels per lane
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= n * nslab) return;  // whole waves
    const int x = gw / n, r = gw % n;
    const size_t row = (size_t)x * slab_rows + r;
    const T* s = src + row * K + lane * CPL;
    T v[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) v[i] = s[i];
    // the (high) words of |v| order like |v|: their max carries the row's largest exponent
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        unsigned hw;
        if constexpr (sizeof(T) == 8)
            hw = (unsigned)(__double_as_longlong(v[i]) >> 32) & 0x7fffffffu;
        else
            hw = __float_as_uint(v[i]) & 0x7fffffffu;
        m = hw > m ? hw : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o, 64);
        m = t > m ? t : m;
    }
    const int e = (R8 || (R3 && sizeof(T) == 8)) ? i8_row_exponent_r8(m)
                  : R3                              ? i8_row_exponent_f32r(m)
                  : sizeof(T) == 8                  ? i8_row_exponent(m)
                                                    : i8_row_exponent_f32(m);
    if (lane == 0) ex[row] = e;
    unsigned long long pk[D] = {};
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        int dg[D];
        if constexpr (R8) {
            const unsigned P = i8_digits_r8((double)v[i], e);
#pragma unroll
            for (int d = 0; d < D; ++d) dg[d] = (int)(signed char)(P >> (8 * (D - 1 - d)));
        } else if constexpr (R3) {
            const unsigned P = i8_digits_r3((double)v[i], e);  // byte d = digit d, slot 3 zero
#pragma unroll
            for (int d = 0; d < D; ++d) dg[d] = (int)(signed char)(P >> (8 * d));
        } else {
            i8_digits<D>(v[i], e, dg);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) pk[d] |= (unsigned long long)(unsigned char)(signed char)dg[d] << (8 * i);
    }
    const int c = lane * CPL, kc = c / 32;
    constexpr int LW = R3 ? 3 * 32 : D * 32;  // row-line bytes (R3: the 3 digits only)
    int8_t* o = RL ? dst + (((size_t)x * (K / 32) + kc) * slab_rows + r) * LW + (c % 32)
                   : dst + ((((size_t)x * (K / 32) + kc) * D) * slab_rows + r) * 32 + (c % 32);
#pragma unroll
    for (int d = 0; d < (R3 ? 3 : D); ++d) {
        int8_t* od = o + (size_t)d * (RL ? 32 : slab_rows * 32);
        if constexpr (CPL == 8)
            *(unsigned long long*)od = pk[d];
        else
            *(unsigned*)od = (unsigned)pk[d];
    }
}

// The GEMM: a workgroup computes 128 rows x 128 output channels of one point
// with 8 waves of 32 x 64 (1 x 2 accumulator blocks per digit level). K
// streams in 32-k stages; a stage is the 5 digit planes of the tile's rows
// (5 x 128 x 32 B of V, the same of U), copied global -> LDS by
// global_load_lds (1 KiB = 32 rows per wave-instruction, 5 per wave per
// stage) into a ring of 3 LDS buffers: the copies of stage kt + 2 run during
// stage kt's MFMAs, retired by a counted s_waitcnt vmcnt and a raw barrier.
// The LDS image is linear; the two 16-byte halves of a row are swapped when
// bit 3 of the row is set (on the global source address), so each ds_read_b128
// lane group reads 16 distinct 4-bank groups.
template <int D>
struct Wino88iTile {
    static constexpr int WR = 4, WC = 2, MT = 1, NT = 2;
    static constexpr int THREADS = WR * WC * 64;
    static constexpr int WM = WR * MT * 32, WN = WC * NT * 32;  // 128 x 128
    static constexpr int PLANE = 128 * 32;                      // bytes of one digit plane of a tile
    static constexpr int STAGE = 2 * D * PLANE;                 // A planes then B planes: 8 D KiB
    static constexpr int GL = STAGE / 1024 / (THREADS / 64);    // global_load_lds per wave and stage (= D)
};

__device__ inline int i8_lds_half(int row, int h) { return 16 * (h ^ ((row >> 3) & 1)); }

// RL layout in LDS: row r of an operand is its 128-byte line (16-byte chunk c = 2 d + half of digit d),
// chunk c at position c ^ ((r >> 1) & 7): a ds_read_b128 lane group (rows {0-3, 12-15, 20-27} or {4-11,
// 16-19, 28-31} of a 32-row block, one chunk) hits 16 distinct 16-byte bank groups -- even rows in the
// first 128 bytes of the 256-byte bank window, odd rows in the second, 8 distinct positions each. (A
// chunk-major image with one base + 256 d per digit needs lanes 128 bytes apart in the copy: the GEMM
// ran 551 us against 523, profiles/r04_i8f32_rowlines_ab.log.)
__device__ inline int i8_rl_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ ((row >> 1) & 7)); }

// The fp32 tower's GEMM on 4 digits in row lines: M[xi] (fp32 [xi][stride rows][cout]) = V[xi] x U[xi]^T from the
// digits (see the header comment). V8: row lines [xi][K/32][stride][4][32], U8: [xi][K/32][cout][4][32] -- a
// stage of a tile is one contiguous 16 KiB block per operand, and one workgroup of the fused output kernel (one
// board) writes whole lines. XCD-aware tile order as kv_wino.h's wino_gemm_kernel. One loop over stage barriers
// in which a wave's MFMAs for stage k are split in two halves: h1(k) = B digits 0-1 (14 of 20 MFMAs per wave),
// h2(k) = B digits 2-3 (6). After barrier k a wave reads stage k's A digits and first B digit while it runs
// h2(k - 1) from registers (the A digits 0-1 and B digits 2-3 of stage k - 1, kept), then h1(k). Every LDS read
// of stage k happens between barriers k and k + 1, so stage k + 2's copies go into stage k - 1's buffer right
// after barrier k (3 buffers, two stages in flight).
#ifndef KV_LAG_OPAQUE
// 1: the lagging operands redefined opaquely after the pre-barrier lgkmcnt(0) (so the compiler's waitcnt pass
// cannot make the first lagging MFMA wait for the new stage's LDS reads). Bit-identical either way; measured
// (profiles/r06_gemm_opaque_lj_ab.log) neutral on the 4-digit tower and 0.6-1.5 % slower forward on R3: off.
#define KV_LAG_OPAQUE 0
#endif
template <int K>
__global__ __launch_bounds__(512) void wino88i32_gemm_lag_kernel(const int8_t* __restrict__ V8,
                                                                 const int* __restrict__ ev,
                                                                 const int8_t* __restrict__ U8,
                                                                 const int* __restrict__ eu, float* __restrict__ M,
                                                                 int rows, int cout, int stride) {
    constexpr int S = 4, NBUF = 3, LJ = 2;  // B digits LJ.. lag
    using T = Wino88iTile<S>;
    constexpr int NT = T::NT, WM = T::WM, WN = T::WN, GL = T::GL;
    constexpr int NK = K / 32;
    constexpr int NA = S - LJ;  // A digits the lagging half uses (0 .. S - LJ - 1)
    static_assert(GL == 4 && NK >= 3, "4 pieces per wave and stage");

    extern __shared__ __attribute__((aligned(16))) i8x16_t lds_i8l[];
    char* const L0 = (char*)lds_i8l;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WC, wn = wave % T::WC;
    const int CT = cout / WN, RT = rows / WM;
    const int nwg = (int)gridDim.x;  // a multiple of 8
    const int idx = (int)(blockIdx.x & 7) * (nwg >> 3) + (int)(blockIdx.x >> 3);
    const int xi = idx / (CT * RT);
    const int n_base = (idx % CT) * WN;
    const int r_base = ((idx / CT) % RT) * WM;

    const int op = (wave * GL) / (4 * S);
    const size_t rstride = op ? (size_t)cout : (size_t)stride;
    const int8_t* gbase = op ? U8 + (((size_t)xi * NK) * cout + (size_t)n_base) * 128
                             : V8 + (((size_t)xi * NK) * stride + (size_t)r_base) * 128;
    const size_t sstep = rstride * 128;
    const int rl_off0 = (lane >> 3) * 128 + 16 * ((lane & 7) ^ (lane >> 4));
    const int rl_off1 = (lane >> 3) * 128 + 16 * ((lane & 7) ^ (lane >> 4) ^ 4);
    auto issue1 = [&](int g, int kt) {
        const int q = wave * GL + g, rg8 = q % 16;
        __builtin_amdgcn_global_load_lds(
            (const void*)(gbase + kt * sstep + (size_t)rg8 * 1024 + ((rg8 & 1) ? rl_off1 : rl_off0)),
            (__attribute__((address_space(3))) void*)(L0 + (kt % NBUF) * T::STAGE + op * S * T::PLANE + rg8 * 1024),
            16, 0, 0);
    };

    const int lr = lane & 31, lh = lane >> 5;
    const int arow = wm * 32 + lr;
    int aoffr[S], boffr[NT][S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        aoffr[i] = i8_rl_off(arow, 2 * i + lh);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) boffr[nt][i] = S * T::PLANE + i8_rl_off(wn * NT * 32 + nt * 32 + lr, 2 * i + lh);
    }

    i32x16_t acc[S][NT];
#pragma unroll
    for (int l = 0; l < S; ++l)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[l][nt] = i32x16_t{};
    // h2 of a stage: B digits j >= LJ with the A digits i < S - j
    i8x16_t pa[NA] = {}, pb[S - LJ][NT] = {};
    auto h2 = [&](const i8x16_t (&x)[NA], const i8x16_t (&y)[S - LJ][NT]) {
#pragma unroll
        for (int j = LJ; j < S; ++j)
#pragma unroll
            for (int i = 0; i + j < S; ++i)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[i + j][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x[i], y[j - LJ][nt], acc[i + j][nt], 0, 0, 0);
    };

    issue1(0, 0); issue1(1, 0); issue1(2, 0); issue1(3, 0);
    issue1(0, 1); issue1(1, 1); issue1(2, 1); issue1(3, 1);
    for (int kt = 0; kt < NK; ++kt) {
        // stage kt landed: only stage kt + 1's copies may still be in flight; lgkmcnt(0): the lagging B digits
        // of stage kt - 1 were read from the buffer stage kt + 2's copies overwrite once every wave passes this
        // barrier, and their reads are only waited for at the MFMAs after it (a formal WAR race)
        if (kt + 1 < NK)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GL) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#if KV_LAG_OPAQUE  // the lagging operands are in registers (wino88i32_gemm_lagt_kernel)
#pragma unroll
        for (int i = 0; i < NA; ++i) asm volatile("" : "+v"(pa[i]));
#pragma unroll
        for (int jb = 0; jb < S - LJ; ++jb)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(pb[jb][nt]));
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char* buf = L0 + (kt % NBUF) * T::STAGE;
        i8x16_t a[S], b[S][NT];
#pragma unroll
        for (int i = 0; i < S; ++i) a[i] = *(const i8x16_t*)(buf + aoffr[i]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[0][nt] = *(const i8x16_t*)(buf + boffr[nt][0]);
        if (kt > 0) h2(pa, pb);  // under the reads above
        // stage kt + 2 into stage kt - 1's buffer, two pieces at the start, two after the first B digit
        if (kt + 2 < NK) {
            issue1(0, kt + 2);
            issue1(1, kt + 2);
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (j + 1 < S) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b[j + 1][nt] = *(const i8x16_t*)(buf + boffr[nt][j + 1]);
            }
            if (j < LJ) {
#pragma unroll
                for (int i = 0; i + j < S; ++i)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[i + j][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j][nt], acc[i + j][nt], 0, 0, 0);
            }
            if (j == 0 && kt + 2 < NK) {
                issue1(2, kt + 2);
                issue1(3, kt + 2);
            }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) pa[i] = a[i];
#pragma unroll
        for (int j = LJ; j < S; ++j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) pb[j - LJ][nt] = b[j][nt];
    }
    h2(pa, pb);

    // epilogue: D col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int* evx = ev + (size_t)xi * stride + r_base + wm * 32;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n_base + wn * NT * 32 + nt * 32 + lr;
        const int ec = eu[(size_t)xi * cout + col] - 14;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            double m = (double)acc[S - 1][nt][r];
#pragma unroll
            for (int l = S - 2; l >= 0; --l) m = __builtin_fma(m, 0.0078125, (double)acc[l][nt][r]);  // exact
            M[((size_t)xi * stride + r_base + wm * 32 + row) * cout + col] = (float)ldexp(m, evx[row] + ec);
        }
    }
}

// wino88i32_gemm_lag_kernel with TPW tiles per workgroup: the copy ring runs across the tile boundaries (a tile's
// first two stages go out during the previous tile's last two), so every tile after a workgroup's first starts
// with its operands in LDS. kv_nn.hip picks TPW so the workgroups fill whole rounds in no more tile-times than
// single tiles: C3's 6,400 tiles as 5 rounds of 5-tile workgroups (497 vs 511 us), C2's 800 as one round of
// 4-tile workgroups (72 vs 76 us; profiles/r05_i8gemm_lagt_ab.log, r05_i8gemm_tpw5_ab.log). The tile loop is
// unrolled (a runtime count recomputing tile coordinates per copy ran 13 % slower,
// profiles/r05_i8gemm_tpw_runtime_ab.log). Tile j of workgroup w is virtual
// block w + j * gridDim in the XCD-aware order (the same XCD). At the first stage of a later tile a wave waits
// for that stage's pieces with the previous tile's 32 M stores still allowed in flight. Same products, same bits.
#ifndef KV_I8F32_LJ
#define KV_I8F32_LJ 2
#endif
// STAMP (a diagnostic build, never the product's): wave 0 of each workgroup records the shader clock
// (s_memtime) and the 100 MHz constant clock (s_memrealtime) at its start and end into stamps[4 * block] -- a
// buffer of its own that no other code reads; kv_dev_gemm_clock turns them into the clock the chip held.
// ND: digit levels (4; round 6's ND = 3 form for KV_PATH_WINO88_I8F32R3 retired with R3's 128-byte lines: R3 runs
// wino88i32_gemm_r3k64_kernel on 96-byte lines).
// KV_COPY_SADDR (1): the ring's copies address a wave-uniform 64-bit base plus an unsigned 32-bit lane offset,
// so they issue in the scalar-base form (one address VGPR per lane); 0: a 64-bit VGPR address pair per lane.
#ifndef KV_COPY_SADDR
#define KV_COPY_SADDR 1
#endif
// NB: buffers of the copy ring (NB x 32 KiB of LDS), so NB - 1 stages are in flight past the one being read: the
// copies of stage k + NB - 1 go into stage k - 1's buffer right after barrier k.
template <int N>
__device__ __forceinline__ void vm_lgkm_wait() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
template <int K, int TPW, int LJ = KV_I8F32_LJ, bool STAMP = false, int ND = 4, int NB = 3>
__global__ __launch_bounds__(512) void wino88i32_gemm_lagt_kernel(const int8_t* __restrict__ V8,
                                                                  const int* __restrict__ ev,
                                                                  const int8_t* __restrict__ U8,
                                                                  const int* __restrict__ eu, float* __restrict__ M,
                                                                  int rows, int cout, int stride,
                                                                  unsigned long long* __restrict__ stamps) {
    unsigned long long t0 = 0, r0 = 0;
    if constexpr (STAMP) {
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    constexpr int S = 4, NBUF = NB, PD = NB - 1;  // PD: prefetch distance in stages
    using T = Wino88iTile<S>;
    constexpr int NT = T::NT, WM = T::WM, WN = T::WN, GL = T::GL;
    constexpr int NK = K / 32, NS = TPW * NK;
    constexpr int NA = ND - LJ;
    static_assert(GL == 4 && NK >= 3 && LJ >= 1 && LJ < ND && ND == 4, "4 pieces per wave and stage, 4 digits");
    static_assert(NB >= 3 && NB <= 5 && PD < NK, "ring of 3-5 stage buffers (at most 160 KiB)");
    constexpr double kStep = ND == 4 ? 0.0078125 : 0.00390625;  // level weight: radix 128 / 256

    extern __shared__ __attribute__((aligned(16))) i8x16_t lds_i8t[];
    char* const L0 = (char*)lds_i8t;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WC, wn = wave % T::WC;
    const int CT = cout / WN, RT = rows / WM;
    const int nwg = (int)gridDim.x, nv = nwg * TPW;  // nwg a multiple of 8
    int xis[TPW], nbs[TPW], rbs[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int vb = (int)blockIdx.x + j * nwg;
        const int idx = (vb & 7) * (nv >> 3) + (vb >> 3);
        xis[j] = idx / (CT * RT);
        nbs[j] = (idx % CT) * WN;
        rbs[j] = ((idx / CT) % RT) * WM;
    }

    const int wu = __builtin_amdgcn_readfirstlane(wave);  // wave-uniform: scalar tile bases
    const int op = (wu * GL) / (4 * S);
    const size_t sstep = (op ? (size_t)cout : (size_t)stride) * 128;
    const int8_t* gb[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
        gb[j] = op ? U8 + (((size_t)xis[j] * NK) * cout + (size_t)nbs[j]) * 128
                   : V8 + (((size_t)xis[j] * NK) * stride + (size_t)rbs[j]) * 128;
    const int rl_off0 = (lane >> 3) * 128 + 16 * ((lane & 7) ^ (lane >> 4));
    const int rl_off1 = (lane >> 3) * 128 + 16 * ((lane & 7) ^ (lane >> 4) ^ 4);
    auto issue1 = [&](int g, int s) {  // piece g of global stage s (tile s / NK, stage s % NK)
        const int q = wu * GL + g, rg8 = q % 16;
        const int j = s / NK, kt = s - j * NK;
        const int8_t* base = gb[0];
#pragma unroll
        for (int jj = 1; jj < TPW; ++jj) base = j == jj ? gb[jj] : base;
        const int8_t* const sb = base + kt * sstep + (size_t)rg8 * 1024;  // wave-uniform
#if KV_COPY_SADDR
        const void* src = (const void*)(sb + (unsigned)((rg8 & 1) ? rl_off1 : rl_off0));
#else
        const void* src = (const void*)(sb + (size_t)((rg8 & 1) ? rl_off1 : rl_off0));
#endif
        __builtin_amdgcn_global_load_lds(
            src, (__attribute__((address_space(3))) void*)(L0 + (s % NBUF) * T::STAGE + op * S * T::PLANE + rg8 * 1024),
            16, 0, 0);
    };

    const int lr = lane & 31, lh = lane >> 5;
    const int arow = wm * 32 + lr;
    int aoffr[ND], boffr[NT][ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        aoffr[i] = i8_rl_off(arow, 2 * i + lh);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) boffr[nt][i] = S * T::PLANE + i8_rl_off(wn * NT * 32 + nt * 32 + lr, 2 * i + lh);
    }

#pragma unroll
    for (int p = 0; p < PD; ++p) {
        issue1(0, p); issue1(1, p); issue1(2, p); issue1(3, p);
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        i32x16_t acc[ND][NT];
#pragma unroll
        for (int l = 0; l < ND; ++l)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[l][nt] = i32x16_t{};
        i8x16_t pa[NA] = {}, pb[ND - LJ][NT] = {};
        auto h2 = [&]() {
#pragma unroll
            for (int jb = LJ; jb < ND; ++jb)
#pragma unroll
                for (int i = 0; i + jb < ND; ++i)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[i + jb][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(pa[i], pb[jb - LJ][nt], acc[i + jb][nt], 0, 0, 0);
        };
        for (int kt = 0; kt < NK; ++kt) {
            const int s = j * NK + kt;
            // stage s's pieces landed: vmcnt counts in issue order, so what may stay outstanding is the m later
            // stages already issued and, for a tile's first PD stages, the previous tile's 32 M stores (issued
            // after them). For NB = 3 and kt = 1 this is one wait less strict than round 5's vmcnt(GL)
            const int m = NS - 1 - s < PD - 1 ? NS - 1 - s : PD - 1;
            if (j > 0 && kt < PD) {
                if (m == 0) vm_lgkm_wait<32>();
                else if (m == 1) vm_lgkm_wait<GL + 32>();
                else if (m == 2) vm_lgkm_wait<2 * GL + 32>();
                else vm_lgkm_wait<3 * GL + 32>();
            } else {
                if (m == 0) vm_lgkm_wait<0>();
                else if (m == 1) vm_lgkm_wait<GL>();
                else if (m == 2) vm_lgkm_wait<2 * GL>();
                else vm_lgkm_wait<3 * GL>();
            }
            // the lagging operands are in registers now (lgkmcnt(0) above); KV_LAG_OPAQUE tells the compiler
            // so by an opaque redefinition (measured: no gain, see its definition)
#if KV_LAG_OPAQUE
#pragma unroll
            for (int i = 0; i < NA; ++i) asm volatile("" : "+v"(pa[i]));
#pragma unroll
            for (int jb = 0; jb < ND - LJ; ++jb)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(pb[jb][nt]));
#endif
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const char* buf = L0 + (s % NBUF) * T::STAGE;
            i8x16_t a[ND], b[ND][NT];
#pragma unroll
            for (int i = 0; i < ND; ++i) a[i] = *(const i8x16_t*)(buf + aoffr[i]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[0][nt] = *(const i8x16_t*)(buf + boffr[nt][0]);
            // the stage's reads issue before the lagging MFMAs (hipcc otherwise hoists those MFMAs above the reads,
            // so the reads start ~14 MFMA issues after the barrier): forward -2.3 % at 2,048 boards, -3.4 % at 256,
            // bit-identical; with the same barrier after each B digit's reads below, -5 % / -6 %
            // (profiles/r05_reads_first_ab.log; the 13-pair fp64-domain GEMM and the one-tile lag kernel came out
            // 1-2 % slower with it, so only here)
            __builtin_amdgcn_sched_barrier(0);
            if (kt > 0) h2();
            if (s + PD < NS) {
                issue1(0, s + PD);
                issue1(1, s + PD);
            }
#pragma unroll
            for (int jb = 0; jb < ND; ++jb) {
                if (jb + 1 < ND) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b[jb + 1][nt] = *(const i8x16_t*)(buf + boffr[nt][jb + 1]);
                }
                __builtin_amdgcn_sched_barrier(0);  // likewise each next B digit's reads before this one's MFMAs
                if (jb < LJ) {
#pragma unroll
                    for (int i = 0; i + jb < ND; ++i)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[i + jb][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[jb][nt], acc[i + jb][nt], 0, 0, 0);
                }
                if (jb == 0 && s + PD < NS) {
                    issue1(2, s + PD);
                    issue1(3, s + PD);
                }
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) pa[i] = a[i];
#pragma unroll
            for (int jb = LJ; jb < ND; ++jb)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) pb[jb - LJ][nt] = b[jb][nt];
        }
        h2();
        const int xi = xis[j], n_base = nbs[j], r_base = rbs[j];
        const int* evx = ev + (size_t)xi * stride + r_base + wm * 32;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = n_base + wn * NT * 32 + nt * 32 + lr;
            const int ec = eu[(size_t)xi * cout + col] - 14;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                double m = (double)acc[ND - 1][nt][r];
#pragma unroll
                for (int l = ND - 2; l >= 0; --l) m = __builtin_fma(m, kStep, (double)acc[l][nt][r]);  // exact
                M[((size_t)xi * stride + r_base + wm * 32 + row) * cout + col] = (float)ldexp(m, evx[row] + ec);
            }
        }
    }
    if constexpr (STAMP) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x < 4) {  // one vector store per value, lanes 0-3
            const unsigned long long v = threadIdx.x == 0 ? t0 : threadIdx.x == 1 ? t1 : threadIdx.x == 2 ? r0 : r1;
            stamps[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
        }
    }
}

__device__ __forceinline__ i32x16_t r3mfma(i8x16_t a, i8x16_t b, i32x16_t c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
}
// R3's GEMM (KV_PATH_WINO88_I8F32R3) with 64-k stages: the 32-k lagt kernel gives a wave 12 MFMAs per stage
// barrier at 3 digits (20 at 4), and its time did not move with 3, 4 or 5 ring buffers (370.6 / 371.3 / 371.6
// us, profiles/r06_ring_depth_ab.log): the barrier's fixed cost, not the copies' latency, sets it. Here a stage is
// two 32-channel chunks (24 MFMAs per wave per barrier) of R3's 96-byte row lines [xi][K/32][row][3][32] (3
// digits, no zero slot), so a stage is 48 KiB and the ring keeps 3 buffers (144 KiB) with two stages in flight.
// LDS image per operand and chunk: 128 rows of 96 bytes (a contiguous 12 KiB block of the global lines), 16-byte
// piece c = 2 d + half at position c ^ ((row >> 4) & 1) -- every ds_read_b128 lane group conflict-free
// (rows 16-31 of a 32-row block land on the odd 16-byte bank groups, rows 0-15 on the even ones). Copies: wave
// w fills 6 KiB pieces of plane (operand w >> 2, chunk (w >> 1) & 1), pieces 6 (w & 1) .. + 5; lane l of piece
// pp carries unit u = 64 pp + l = (row u / 6, slot u % 6). Per stage a wave runs chunk 0's 12 MFMAs, chunk 1's
// B digit 0 (6), and chunk 1's B digits 1-2 (6) after the next barrier under that stage's first reads. Same
// products, same exact int32 levels, same bits as the 32-k lagt form it replaced (measured bit-identical,
// profiles/r06_r3k64_ab.log; that form read 128-byte lines with a zero 4th slot and was retired with them).
// A tile's last stage (more than one tile per workgroup) has nothing to lag: it runs column half 0's MFMAs first,
// chunk 1's B digits 1-2 included, and half 0's epilogue (the exact three-level combine, one rounding, 16 stores)
// between half 1's last 9 MFMAs, placed by sched_group_barrier; half 1's epilogue follows the stage. The
// epilogue's stores address a wave-uniform 64-bit tile base plus a 32-bit lane offset. Exposed epilogue (the kernel
// against ABL 16): 66 of 346 us at 2,048 rows before this, profiles/r3_gemm_epilogue_ab.log.
// ABL 16 (a timing ablation, outputs invalid; never the product's, kv_dev_r3gemm_clock only): no epilogue at all,
// the accumulators consumed by an opaque use, and the waits allow no M stores in flight.
// KV_R3_M_NT (1): M stored non-temporally -- the GEMM 339 -> 325 us, the
// output kernels that read it +2 %, forward -1.5 % at 2,048 boards, neutral at 256 (profiles/r06_mnt_ab.log).
#ifndef KV_R3_M_NT
#define KV_R3_M_NT 1
#endif
template <int K, int TPW, bool STAMP = false, int ABL = 0>
__global__ __launch_bounds__(512) void wino88i32_gemm_r3k64_kernel(const int8_t* __restrict__ V8,
                                                                   const int* __restrict__ ev,
                                                                   const int8_t* __restrict__ U8,
                                                                   const int* __restrict__ eu, float* __restrict__ M,
                                                                   int rows, int cout, int stride,
                                                                   unsigned long long* __restrict__ stamps) {
    unsigned long long t0 = 0, r0 = 0;
    if constexpr (STAMP) {
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    constexpr int ND = 3, NB = 3, PD = NB - 1, GL = 6;
    constexpr int NT = 2, WM = 128, WN = 128, WC = 2;
    constexpr int NK = K / 32, NU = NK / 2, NSG = TPW * NU;  // stages per group of TPW tiles
    constexpr int PLANE = 128 * 96, STAGE = 4 * PLANE;  // [operand][chunk] planes: 48 KiB
    static_assert(NK % 2 == 0 && NU > PD && 8 * GL * 1024 == STAGE, "64-k stages, 6 pieces per wave");
    constexpr double kStep = 0.00390625;  // level weight: radix 256
    // SPLIT: a tile's last stage finishes column half 0 first and runs that half's epilogue between half 1's last
    // MFMAs (below). Not with one tile per workgroup: that form gains nothing from it (its two workgroups per CU
    // run out of step already) and the compiler spills registers there
    constexpr bool SPLIT = TPW > 1;
    static_assert(ABL == 0 || ABL == 16, "the product, or the no-epilogue ablation");
    constexpr int MST = ABL == 16 ? 0 : 32;  // M stores a tile's epilogue leaves in flight (none: ablated)

    extern __shared__ __attribute__((aligned(16))) i8x16_t lds_i8k64[];
    char* const L0 = (char*)lds_i8k64;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WC, wn = wave % WC;
    const int CT = cout / WN, RT = rows / WM;
    // nwg a multiple of 8; a workgroup runs ng groups of TPW tiles (the host makes nv = nwg TPW ng exact): one group
    // per workgroup in rounds, or, when the groups fill whole rounds of the CUs, ng of them per workgroup in one
    // round, the copy ring running across the group boundaries too
    const int nwg = (int)gridDim.x, nv = kv::W88_XI * RT * CT, ng = nv / (nwg * TPW), NST = ng * NSG;
    auto coords = [&](int T, int& xi, int& nb, int& rb) {  // tile T of this workgroup (XCD-aware order)
        const int vb = (int)blockIdx.x + T * nwg;
        const int idx = (vb & 7) * (nv >> 3) + (vb >> 3);
        xi = idx / (CT * RT);
        nb = (idx % CT) * WN;
        rb = ((idx / CT) % RT) * WM;
    };
    int xis[TPW], nbs[TPW], rbs[TPW];

    const int wu = __builtin_amdgcn_readfirstlane(wave);  // wave-uniform: the plane this wave copies
    const int op = wu >> 2, chunk = (wu >> 1) & 1, pp0 = 6 * (wu & 1);
    const size_t sstep = (op ? (size_t)cout : (size_t)stride) * 96;  // one 32-channel chunk of 96-byte row lines
    auto tile_base = [&](int xi, int nb, int rb) {
        return (op ? U8 + (((size_t)xi * NK) * cout + (size_t)nb) * 96 : V8 + (((size_t)xi * NK) * stride + (size_t)rb) * 96) +
               (size_t)chunk * sstep;
    };
    const int8_t* gb[TPW + 1];  // the group's tiles, then the next group's first
    // this lane's source byte in a chunk's row-line block, per piece: unsigned 32-bit, so the copy takes the
    // scalar-base + 32-bit-offset address form (one address VGPR per lane instead of a 64-bit pair)
    unsigned goff[GL];
#pragma unroll
    for (int g = 0; g < GL; ++g) {
        const int u = (pp0 + g) * 64 + lane, row = u / 6, slot = u - 6 * (u / 6);
        goff[g] = (unsigned)(row * 96 + 16 * (slot ^ ((row >> 4) & 1)));
    }
    const int ldst = (op * 2 + chunk) * PLANE + pp0 * 1024;
    auto issue1 = [&](int g, int s, int sg) {  // piece g of the group's stage s (tile s / NU), ring stage sg
        const int j = s / NU, ku = s - j * NU;
        const int8_t* base = gb[0];
#pragma unroll
        for (int jj = 1; jj <= TPW; ++jj) base = j == jj ? gb[jj] : base;
        const int8_t* const sb = base + (size_t)(2 * ku) * sstep;  // wave-uniform
#if KV_COPY_SADDR
        const void* src = (const void*)(sb + goff[g]);
#else
        const void* src = (const void*)(sb + (size_t)(int)goff[g]);
#endif
        __builtin_amdgcn_global_load_lds(src,
                                         (__attribute__((address_space(3))) void*)(L0 + (sg % NB) * STAGE + ldst +
                                                                                   g * 1024),
                                         16, 0, 0);
    };

    const int lr = lane & 31, lh = lane >> 5;
    const unsigned mlo = (unsigned)(4 * lh * cout + lr) * 4u;  // this lane's byte in its wave's block of an M tile
    const int arow = wm * 32 + lr;
    int aoff[2][ND], boff[2][NT][ND];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            aoff[h][d] = h * PLANE + arow * 96 + 16 * ((2 * d + lh) ^ ((arow >> 4) & 1));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int brow = wn * NT * 32 + nt * 32 + lr;
                boff[h][nt][d] = (2 + h) * PLANE + brow * 96 + 16 * ((2 * d + lh) ^ ((brow >> 4) & 1));
            }
        }

    // each group's row / column exponents staged in LDS beside the ring (2 x TPW x 1 KiB, by group parity): loaded
    // into registers at the group's start and stored after its first two stages, so the epilogue reads LDS instead
    // of waiting on global loads at each tile's end (timing ablation without the loads: 339 -> 323 us,
    // profiles/r06_r3k64_ablations_final.log)
    constexpr int NEX = (TPW * 256 + 511) / 512;
    int* const exl = (int*)(L0 + NB * STAGE);  // [2][TPW][256]: ev rows 0-127, eu columns 128-255
    for (int gi = 0; gi < ng; ++gi) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        coords(gi * TPW + j, xis[j], nbs[j], rbs[j]);
        gb[j] = tile_base(xis[j], nbs[j], rbs[j]);
    }
    {
        int xn, nn, rn;
        coords(gi + 1 < ng ? (gi + 1) * TPW : gi * TPW, xn, nn, rn);
        gb[TPW] = tile_base(xn, nn, rn);
    }
    int exv[NEX];
#pragma unroll
    for (int q = 0; q < NEX; ++q) {
        const int t = tid + q * 512;
        exv[q] = 0;
        if (t < TPW * 256) {
            const int jj = t >> 8, k = t & 255;
            exv[q] = k < 128 ? ev[(size_t)xis[jj] * stride + rbs[jj] + k] : eu[(size_t)xis[jj] * cout + nbs[jj] + k - 128];
        }
    }
    int* const exg = exl + (gi & 1) * TPW * 256;
    if (gi == 0) {
#pragma unroll
        for (int p = 0; p < PD; ++p)
#pragma unroll
            for (int g = 0; g < GL; ++g) issue1(g, p, p);
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        i32x16_t acc[ND][NT];
#pragma unroll
        for (int l = 0; l < ND; ++l)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[l][nt] = i32x16_t{};
        i8x16_t pa[2] = {}, pb[2][NT] = {};  // chunk 1's A digits 0-1 and B digits 1-2, lagging
        auto h2 = [&]() {
#pragma unroll
            for (int jb = 1; jb < ND; ++jb)
#pragma unroll
                for (int i = 0; i + jb < ND; ++i)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[i + jb][nt] = r3mfma(pa[i], pb[jb - 1][nt], acc[i + jb][nt]);
        };
        // M addresses: one wave-uniform 64-bit base per tile plus this lane's unsigned 32-bit byte offset mlo inside
        // the wave's 32 x 64 block (< 128 cout 4 = 256 KiB); a row or column half of the block is a wave-uniform
        // step from the base -- no per-store 64-bit row * cout multiply
        float* const Mt = M + ((size_t)xis[j] * stride + rbs[j] + wu / WC * 32) * cout + nbs[j] + wu % WC * NT * 32;
        const int* const evx = exg + j * 256 + wm * 32;  // LDS (staged below)
        auto epi = [&](int nt) {  // column half nt of the tile: the three levels combined (exact), one rounding
            const int ec = exg[j * 256 + 128 + wn * NT * 32 + nt * 32 + lr] - 14;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rowu = (r & 3) + 8 * (r >> 2), row = rowu + 4 * lh;
                double mm = (double)acc[ND - 1][nt][r];
#pragma unroll
                for (int l = ND - 2; l >= 0; --l) mm = __builtin_fma(mm, kStep, (double)acc[l][nt][r]);  // exact
                const float o = (float)ldexp(mm, evx[row] + ec);
                float* const mp = (float*)((char*)(Mt + (size_t)rowu * cout + nt * 32) + mlo);
                if constexpr (KV_R3_M_NT)
                    __builtin_nontemporal_store(o, mp);
                else
                    *mp = o;
            }
        };
        for (int ku = 0; ku < NU; ++ku) {
            const int s = j * NU + ku, sg = gi * NSG + s;
            const bool last = SPLIT && ku == NU - 1;
            // stage sg's pieces landed (vmcnt counts in issue order): what may stay outstanding is the m later
            // stages already issued and, for a tile's first PD stages, the previous tile's 32 M stores
            const int m = NST - 1 - sg < PD - 1 ? NST - 1 - sg : PD - 1;
            if (MST && (gi > 0 || j > 0) && ku < PD) {
                if (m == 0) vm_lgkm_wait<MST>();
                else vm_lgkm_wait<GL + MST>();
            } else {
                if (m == 0) vm_lgkm_wait<0>();
                else vm_lgkm_wait<GL>();
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const char* buf = L0 + (sg % NB) * STAGE;
            i8x16_t a0[ND], b0[ND][NT], a1[ND], b1[ND][NT];
#pragma unroll
            for (int d = 0; d < ND; ++d) a0[d] = *(const i8x16_t*)(buf + aoff[0][d]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b0[0][nt] = *(const i8x16_t*)(buf + boff[0][nt][0]);
            __builtin_amdgcn_sched_barrier(0);
            if (ku > 0) h2();
            if (sg + PD < NST) {
                issue1(0, s + PD, sg + PD);
                issue1(1, s + PD, sg + PD);
                issue1(2, s + PD, sg + PD);
            }
            // chunk 0: all 6 pairs
#pragma unroll
            for (int jb = 0; jb < ND; ++jb) {
                if (jb + 1 < ND) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b0[jb + 1][nt] = *(const i8x16_t*)(buf + boff[0][nt][jb + 1]);
                } else {
#pragma unroll
                    for (int d = 0; d < ND; ++d) a1[d] = *(const i8x16_t*)(buf + aoff[1][d]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b1[0][nt] = *(const i8x16_t*)(buf + boff[1][nt][0]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i + jb < ND; ++i)
#pragma unroll
                    for (int nt = 0; nt < (last && jb > 0 ? 1 : NT); ++nt)  // last: nt 1's come below
                        acc[i + jb][nt] = r3mfma(a0[i], b0[jb][nt], acc[i + jb][nt]);
                if (jb == 0 && sg + PD < NST) {
                    issue1(3, s + PD, sg + PD);
                    issue1(4, s + PD, sg + PD);
                    issue1(5, s + PD, sg + PD);
                }
            }
            // chunk 1: B digit 0 now, digits 1-2 after the next barrier
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                b1[1][nt] = *(const i8x16_t*)(buf + boff[1][nt][1]);
                b1[2][nt] = *(const i8x16_t*)(buf + boff[1][nt][2]);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (last) {
                // the tile's last stage: column half 0 finishes first (chunk 1's B digit 0 and, nothing left to lag
                // behind a barrier, its digits 1-2), then its 16 values are combined, rounded and stored between
                // column half 1's 9 remaining MFMAs (chunk 0's B digits 1-2, chunk 1's three) -- the matrix pipe
                // runs under half of the epilogue's VALU work instead of idling through all of it. Same products
                // into the same exact int32 levels, so the same bits; every store still issues before the next
                // tile's first wait, so no wait count changes
#pragma unroll
                for (int i = 0; i < ND; ++i) acc[i][0] = r3mfma(a1[i], b1[0][0], acc[i][0]);
#pragma unroll
                for (int jb = 1; jb < ND; ++jb)
#pragma unroll
                    for (int i = 0; i + jb < ND; ++i) acc[i + jb][0] = r3mfma(a1[i], b1[jb][0], acc[i + jb][0]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int jb = 1; jb < ND; ++jb)
#pragma unroll
                    for (int i = 0; i + jb < ND; ++i) acc[i + jb][1] = r3mfma(a0[i], b0[jb][1], acc[i + jb][1]);
#pragma unroll
                for (int i = 0; i < ND; ++i) acc[i][1] = r3mfma(a1[i], b1[0][1], acc[i][1]);
#pragma unroll
                for (int jb = 1; jb < ND; ++jb)
#pragma unroll
                    for (int i = 0; i + jb < ND; ++i) acc[i + jb][1] = r3mfma(a1[i], b1[jb][1], acc[i + jb][1]);
                if constexpr (ABL != 16) {
                    epi(0);
#pragma unroll
                    for (int q = 0; q < 9; ++q) {  // per MFMA: 16 VALU issues (two values' worth), two of the 16 stores
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
                        __builtin_amdgcn_sched_group_barrier(0x040, 2, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            } else {
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[i][nt] = r3mfma(a1[i], b1[0][nt], acc[i][nt]);
                pa[0] = a1[0];
                pa[1] = a1[1];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    pb[0][nt] = b1[1][nt];
                    pb[1][nt] = b1[2][nt];
                }
            }
            if (j == 0 && ku == 1) {  // the group's exponents (read back after the next barrier)
#pragma unroll
                for (int q = 0; q < NEX; ++q)
                    if (tid + q * 512 < TPW * 256) exg[tid + q * 512] = exv[q];
            }
        }
        if constexpr (!SPLIT) h2();
        if constexpr (ABL == 16) {  // ablation: no epilogue, the accumulators consumed by an opaque use
#pragma unroll
            for (int l = 0; l < ND; ++l)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) asm volatile("" ::"v"(acc[l][nt]));
        } else {
            if constexpr (!SPLIT) epi(0);
            epi(1);
        }
    }
    }  // groups
    if constexpr (STAMP) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x < 4) {  // one vector store per value, lanes 0-3
            const unsigned long long v = threadIdx.x == 0 ? t0 : threadIdx.x == 1 ? t1 : threadIdx.x == 2 ? r0 : r1;
            stamps[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
        }
    }
}

// KV_PREC_I8X5's GEMM (5 digits, digit planes, fp64 M) with wino88i32_gemm_lag_kernel's schedule: the
// B digits j >= LJ of a stage (their pairs i + j <= 4) run after the next barrier, under that stage's first
// LDS reads; stage k + 2's copies (5 pieces per wave) go into stage k - 1's buffer right after barrier k.
// V8: planes [xi][K/32][5][stride][32], U8: [xi][K/32][5][cout][32]; M fp64 [xi][stride rows][cout]. Exact int32
// levels, one exact fp64 combine: the bits of tests/_i8_digits' restatement, whatever the schedule.
// S = 4, RB = 8 (KV_PATH_WINO88_I8R): 4 radix-256 digit planes per operand (4 pieces per wave and stage), the
// 13 pairs i + j <= 4 of 16 -- the same 5 levels, weighted 2^-8l -- combined in fp64 (the last two fma steps
// may round: |level| <= 4 K 2^14 = 2^25, so the value has up to 57 significant bits; one fp64 rounding each).
// RL (S = 4): the operands in row lines [xi][K/32][row][4][32] (the fp32 tower's layout and LDS image: a
// stage of a tile is one contiguous 16 KiB block per operand), so the fused output kernel of one board writes
// whole 128-byte lines.
template <int K, int LJ = 3, int S = 5, int RB = 7, bool RL = false>
__global__ __launch_bounds__(512) void wino88i_gemm_lag5_kernel(const int8_t* __restrict__ V8,
                                                                const int* __restrict__ ev,
                                                                const int8_t* __restrict__ U8,
                                                                const int* __restrict__ eu, double* __restrict__ M,
                                                                int rows, int cout, int stride) {
    constexpr int LEV = 5, NBUF = 3;  // levels: pairs i + j < LEV
    using T = Wino88iTile<S>;
    constexpr int NT = T::NT, WM = T::WM, WN = T::WN, GL = T::GL;
    constexpr int NK = K / 32;
    constexpr int NA = S < LEV - LJ ? S : LEV - LJ;  // A digits the lagging half uses
    static_assert(GL == S && NK >= 3 && LJ >= 1 && LJ < S && (S == 5 || (S == 4 && RB == 8)) && (!RL || S == 4),
                  "S pieces per wave and stage; row lines hold 4 digits");

    extern __shared__ __attribute__((aligned(16))) i8x16_t lds_i8l5[];
    char* const L0 = (char*)lds_i8l5;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WC, wn = wave % T::WC;
    const int CT = cout / WN, RT = rows / WM;
    const int nwg = (int)gridDim.x;  // a multiple of 8
    const int idx = (int)(blockIdx.x & 7) * (nwg >> 3) + (int)(blockIdx.x >> 3);
    const int xi = idx / (CT * RT);
    const int n_base = (idx % CT) * WN;
    const int r_base = ((idx / CT) % RT) * WM;

    // copy pieces of the planes path: piece q = wave * S + g covers operand q / 4S, digit
    // (q % 4S) / 4, rows 32 (q % 4) .. +31; lane l fills LDS row 32 (q % 4) + l / 2, half l & 1 (swapped on
    // bit 3 of the row)
    const int op = (__builtin_amdgcn_readfirstlane(wave) * GL) / (4 * S);  // wave-uniform
    const size_t rstride = op ? (size_t)cout : (size_t)stride;
    // (a tile's rows start at row * 32 in a plane, row * 128 in row lines; a stage is S * 32 B per row in both)
    const int8_t* gbase = op ? U8 + ((size_t)xi * NK) * S * cout * 32 + (size_t)n_base * (RL ? 128 : 32)
                             : V8 + ((size_t)xi * NK) * S * stride * 32 + (size_t)r_base * (RL ? 128 : 32);
    const size_t sstep = (size_t)S * rstride * 32;
    const int lane_off = (lane >> 1) * 32 + 16 * ((lane & 1) ^ ((lane >> 4) & 1));
    // RL: piece q = wave * 4 + g is 8 row lines (1 KiB) of operand q / 16, rows 8 (q % 16) .. +7, copied as
    // wino88i32_gemm_lag_kernel's (the 16-byte chunks swizzled by i8_rl_off on the global side)
    const int rl_off0 = (lane >> 3) * 128 + 16 * ((lane & 7) ^ (lane >> 4));
    const int rl_off1 = (lane >> 3) * 128 + 16 * ((lane & 7) ^ (lane >> 4) ^ 4);
    auto issue1 = [&](int g, int kt) {
        const int q = wave * GL + g;
        if constexpr (RL) {
            const int rg8 = __builtin_amdgcn_readfirstlane(q) % 16;  // wave-uniform: the scalar-base form
            const int8_t* const sb = gbase + kt * sstep + (size_t)rg8 * 1024;
#if KV_COPY_SADDR
            const void* src = (const void*)(sb + (unsigned)((rg8 & 1) ? rl_off1 : rl_off0));
#else
            const void* src = (const void*)(sb + (size_t)((rg8 & 1) ? rl_off1 : rl_off0));
#endif
            __builtin_amdgcn_global_load_lds(
                src, (__attribute__((address_space(3))) void*)(L0 + (kt % NBUF) * T::STAGE + op * S * T::PLANE + rg8 * 1024),
                16, 0, 0);
        } else {
            const int d = (q % (4 * S)) / 4, rg = q % 4;
            __builtin_amdgcn_global_load_lds(
                (const void*)(gbase + kt * sstep + ((size_t)d * rstride + rg * 32) * 32 + lane_off),
                (__attribute__((address_space(3))) void*)(L0 + (kt % NBUF) * T::STAGE + op * S * T::PLANE +
                                                          d * T::PLANE + rg * 1024),
                16, 0, 0);
        }
    };

    const int lr = lane & 31, lh = lane >> 5;
    const int arow = wm * 32 + lr;
    // LDS offsets of digit d's fragments: planes (d * PLANE + a fixed offset) or row lines (i8_rl_off per digit)
    int aoffd[S], boffd[NT][S];
#pragma unroll
    for (int d = 0; d < S; ++d) {
        aoffd[d] = RL ? i8_rl_off(arow, 2 * d + lh) : d * T::PLANE + arow * 32 + i8_lds_half(arow, lh);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int bcol = wn * NT * 32 + nt * 32 + lr;
            boffd[nt][d] = S * T::PLANE + (RL ? i8_rl_off(bcol, 2 * d + lh) : d * T::PLANE + bcol * 32 +
                                                                               i8_lds_half(bcol, lh));
        }
    }

    i32x16_t acc[LEV][NT];
#pragma unroll
    for (int l = 0; l < LEV; ++l)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[l][nt] = i32x16_t{};
    i8x16_t pa[NA] = {}, pb[S - LJ][NT] = {};
    auto h2 = [&]() {
#pragma unroll
        for (int j = LJ; j < S; ++j)
#pragma unroll
            for (int i = 0; i < S && i + j < LEV; ++i)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[i + j][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(pa[i], pb[j - LJ][nt], acc[i + j][nt], 0, 0, 0);
    };

#pragma unroll
    for (int g = 0; g < GL; ++g) issue1(g, 0);
#pragma unroll
    for (int g = 0; g < GL; ++g) issue1(g, 1);
    for (int kt = 0; kt < NK; ++kt) {
        if (kt + 1 < NK)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GL) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#if KV_LAG_OPAQUE  // the lagging operands are in registers (wino88i32_gemm_lagt_kernel)
#pragma unroll
        for (int i = 0; i < NA; ++i) asm volatile("" : "+v"(pa[i]));
#pragma unroll
        for (int jb = 0; jb < S - LJ; ++jb)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(pb[jb][nt]));
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char* buf = L0 + (kt % NBUF) * T::STAGE;
        i8x16_t a[S], b[NT];
#pragma unroll
        for (int i = 0; i < S; ++i) a[i] = *(const i8x16_t*)(buf + aoffd[i]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = *(const i8x16_t*)(buf + boffd[nt][0]);
        if (kt > 0) h2();  // the previous stage's lagging half, under the reads above
        if (kt + 2 < NK) {
            issue1(0, kt + 2);
            issue1(1, kt + 2);
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (j > 0) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b[nt] = *(const i8x16_t*)(buf + boffd[nt][j]);
            }
            if (j < LJ) {
#pragma unroll
                for (int i = 0; i < S && i + j < LEV; ++i)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[i + j][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[nt], acc[i + j][nt], 0, 0, 0);
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) pb[j - LJ][nt] = b[nt];
            }
            if (j == 0 && kt + 2 < NK) {
#pragma unroll
                for (int g = 2; g < GL; ++g) issue1(g, kt + 2);
            }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) pa[i] = a[i];
    }
    h2();

    // epilogue: D col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int* evx = ev + (size_t)xi * stride + r_base + wm * 32;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n_base + wn * NT * 32 + nt * 32 + lr;
        const int ec = eu[(size_t)xi * cout + col] - 14;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            constexpr double w = RB == 8 ? 0.00390625 : 0.0078125;  // 2^-RB (radix 128: every step exact)
            double m = (double)acc[LEV - 1][nt][r];
#pragma unroll
            for (int l = LEV - 2; l >= 0; --l) m = __builtin_fma(m, w, (double)acc[l][nt][r]);
            M[((size_t)xi * stride + r_base + wm * 32 + row) * cout + col] = ldexp(m, evx[row] + ec);
        }
    }
}

// The next conv's digits come from two kernels, each at the occupancy of the
// fp64 out kernel (one workgroup = 128 channels of one board): the exponent of
// a V row needs the largest magnitude over all 512 channels, i.e. over 4
// workgroups. (One 1,024-thread workgroup per board computing both in one
// kernel was measured and dropped: 540-665 us per layer at 2,048 boards, its
// two passes serialised at one workgroup per CU, against 300-420 us for the
// fp64 out kernel; profiles/r04_i8_fused_out.log.)
//   wino88i_outmax_kernel: output transform + BN (+ residual) + ReLU -> fp32 Y
//     (as wino88d_out_half_kernel), the next V64 rows computed and reduced to
//     each point's max |V| over the workgroup's channels, folded into
//     evmax[xi][board] (high words of the doubles, atomicMax; zeroed before);
//   wino88i_in_kernel: the input transform of Y again (the same fma chains on
//     the same fp32 inputs: the same bits) and its 5 digits under the row
//     exponents -- what wino88i_slice_kernel makes of that V64.

template <bool RESID>
__global__ __launch_bounds__(256) void wino88i_outmax_kernel(const double* __restrict__ M, int rows,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* resid,
                                                             float* Y, unsigned* __restrict__ evmax) {
    __shared__ __attribute__((aligned(16))) unsigned red[4][2][5][16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
    const int c = blockIdx.x * 128 + w * 32 + (lane & 31), b = blockIdx.y;
    double t2[10][4];
    {
        float x2[4][8];
        wino88d_out_plane<RESID, true>(M, rows, b, c, h, (double)scale[c], (double)shift[c], resid, Y, x2);
        wino88d_input_cols(x2, h, t2);
    }
#pragma unroll
    for (int aa = 0; aa < 5; ++aa) {
        double o[10];
        wino88d_input_row(t2, h, aa, o);
        unsigned m[10];
#pragma unroll
        for (int bb = 0; bb < 10; ++bb)
            m[bb] = i8_half_max_dpp((unsigned)(__double_as_longlong(o[bb]) >> 32) & 0x7fffffffu);
        if ((lane & 31) == 16) {  // this half's 10 maxima (high words), written by one lane
            uint4* rr = (uint4*)&red[w][h][aa][0];
            rr[0] = make_uint4(m[0], m[1], m[2], m[3]);
            rr[1] = make_uint4(m[4], m[5], m[6], m[7]);
            *(uint2*)&red[w][h][aa][8] = make_uint2(m[8], m[9]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 100) {
        const int xi = threadIdx.x, a = xi / 10, bb = xi % 10, hh = a / 5, aa = a % 5;
        unsigned m = 0;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) m = red[ww][hh][aa][bb] > m ? red[ww][hh][aa][bb] : m;
        if (m) atomicMax(evmax + (size_t)xi * rows + b, m);
    }
}

// grid (512 / 32, boards / 4) x 256: wave w = board 4 blockIdx.y + w, lanes = the 32 channels of chunk
// kc = blockIdx.x (plane split over lanes l, l ^ 32), so the 4 waves write 4 consecutive rows -- one
// whole 128-byte line -- of each digit plane (xi, kc, d): 32-byte pieces from different workgroups made
// the plane writes 2.8x slower (421 us per layer at 2,048 boards, profiles/r04_i8_fused_out.log).
// X the fp32 activation [board][64][512]; writes the row exponents ex[xi][board] (from evmax) too.
// R8 (KV_PATH_WINO88_I8R): 4 radix-256 digit planes (i8_digits_r8) instead of 5 radix-128 ones.
template <bool R8 = false>
__global__ __launch_bounds__(256) void wino88i_in_kernel(const float* __restrict__ X, int rows,
                                                         const unsigned* __restrict__ evmax,
                                                         int8_t* __restrict__ V8n, int* __restrict__ ex) {
    constexpr int C = 512, D = R8 ? 4 : kI8Digits;
    __shared__ int exs[4][100];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
    const int kc = blockIdx.x, c = kc * 32 + (lane & 31), b = blockIdx.y * 4 + w;
    for (int i = threadIdx.x; i < 400; i += 256) {
        const int bw = i / 100, xi = i % 100, bb = blockIdx.y * 4 + bw;
        const unsigned m = evmax[(size_t)xi * rows + bb];
        const int e = R8 ? i8_row_exponent_r8(m) : i8_row_exponent(m);
        exs[bw][xi] = e;
        if (kc == 0) ex[(size_t)xi * rows + bb] = e;
    }
    float x2[4][8];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int j = 0; j < 8; ++j) x2[ii][j] = X[((size_t)b * 64 + (4 * h + ii) * 8 + j) * C + c];
    double t2[10][4];
    wino88d_input_cols(x2, h, t2);
    __syncthreads();
    // 32-bit byte offsets (the digit planes of 100 x rows x 512 values, 5 digits: < 2^32 bytes): one base
    // register + a 32-bit offset per store
    const unsigned off0 = ((unsigned)kc * D * rows + b) * 32 + (lane & 31);
    const unsigned dstride = (unsigned)rows * 32, xstride = (C / 32) * D * dstride;
    // (one byte store per digit: a lane-quad transpose into dword stores measured 3 % slower here,
    // profiles/r05_i8x5_ab.log -- the kernel is bound by its fp64 transform and digit arithmetic; the digits
    // by magic-number adds: profiles/r05_i8x5_magic_ab.log; non-temporal byte stores -- 32-byte pieces of
    // lines -- made the forward 28 % slower: profiles/r05_i8x5_nt_ab.log)
#pragma unroll
    for (int aa = 0; aa < 5; ++aa) {
        double o[10];
        wino88d_input_row(t2, h, aa, o);
        const int a = 5 * h + aa;
#pragma unroll
        for (int bb = 0; bb < 10; ++bb) {
            const int xi = a * 10 + bb;
            unsigned dg[D];
            if constexpr (R8) {
                const unsigned P = i8_digits_r8(o[bb], exs[w][xi]);
#pragma unroll
                for (int d = 0; d < D; ++d) dg[d] = P >> (8 * (D - 1 - d));
            } else {
                i8_digits_magic<D>(o[bb], exs[w][xi], dg);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) V8n[off0 + (unsigned)xi * xstride + (unsigned)d * dstride] = (int8_t)dg[d];
        }
    }
}

// ---- the fp32 Winograd domain with int8-digit GEMMs (KV_PATH_WINO88_I8F32) ----
// The fp32 F(8x8) tower's arithmetic (kv_wino88.h: fp32 transforms, V, M and activations; U as
// 4 digits of the fp64 U) with each GEMM taken from 4 int8 digits per value: per-row 28-bit block
// fixed point (each value cut to the multiples of 2^(e-29) of its row's exponent e), the 10 digit pairs
// i + j <= 3 of the 16, exact int32 levels, combined exactly and rounded to fp32 once -- where the fp32
// MFMA GEMM rounds after every product. An fp32 value within 2^-4 of its row's max keeps all its bits; one
// 2^-k below keeps 28 - k (the bound test: tests/test_wino_i8_gpu.py). 10 int8 MFMAs per point product against one fp32 one at
// 1/32 the rate.

// wino88i32_out_kernel: the fp32 tower's output transform + BN (+ residual) + ReLU -> Y (optional), then
// the next conv's V as row-line digits under each row's exponent -- what wino88_out_kernel's fp32 V
// followed by wino88i_slice_kernel<512, float, 4, true> gives, bit for bit, without V's HBM round trip.
// One 512-thread workgroup per board, thread = channel, so the 512 channels of a row (the exponent's
// domain) are in one workgroup. Each (board, channel) plane is split over lanes l and l ^ 32 (the
// transforms' half exchanges are v_permlane32_swap), so a lane keeps its 50 V values in registers across
// the exponent barrier: the row maxima (DPP max per half-wave, then LDS over the waves), the exponents, then
// the digits of the kept values -- the same fmaf chains on the same inputs as wino88_out_kernel + the slice
// kernel, so the same bits. A thread's 4 digits of a point go through a 4x4 byte transpose within its lane
// quad (two DPP exchanges + v_perm), so every lane stores one dword and each half-wave writes one whole
// 128-byte line.
// (Round 4 dropped a form that kept all 100 V values in registers for the reduction: 246 VGPRs, one
// workgroup per CU, 436-511 us per layer against 142-238 + 165 us for the out kernel + slice,
// profiles/r04_i8f32_fused_out.log; and an output kernel computing only the row maxima plus a second
// input-transform pass, 294-356 + 220 us, profiles/r04_i8f32_outmax_form.log.)

// Row-line width: 4 digit slots (128 bytes) per 32-channel chunk, or R3's 3 (96 bytes: no zero slot in memory)
template <bool R3>
constexpr unsigned kI8LineBytes = R3 ? 96u : 128u;
// The board an output workgroup handles. R3's 96-byte lines of boards 4g .. 4g+3 share 128-byte lines (4 x 96 =
// 3 x 128), so those 4 boards go to one XCD (workgroups are dealt to the 8 XCDs round-robin: id mod 8), whose L2
// merges their partial lines; dealt board by board, each shared line took partial writes from two XCDs. A
// bijection on [0, nb) for nb a multiple of 32.
template <bool R3>
__device__ inline int out_board(int id) {
    if constexpr (!R3) return id;
    const int x = id & 7, s = id >> 3;
    return 4 * (x + 8 * (s >> 2)) + (s & 3);
}

// R3 (KV_PATH_WINO88_I8F32R3): the next V's 3 radix-256 digits (i8_digits_r3 under i8_row_exponent_f32r) in
// the same lines, slot 3 zero
template <bool R3>
__device__ inline int i8f32_row_exponent(unsigned m) {
    return R3 ? i8_row_exponent_f32r(m) : i8_row_exponent_f32(m);
}
template <bool R3>
__device__ inline unsigned i8f32_digits(float v, int e) {
    if constexpr (R3)
        return i8_digits_r3((double)v, e);
    else
        return i8_digits4_packed(v, e);
}

// STAMP (a diagnostic build, never the product's; kv_dev_out_phases): waves 0 and 15 record the shader clock at the
// kernel's phase boundaries into kOutStamps[board][wave 0/15][8] -- a buffer no other code reads: start, V ready
// (M loaded, both transforms done), after the maxima barrier, after the exponent barrier, digit stores issued,
// stores drained.
constexpr int kOutStampBoards = 4096;
__device__ unsigned long long kOutStamps[kOutStampBoards][2][8];

// CW channels per workgroup (2 CW threads: a plane split over lanes l, l ^ 32): 512 only -- the row's exponent
// over all its channels, one workgroup per board, grid (1, boards), so blockIdx.x is 0. (The CW 256 form, an
// exponent per 256-channel segment from two workgroups per board, was built, measured and removed; the callers'
// exponent buffers hold one exponent per row and would not take it.)
template <bool RESID, bool WRITE_Y, int CW, bool R3 = false, bool STAMP = false, bool YNT = false>
__global__ __launch_bounds__(2 * CW) void wino88i32_out_kernel(const float* __restrict__ M, int rows,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift, const float* resid,
                                                               float* Y, int8_t* __restrict__ V8,
                                                               int* __restrict__ ex) {
#pragma clang fp contract(off)
    static_assert(CW == 512, "a row per workgroup (the exponent buffers hold one exponent per row)");
    constexpr int NK = 512 / 32, NW = CW / 32, NSEG = 512 / CW;
    __shared__ __attribute__((aligned(16))) unsigned red[NW][2][5][16];
    __shared__ int exs[100];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
    const int seg = blockIdx.x, c = seg * CW + w * 32 + (lane & 31), b = out_board<R3>((int)blockIdx.y);
    unsigned long long st[6] = {};
    const bool stamper = STAMP && (w == 0 || w == NW - 1) && lane == 0 && b < kOutStampBoards;
    if constexpr (STAMP) st[0] = __builtin_amdgcn_s_memtime();
    float vk[5][10];  // this half's 50 V values (rows 5h .. 5h+4), kept across the exponent barrier
    {
        float t2[10][4];  // B10^T of the plane's columns 4h .. 4h+3
        {
            float x2[4][8];
            wino88_out_plane_half<RESID, WRITE_Y, YNT>(M, rows, b, c, h, scale[c], shift[c], resid, Y, x2);
            wino88_input_cols(x2, h, t2);
        }
#pragma unroll
        for (int aa = 0; aa < 5; ++aa) wino88_input_row(t2, h, aa, vk[aa]);
    }
    if constexpr (STAMP) {  // V ready: the transforms' results are consumed by an opaque use first
#pragma unroll
        for (int aa = 0; aa < 5; ++aa)
#pragma unroll
            for (int bb = 0; bb < 10; ++bb) asm volatile("" ::"v"(vk[aa][bb]));
        st[1] = __builtin_amdgcn_s_memtime();
    }
#pragma unroll
    for (int aa = 0; aa < 5; ++aa) {
        const float (&o)[10] = vk[aa];
        unsigned m[10];
#pragma unroll
        for (int bb = 0; bb < 10; ++bb) m[bb] = i8_half_max_dpp(__float_as_uint(o[bb]) & 0x7fffffffu);
        if ((lane & 31) == 16) {  // this half's 10 maxima, written by one lane
            uint4* rr = (uint4*)&red[w][h][aa][0];
            rr[0] = make_uint4(m[0], m[1], m[2], m[3]);
            rr[1] = make_uint4(m[4], m[5], m[6], m[7]);
            *(uint2*)&red[w][h][aa][8] = make_uint2(m[8], m[9]);
        }
    }
    __syncthreads();
    if constexpr (STAMP) st[2] = __builtin_amdgcn_s_memtime();
    if (threadIdx.x < 100) {
        const int xi = threadIdx.x, a = xi / 10, bb = xi % 10, hh = a / 5, aa = a % 5;
        unsigned m = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) m = red[ww][hh][aa][bb] > m ? red[ww][hh][aa][bb] : m;
        const int e = i8f32_row_exponent<R3>(m);
        exs[xi] = e;
        ex[((size_t)xi * NSEG + seg) * rows + b] = e;
    }
    __syncthreads();
    if constexpr (STAMP) st[3] = __builtin_amdgcn_s_memtime();
    // row line (xi, kc = c / 32, b): 128 bytes, digit d of channel 32 kc + i at byte 32 d + i
    const int q = lane & 3;
    // 32-bit byte offsets (the digits of 100 x rows x 512 values < 2^32 bytes)
    const unsigned off0 = ((unsigned)(c >> 5) * rows + b) * kI8LineBytes<R3> + q * 32 + (c & 28),
                   xstride = NK * rows * kI8LineBytes<R3>;
    unsigned* const dst = (unsigned*)V8;
#pragma unroll
    for (int aa = 0; aa < 5; ++aa) {
        const int a = 5 * h + aa;
#pragma unroll
        for (int bb = 0; bb < 10; ++bb) {
            const int xi = a * 10 + bb;
            const unsigned P = i8f32_digits<R3>(vk[aa][bb], exs[xi]);
            // non-temporal: the digits are read once, by the next GEMM (forward -1.2 % at 2,048 boards against
            // plain stores, bit-identical; the GEMM's M stored non-temporal instead slowed the output kernel that
            // reads it: profiles/r05_out_nt_ab.log)
            {
                const unsigned T4 = i8_quad_transpose(P, lane);  // lane q of the quad: digit q's 4 channels
                if constexpr (!R3)
                    __builtin_nontemporal_store(T4, &dst[(off0 + (unsigned)xi * xstride) >> 2]);
                else if (q < 3)  // R3's 96-byte lines share 128-byte lines: ordinary stores, merged in L2
                    dst[(off0 + (unsigned)xi * xstride) >> 2] = T4;
            }
        }
    }
    if constexpr (STAMP) {
        st[4] = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        st[5] = __builtin_amdgcn_s_memtime();
        if (stamper) {
            unsigned long long* o = kOutStamps[b][w == 0 ? 0 : 1];
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = st[k];
        }
    }
}

// stem_r3_kernel: the front of the R3 tower in one kernel -- conv1 + BN + ReLU straight from the int8 board codes
// (stem_kernel<4>'s arithmetic: the occupied 3x3 neighbours' weights added in tap order, one fmaf for the folded
// BN, as the compiler contracts it there), conv2's input transform by lane swaps (wino88_input_cols / _row, as
// wino88_input_half), then wino88i32_out_kernel's back half at 256 channels: row maxima (DPP, then LDS over the 8
// waves), i8_row_exponent_f32r, i8_digits_r3, the quad byte transpose, 96-byte row lines [100][8][rows][3][32] and
// exponents [100][rows] -- what stem_kernel<4>'s fp32 V256 followed by wino88i_slice_kernel<256, float, 4, true, 1,
// false, true> gives, bit for bit, without V256's HBM round trip (105 KB written and read per board).
// 512 threads = a board's 256 channels, a plane split over lanes l and l ^ 32. conv1 ([code 0..12][tap][256], code
// 0 = empty = zero rows: 117 KiB) is staged in LDS once per workgroup, and the workgroup loops over boards
// out_board(blockIdx.x + k gridDim.x): with gridDim.x a multiple of 8, every id it runs has its own id mod 8, so
// the 4 boards that share 128-byte lines stay on one XCD (out_board). Boards >= nb are empty (padding rows).
constexpr int kStemR3Lds = 9 * 13 * 256 * 4;
__global__ __launch_bounds__(512) void stem_r3_kernel(const int8_t* __restrict__ boards, int nb, int rows,
                                                      const float* __restrict__ wT, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, int8_t* __restrict__ V8,
                                                      int* __restrict__ ex) {
#pragma clang fp contract(off)
    constexpr int NK = 256 / 32, NW = 8;
    extern __shared__ __attribute__((aligned(16))) float stem_wl[];  // [13][9][256]
    // the board with a one-square empty border (10x10), each code as its table offset: a square's address (+ the
    // lane's channel) is computed once for the up to 9 taps that read it, the tap an immediate offset
    __shared__ int codes[100];
    __shared__ __attribute__((aligned(16))) unsigned red[NW][2][5][16];
    __shared__ int exs[100];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
    const int c = w * 32 + (lane & 31);
    for (int i = threadIdx.x; i < 9 * 13 * 256; i += 512) {
        const int r = i >> 8, code = r / 9, t = r % 9;
        stem_wl[i] = code ? wT[(size_t)(t * 12 + code - 1) * 256 + (i & 255)] : 0.f;
    }
    const float sc = scale[c], sh = shift[c];
    const int q = lane & 3;
    unsigned* const dst = (unsigned*)V8;
    const unsigned xstride = NK * (unsigned)rows * 96u;
    for (int id = blockIdx.x; id < rows; id += gridDim.x) {
        const int b = out_board<true>(id);
        __syncthreads();  // the table staged; the previous board's codes and exponents read
        if (threadIdx.x < 100) {
            const int i = threadIdx.x, r = i / 10 - 1, f = i % 10 - 1;
            const bool in = b < nb && r >= 0 && r < 8 && f >= 0 && f < 8;
            codes[i] = in ? boards[(size_t)b * 64 + r * 8 + f] * (9 * 256) : 0;
        }
        __syncthreads();
        float vk[5][10];  // this half's 50 V values (rows 5h .. 5h+4), kept across the exponent barrier
        {
            float t2[10][4];
            {
                float x2[4][8];
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                    for (int px = 0; px < 8; ++px) {
                        const int py = 4 * h + ii;
                        float acc = 0.f;
#pragma unroll
                        for (int t = 0; t < 9; ++t)
                            acc += stem_wl[codes[(py + t / 3) * 10 + px + t % 3] + t * 256 + c];
                        const float v = __builtin_fmaf(acc, sc, sh);
                        x2[ii][px] = v > 0.f ? v : 0.f;
                    }
                wino88_input_cols(x2, h, t2);
            }
#pragma unroll
            for (int aa = 0; aa < 5; ++aa) wino88_input_row(t2, h, aa, vk[aa]);
        }
#pragma unroll
        for (int aa = 0; aa < 5; ++aa) {
            unsigned m[10];
#pragma unroll
            for (int bb = 0; bb < 10; ++bb) m[bb] = i8_half_max_dpp(__float_as_uint(vk[aa][bb]) & 0x7fffffffu);
            if ((lane & 31) == 16) {  // this half's 10 maxima, written by one lane
                uint4* rr = (uint4*)&red[w][h][aa][0];
                rr[0] = make_uint4(m[0], m[1], m[2], m[3]);
                rr[1] = make_uint4(m[4], m[5], m[6], m[7]);
                *(uint2*)&red[w][h][aa][8] = make_uint2(m[8], m[9]);
            }
        }
        __syncthreads();
        if (threadIdx.x < 100) {
            const int xi = threadIdx.x, a = xi / 10, bb = xi % 10, hh = a / 5, aa = a % 5;
            unsigned m = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) m = red[ww][hh][aa][bb] > m ? red[ww][hh][aa][bb] : m;
            const int e = i8_row_exponent_f32r(m);
            exs[xi] = e;
            ex[(size_t)xi * rows + b] = e;
        }
        __syncthreads();
        // row line (xi, kc = c / 32, b): 96 bytes, digit d of channel 32 kc + i at byte 32 d + i
        const unsigned off0 = ((unsigned)(c >> 5) * rows + b) * 96u + q * 32 + (c & 28);
#pragma unroll
        for (int aa = 0; aa < 5; ++aa) {
            const int a = 5 * h + aa;
#pragma unroll
            for (int bb = 0; bb < 10; ++bb) {
                const int xi = a * 10 + bb;
                const unsigned P = i8_digits_r3((double)vk[aa][bb], exs[xi]);
                const unsigned T4 = i8_quad_transpose(P, lane);  // lane q of the quad: digit q's 4 channels
                if (q < 3) dst[(off0 + (unsigned)xi * xstride) >> 2] = T4;  // ordinary stores, merged in L2
            }
        }
    }
}

// ---- the fp32 tower with fp64 input transforms (KV_PATH_WINO88_I8F32V) ----
// The same tower as KV_PATH_WINO88_I8F32 (fp32 M, output transform and activations, the 4-digit GEMM)
// except that every conv's V is the fp64 input transform of its fp32 input, cut to 4 digits from fp64:
// on learn-loop weights the fp32 input transform is what sets the fp32 tower's value error
// (profiles/r05_learn_stage_emulate.log).

// Transform rows of the two halves at step aa: one +-p row pair of w88d_bt's even / odd form, (1, 2), (3, 4),
// (5, 6), (7, 8), or (0, 9) at aa = 0 -- half 0 takes the first, half 1 the second.
__device__ inline int w88v_row(int h, int aa) { return aa == 0 ? 9 * h : 2 * aa - 1 + h; }

// fp64 transform row w88v_row(h, aa) of a plane split over lanes l, l ^ 32, from the half's 4 columns after
// the half exchange (xc[kk][i] = pixel (i, 4h + kk)): the fma chains of wino88d_input_cols +
// wino88d_input_row on the same inputs -- so the same bits as wino88d_input_plane -- one transform row pair
// at a time (each column's w88d_bt is taken for that pair only, which shares its even / odd halves), so no
// 10x4 fp64 intermediate is live.
__device__ inline void wino88d_input_row_of_cols(float (&xc)[4][8], int aa, double (&o)[10]) {
    // opaque to the compiler per row: otherwise it keeps the 32 widened values (64 VGPRs) live across the
    // rows and both passes instead of widening them again, and spills
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(xc[kk][i]));
    double row[10];
    row[0] = 0.0;
    row[9] = 0.0;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        double col[10], t[10];
        col[0] = 0.0;
        col[9] = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) col[1 + i] = (double)xc[kk][i];
        w88d_bt(col, t);
        double lo = t[w88v_row(0, aa)], hi = t[w88v_row(1, aa)];
        half_swap(lo, hi);
        row[1 + kk] = lo;
        row[5 + kk] = hi;
    }
    w88d_bt(row, o);
}

// wino88i32v_out_kernel: wino88i32_out_kernel<RESID, WRITE_Y, 512> with the next conv's V taken as the fp64
// input transform of the fp32 activation (what wino88d_in_kernel + wino88i_slice_kernel<512, double, 4,
// true> give, bit for bit). 50 fp64 V values per lane do not fit beside the rest at 1,024 threads, so the
// lane keeps its 32 fp32 activations across the exponent barrier instead and transforms them twice: once
// for the row maxima (the high words of |V|), once for the digits (magic-number fp64 rint).
// wino88i64r_out_kernel (KV_PATH_WINO88_I8R): the same from an fp64 M with the fp64 output transform
// (wino88d_out_plane, as wino88d_out_half_kernel) and the 4 radix-256 digits (i8_digits_r8 under
// i8_row_exponent_r8) -- what wino88d_out_half_kernel's Y + wino88d_in_kernel + the radix-256 slice kernel
// give, bit for bit -- replacing the outmax + in kernel pair of the planes layout.
template <bool RESID, bool WRITE_Y, class MT>
__device__ inline void wino88v_out_body(const MT* __restrict__ M, int rows, const float* __restrict__ scale,
                                        const float* __restrict__ shift, const float* resid, float* Y,
                                        int8_t* __restrict__ V8, int* __restrict__ ex) {
    constexpr bool R8 = sizeof(MT) == 8;
    constexpr int NK = 512 / 32, NW = 16;
    __shared__ __attribute__((aligned(16))) unsigned red[NW][2][5][16];
    __shared__ int exs[100];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5;
    const int c = w * 32 + (lane & 31), b = blockIdx.y;
    float xc[4][8];  // the half's columns 4h .. 4h+3, all 8 rows (after the half exchange)
    {
        float x2[4][8];
        if constexpr (R8)
            wino88d_out_plane<RESID, WRITE_Y>(M, rows, b, c, h, (double)scale[c], (double)shift[c], resid, Y, x2);
        else
            wino88_out_plane_half<RESID, WRITE_Y>(M, rows, b, c, h, scale[c], shift[c], resid, Y, x2);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                float lo = x2[ii][kk], hi = x2[ii][4 + kk];
                half_swap(lo, hi);
                xc[kk][ii] = lo;
                xc[kk][4 + ii] = hi;
            }
    }
#pragma unroll
    for (int aa = 0; aa < 5; ++aa) {
        double o[10];
        wino88d_input_row_of_cols(xc, aa, o);
        unsigned m[10];
#pragma unroll
        for (int bb = 0; bb < 10; ++bb)
            m[bb] = i8_half_max_dpp((unsigned)(__double_as_longlong(o[bb]) >> 32) & 0x7fffffffu);
        if ((lane & 31) == 16) {
            uint4* rr = (uint4*)&red[w][h][aa][0];
            rr[0] = make_uint4(m[0], m[1], m[2], m[3]);
            rr[1] = make_uint4(m[4], m[5], m[6], m[7]);
            *(uint2*)&red[w][h][aa][8] = make_uint2(m[8], m[9]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 100) {  // point row a came from half hh at step aa (w88v_row)
        const int xi = threadIdx.x, a = xi / 10, bb = xi % 10;
        const int hh = a == 9 ? 1 : (a == 0 ? 0 : (a - 1) & 1), aa = (a == 0 || a == 9) ? 0 : (a + 1) >> 1;
        unsigned m = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) m = red[ww][hh][aa][bb] > m ? red[ww][hh][aa][bb] : m;
        const int e = R8 ? i8_row_exponent_r8(m) : i8_row_exponent(m);
        exs[xi] = e;
        ex[(size_t)xi * rows + b] = e;
    }
    __syncthreads();
    const int q = lane & 3;
    const unsigned off0 = ((unsigned)(c >> 5) * rows + b) * 128 + q * 32 + (c & 28), xstride = NK * rows * 128;
    unsigned* const dst = (unsigned*)V8;
#pragma unroll
    for (int aa = 0; aa < 5; ++aa) {
        double o[10];
        wino88d_input_row_of_cols(xc, aa, o);
        const int a = w88v_row(h, aa);
#pragma unroll
        for (int bb = 0; bb < 10; ++bb) {
            const int xi = a * 10 + bb;
            unsigned P;  // byte d = digit d (the most significant first)
            if constexpr (R8) {
                P = __builtin_bswap32(i8_digits_r8(o[bb], exs[xi]));
            } else {
                unsigned dq[4];
                i8_digits_magic<4>(o[bb], exs[xi], dq);
                P = __builtin_amdgcn_perm(dq[1], dq[0], 0x0c0c0400u) | __builtin_amdgcn_perm(dq[3], dq[2], 0x0c0c0400u) << 16;
            }
            __builtin_nontemporal_store(i8_quad_transpose(P, lane), &dst[(off0 + (unsigned)xi * xstride) >> 2]);
        }
    }
}

template <bool RESID, bool WRITE_Y>
__global__ __launch_bounds__(1024) void wino88i32v_out_kernel(const float* __restrict__ M, int rows,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* resid,
                                                              float* Y, int8_t* __restrict__ V8, int* __restrict__ ex) {
    wino88v_out_body<RESID, WRITE_Y>(M, rows, scale, shift, resid, Y, V8, ex);
}

template <bool RESID, bool WRITE_Y>
__global__ __launch_bounds__(1024) void wino88i64r_out_kernel(const double* __restrict__ M, int rows,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* resid,
                                                              float* Y, int8_t* __restrict__ V8, int* __restrict__ ex) {
    wino88v_out_body<RESID, WRITE_Y>(M, rows, scale, shift, resid, Y, V8, ex);
}

}  // namespace kv
