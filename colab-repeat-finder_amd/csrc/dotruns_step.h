// dotruns_step.h -- 64 cells of a diagonal or anti-diagonal of the dot plot of two ranges per step, straight on the planes in
// global memory: what the kernels of dotruns.hip and dotchain.hip walk a line with.  Device code, in an
// anonymous namespace: each translation unit that includes it gets its own copy, moved here unchanged from dotruns.hip.
// No address outside the words first .. last of the planes that hold a range is ever formed (dr_bits).
#pragma once
#include "../../include/prf.h"
#include "prf_host.h"

namespace {

// the complement of a letter outside ACGTN by its 5-bit code (A = 1 ... Z = 26; 0: N, which stays): R <-> Y, K <-> M, B <-> V,
// D <-> H; S, W and every other letter map to themselves
__device__ __forceinline__ u32 dot_comp_letter(u32 e) {
    switch (e) {
        case 18u: return 25u;   // R -> Y
        case 25u: return 18u;
        case 11u: return 13u;   // K -> M
        case 13u: return 11u;
        case 2u: return 22u;    // B -> V
        case 22u: return 2u;
        case 4u: return 8u;     // D -> H
        case 8u: return 4u;
        default: return e;
    }
}

// ---- the follow: 64 cells of a run per step, straight on the planes ----

// the words of the planes that hold the two ranges
struct dr_words {
    long long a_first, a_last, b_first, b_last;
};
__device__ __forceinline__ dr_words dr_words_of(const prf_dotruns_args &a) {     // na, nb > 0
    return {(long long)(a.a_g_begin >> 6), (long long)((a.a_g_begin + a.na - 1) >> 6), (long long)(a.b_g_begin >> 6),
            (long long)((a.b_g_begin + a.nb - 1) >> 6)};
}

// the 64 bits of plane P from global position q (which may lie in front of the planes: q < 0); words outside first .. last read as 0
__device__ __forceinline__ u64 dr_bits(const u64 *__restrict__ P, long long q, long long first, long long last) {
    const long long w = q >> 6;                      // floor
    const u64 lo = (w >= first && w <= last) ? P[w] : 0ull;
    const u64 hi = (w + 1 >= first && w + 1 <= last) ? P[w + 1] : 0ull;
    return prf_fsr(lo, hi, (unsigned)(q & 63));
}

// positions at which all five planes spell the letter `code`
__device__ __forceinline__ u64 dr_is_letter(const u64 *e, u32 code) {
    u64 m = ~0ull;
#pragma unroll
    for (int k = 0; k < 5; k++) m &= ((code >> k) & 1u) ? e[k] : ~e[k];
    return m;
}

// The mismatches among cells s .. s + 63 of the run of direction `dir` that starts at (i, j): bit t = cell (i + s + t, j + s + t)
// (main) or (i + s + t, j - s - t) (anti) is not raw, or lies outside the rectangle.  The comparison is that of the raw cells of
// the tile: ACGT by the two code bits (the minus strand flips the high one), N == N, any other letter by its five planes against
// the complement of the column's letter.
template <bool EXOTIC>
__device__ __forceinline__ u64 dr_step(const prf_dotruns_args &a, const dr_words &w, u64 i, u64 j, u32 dir, u64 s) {
    const bool anti = dir == PRF_DOTRUN_ANTI;
    const u64 left_a = a.na - i;                                  // cells to the rectangle's edge from the start, > 0
    const u64 left_b = anti ? j + 1 : a.nb - j;
    const u64 left = left_a < left_b ? left_a : left_b;
    if (s >= left) return ~0ull;
    const u64 lim = left - s;
    const u64 inside = lim >= 64 ? ~0ull : (1ull << lim) - 1ull;
    const long long qa = (long long)(a.a_g_begin + i + s);
    const long long qb = anti ? (long long)(a.b_g_begin + j - s) - 63ll : (long long)(a.b_g_begin + j + s);
    const u64 ah = dr_bits(a.pl.H, qa, w.a_first, w.a_last), al = dr_bits(a.pl.L, qa, w.a_first, w.a_last);
    const u64 ax = dr_bits(a.pl.X, qa, w.a_first, w.a_last);
    u64 bh = dr_bits(a.pl.H, qb, w.b_first, w.b_last), bl = dr_bits(a.pl.L, qb, w.b_first, w.b_last);
    u64 bx = dr_bits(a.pl.X, qb, w.b_first, w.b_last);
    if (anti) bh = __brevll(bh), bl = __brevll(bl), bx = __brevll(bx);        // bit t = B[j - s - t]
    if (a.strand) bh = ~bh;                                                    // A <-> T, C <-> G
    u64 match = ~ax & ~bx & ~((ah ^ bh) | (al ^ bl));
    u64 both_x = ax & bx;
    if (EXOTIC) {
        if (both_x) {
            u64 ae[5], be[5];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                ae[k] = dr_bits(a.pl.E[k], qa, w.a_first, w.a_last);
                be[k] = dr_bits(a.pl.E[k], qb, w.b_first, w.b_last);
                if (anti) be[k] = __brevll(be[k]);
            }
            if (a.strand) {                                                    // dot_comp_letter on 64 columns at once
                const u64 ry = dr_is_letter(be, 18u) | dr_is_letter(be, 25u), km = dr_is_letter(be, 11u) | dr_is_letter(be, 13u);
                const u64 bv = dr_is_letter(be, 2u) | dr_is_letter(be, 22u), dh = dr_is_letter(be, 4u) | dr_is_letter(be, 8u);
#pragma unroll
                for (int k = 0; k < 5; k++)
                    be[k] ^= (((11u >> k) & 1u) ? ry : 0ull) ^ (((6u >> k) & 1u) ? km : 0ull) ^      // 18 xor 25 = 11, 11 xor 13 = 6,
                             (((20u >> k) & 1u) ? bv : 0ull) ^ (((12u >> k) & 1u) ? dh : 0ull);      // 2 xor 22 = 20, 4 xor 8 = 12
            }
            u64 diff = 0;
#pragma unroll
            for (int k = 0; k < 5; k++) diff |= ae[k] ^ be[k];
            both_x &= ~diff;
        }
    }
    match |= both_x;
    return ~(match & inside);
}

}  // namespace
