// periodchain_word.h -- the word source of the period lines of ONE range (include/prf_periodchain.h): 64 cells of
// line k per call, cell t = raw(s[t], s[t + k]) for t < n - k, s = the n positions from global position g_begin of linear
// planes.  No strand, no anti lines.  Both N rules: n_matches 1 = the periodicity matrix's cell (N == N matches), n_matches 0 =
// the same and the symbol is not N (the reference tracker's rule).  Written over a plane accessor
//     u64 h(u64 w), l(u64 w), x(u64 w), e(int i, u64 w);  bool exotic()
// (word w of the planes H, L, X, E[i]; exotic(): the five letter planes exist), so that the same text runs in the kernels of
// periodchain.hip and, compiled for the host, against a brute force (tests/periodchain_word_check.cpp).
// No word outside first .. last, the words of the planes that hold [g_begin, g_begin + n), is ever asked of the accessor.
#pragma once
#include "dotchain_walk.h"

namespace {

struct pc_range {
    u64 g_begin, n;         // the range, in global positions; n > 0
    u64 first, last;        // the words of the planes that hold it
    u32 n_matches;
};

PRF_WALK_FN pc_range pc_range_of(u64 g_begin, u64 n, u32 n_matches) {
    return pc_range{g_begin, n, g_begin >> 6, (g_begin + n - 1ull) >> 6, n_matches};
}

PRF_WALK_FN u64 pc_fsr(u64 lo, u64 hi, u32 s) { return s ? (lo >> s) | (hi << (64u - s)) : lo; }

// the raw cells of 64 pairs of symbols given by their planes; ae / be are read only if exotic
PRF_WALK_FN u64 pc_cells(u64 ah, u64 al, u64 ax, const u64 *ae, u64 bh, u64 bl, u64 bx, const u64 *be, bool exotic, u32 n_matches) {
    const u64 acgt = ~(ax | bx) & ~((ah ^ bh) | (al ^ bl));
    u64 other = ax & bx;                            // both outside ACGT: N, or a letter of the five planes
    if (exotic) {
        u64 diff = 0, letter = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) diff |= ae[i] ^ be[i], letter |= ae[i];
        other &= ~diff;
        if (!n_matches) other &= letter;            // N spells 0 in the five planes
    } else if (!n_matches) {
        other = 0;                                  // without the five planes every such symbol is N
    }
    return acgt | other;
}

// 64 bits of one plane from global position q; words outside first .. last read as 0 and are not asked for
template <class G>
PRF_WALK_FN u64 pc_bits(const pc_range &r, u64 q, G &&get) {
    const u64 w = q >> 6;
    const u64 lo = (w >= r.first && w <= r.last) ? get(w) : 0ull;
    const u64 hi = (w + 1ull >= r.first && w + 1ull <= r.last) ? get(w + 1ull) : 0ull;
    return pc_fsr(lo, hi, (u32)(q & 63ull));
}

// word wk of line k: bit b = cell 64 wk + b is raw; cells at and behind n - k (and every cell of a line k >= n) are 0
template <class A>
PRF_WALK_FN u64 pc_word(const A &pl, const pc_range &r, u64 k, u64 wk) {
    if (k >= r.n || wk >= ((r.n - k + 63ull) >> 6)) return 0ull;
    const u64 lim = r.n - k - 64ull * wk;           // > 0
    const u64 inside = lim >= 64ull ? ~0ull : (1ull << lim) - 1ull;
    const u64 qa = r.g_begin + 64ull * wk, qb = qa + k;
    const u64 ah = pc_bits(r, qa, [&](u64 w) { return pl.h(w); }), bh = pc_bits(r, qb, [&](u64 w) { return pl.h(w); });
    const u64 al = pc_bits(r, qa, [&](u64 w) { return pl.l(w); }), bl = pc_bits(r, qb, [&](u64 w) { return pl.l(w); });
    const u64 ax = pc_bits(r, qa, [&](u64 w) { return pl.x(w); }), bx = pc_bits(r, qb, [&](u64 w) { return pl.x(w); });
    u64 ae[5] = {0, 0, 0, 0, 0}, be[5] = {0, 0, 0, 0, 0};
    // without a pair of symbols outside ACGT among the word's cells the five planes decide nothing and are not read
    if (pl.exotic() && (ax & bx & inside) != 0ull) {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            ae[i] = pc_bits(r, qa, [&](u64 w) { return pl.e(i, w); });
            be[i] = pc_bits(r, qb, [&](u64 w) { return pl.e(i, w); });
        }
    }
    return pc_cells(ah, al, ax, ae, bh, bl, bx, be, pl.exotic(), r.n_matches) & inside;
}

// Walks forward from cell p, which lies in a run, to the run's end: true with p = the first cell behind the run (a mismatch
// or the line's end); false with p >= stop if the run is still going there.  word(k) as in dotchain_walk.h.
template <class F>
PRF_WALK_FN bool pc_run_end(u64 &p, u64 stop, F &&word) {
#pragma unroll 1
    for (;;) {
        if (p >= stop) return false;
        const u64 k = p >> 6;
        const u64 m = ~word(k) & (~0ull << (p & 63ull));
        if (m) {
            p = 64ull * k + (u64)__builtin_ctzll(m);
            return true;
        }
        p = 64ull * (k + 1ull);
    }
}

}  // namespace
