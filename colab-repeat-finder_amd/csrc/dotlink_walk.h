// dotlink_walk.h -- the two walks of dotlink.hip along one line of the dot plot, over a source of 64-cell words of
// raw cells as dotchain_walk.h's: the chain's end (tail) in a stretch of a line and the chain's start (head) in a stretch.  They
// form no address and know nothing of the planes, so the same text runs in the kernel and, compiled for the host, against a brute
// force (tests/dotlink_walk_check.cpp).  Cells of a line are numbered t = 0, 1, ... from the cell with the smallest row;
// word(k): bit b = cell 64 k + b of the line is raw; cells behind the line's end are not raw, and neither is anything in front of
// cell 0: the line's edges behave as mismatches.
// The stretches are short (max_gap + min(min_seed - 1, 16) + 1 cells): among the seeds that end in one only the last can be a
// chain's end, among those that start in one only the first can be a chain's start (include/prf_dotlink.h).
// Each walk takes at most ceil((max_gap + 2 min_seed + 17) / 64) + 2 word steps in one direction, and ceil(min_seed / 64) + 1
// more where a run has to be followed until it has min_seed cells.
#pragma once
#include "dotchain_walk.h"

namespace {

// the first cell at or behind p that is raw (want) or not raw (!want); cells behind the line's end are not raw, so a look for a
// mismatch always ends.  A look for a raw cell gives up behind `limit` (any value > limit: none).
template <class F>
PRF_WALK_FN u64 dl_next(u64 p, bool want, u64 limit, F &&word) {
#pragma unroll 1
    for (;;) {
        const u64 k = p >> 6;
        const u64 w = word(k);
        const u64 m = (want ? w : ~w) & (~0ull << (p & 63));
        if (m) return 64ull * k + (u64)__builtin_ctzll(m);
        p = 64ull * (k + 1ull);
        if (p > limit) return p;
    }
}

// the last cell below p (cells p - 1, p - 2, ... 0) that is raw (want) or not; ~0ull: none down to cell `floor` (the look may
// give up once it is below floor; what it returns then is ~0ull or a cell below floor)
template <class F>
PRF_WALK_FN u64 dl_prev(u64 p, bool want, u64 floor, F &&word) {
#pragma unroll 1
    for (;;) {
        if (!p) return ~0ull;
        const u64 k = (p - 1ull) >> 6;
        const u64 w = word(k);
        const u32 n = (u32)(p - 64ull * k);             // 1 .. 64 bits of this word lie below p
        const u64 m = (want ? w : ~w) & (n == 64 ? ~0ull : (1ull << n) - 1ull);
        if (m) return 64ull * k + 63ull - (u64)__builtin_clzll(m);
        p = 64ull * k;
        if (p <= floor) return ~0ull;
    }
}

// TAIL IN STRETCH: the last cell of the chain that ends in cells lo .. hi of the line, or ~0ull.  lo <= hi; hi may lie behind
// the line's end.  The last seed whose last cell lies in the stretch is found by walking down from hi; a run that reaches into
// the stretch is followed back past lo until it has min_seed cells.  That seed ends a chain iff no seed starts in the max_gap
// cells behind its mismatch.
template <class F>
PRF_WALK_FN u64 dl_tail_in_stretch(u64 lo, u64 hi, u64 min_seed, u32 max_gap, F &&word) {
    u64 p = hi + 1ull;                                  // cells below p are still to be looked at
    // a run that holds cell hi + 1 does not end in the stretch: step over its cells
    if ((word(p >> 6) >> (p & 63)) & 1ull) {
        const u64 x = dl_prev(p, false, lo, word);
        if (x == ~0ull || x < lo) return ~0ull;
        p = x;
    }
    u64 e;
#pragma unroll 1
    for (;;) {
        e = dl_prev(p, true, lo, word);                 // a run's last cell: cell e + 1 is not raw
        if (e == ~0ull || e < lo) return ~0ull;
        const u64 floor = e + 1ull >= min_seed ? e + 1ull - min_seed : 0ull;     // a mismatch at or above it: the run is too short
        const u64 x = dl_prev(e, false, floor, word);
        if (x == ~0ull || x < floor) {
            if (e + 1ull >= min_seed) break;            // cells e - min_seed + 1 .. e are raw: a seed
            return ~0ull;                               // the run begins with the line and is too short
        }
        p = x;                                          // the run is x + 1 .. e, shorter than min_seed
    }
    // no seed starts in e + 2 .. e + 1 + max_gap
    const u64 last = e + 1ull + max_gap;
    p = e + 2ull;
#pragma unroll 1
    for (;;) {
        if (p > last) return e;
        const u64 s = dl_next(p, true, last, word);
        if (s > last) return e;
        const u64 x = dl_next(s, false, s + min_seed - 1ull, word);   // the run is s .. x - 1, if it is shorter than min_seed
        if (x - s >= min_seed) return ~0ull;
        p = x + 1ull;
    }
}

// HEAD IN STRETCH: the first cell of the chain that starts in cells lo .. hi of the line, or ~0ull: the first maximal run of at
// least min_seed cells that starts there, if dc_is_head holds for it.
template <class F>
PRF_WALK_FN u64 dl_head_in_stretch(u64 lo, u64 hi, u64 min_seed, u32 max_gap, F &&word) {
    u64 p = lo;
    // a run that holds cell lo - 1 does not start in the stretch: step over its cells
    if (lo && ((word((lo - 1ull) >> 6) >> ((lo - 1ull) & 63)) & 1ull)) p = dl_next(lo, false, hi, word) + 1ull;
#pragma unroll 1
    for (;;) {
        if (p > hi) return ~0ull;
        const u64 s = dl_next(p, true, hi, word);
        if (s > hi) return ~0ull;
        // the run's first mismatch, looked for over min_seed cells only: a run may be as long as the line
        const u64 x = dl_next(s, false, s + min_seed - 1ull, word);
        if (x - s >= min_seed) return dc_is_head(s, min_seed, max_gap, word) ? s : ~0ull;
        p = x + 1ull;
    }
}

}  // namespace
