// periodlink_step.h -- the arithmetic of one junction between two period lines (include/prf_periodlink.h): which shift
// a lane of the join kernel stands for, the stretch of its line in which a chain's end (step A) or start (step B) makes a
// candidate, the packed key, and which lane holds Y's line.  With the walks of dotlink_walk.h over a source of line words
//     u64 line(u64 k, u64 wk)      word wk of line k: bit b = cell 64 wk + b is raw; 0 behind the line's end
// (in the kernel: pc_word of periodchain_word.h behind a one-word cache, kept here) this is everything a lane does between the
// two wave minima of prf_periodlink_join_kernel.  It forms no address and knows nothing of the planes, so the same text runs in
// the kernel and, compiled for the host, against a brute force (tests/periodlink_step_check.cpp).
// A cell of line k is (i, c) = (t, t + k): delta = k, every line begins at i = 0, so a line's cell number IS its row.
// Lane l stands for the shift s = l - 32 (l < 32) or l - 31: -32 .. -1, 1 .. 32.  A packed key is
// (m + |s|) << 12 | |s| << 6 | o << 1 | (s < 0), as in dotlink.hip: m <= 4096, |s| <= 32, o <= 16.
#pragma once
#include "../../include/prf.h"
#include "dotlink_walk.h"

namespace {

typedef long long pl_i64;

static_assert(PRF_DOTLINK_MAX_SHIFT == 32, "one lane of a wave per shift");
static_assert(PRF_DOTCHAIN_MAX_GAP + PRF_DOTLINK_MAX_SHIFT < (1u << 13) && PRF_DOTLINK_OVERLAP < 32, "the packed key");

#define PL_NO_KEY (~0u)

struct pl_params {
    u64 n;                  // positions of the range: the lines 1 .. n - 1 take part
    u64 min_seed;
    u32 max_gap, max_shift;
};

struct pl_stretch {
    u64 k;                  // the lane's line
    pl_i64 base;            // the cell of that line with g = 0
    u64 lo, hi;             // the cells to look at: lo <= hi, lo inside the line, hi possibly behind its end
};

PRF_WALK_FN u32 pl_lane_shift(u32 lane) { return lane < 32u ? 32u - lane : lane - 31u; }   // |s|
PRF_WALK_FN bool pl_lane_neg(u32 lane) { return lane < 32u; }

PRF_WALK_FN pl_i64 pl_ov(u64 min_seed) { return (pl_i64)(min_seed - 1ull < PRF_DOTLINK_OVERLAP ? min_seed - 1ull : PRF_DOTLINK_OVERLAP); }

PRF_WALK_FN u32 pl_key(pl_i64 g, u32 shift, bool neg) {
    const u32 m = g > 0 ? (u32)g : 0u, o = g < 0 ? (u32)-g : 0u;
    return (m + shift) << 12 | shift << 6 | o << 1 | (neg ? 1u : 0u);
}

PRF_WALK_FN u32 pl_key_most(u32 key) { return key >> 12; }                     // m + |s|
PRF_WALK_FN u32 pl_key_abs_shift(u32 key) { return (key >> 6) & 63u; }
PRF_WALK_FN int pl_key_shift(u32 key) { return (key & 1u) ? -(int)pl_key_abs_shift(key) : (int)pl_key_abs_shift(key); }
PRF_WALK_FN u32 pl_key_overlap(u32 key) { return (key >> 1) & 31u; }
PRF_WALK_FN u32 pl_key_lane(u32 key) { return (key & 1u) ? 32u - pl_key_abs_shift(key) : 31u + pl_key_abs_shift(key); }

// the lane's line k + s, if it takes part
PRF_WALK_FN bool pl_line(const pl_params &p, u64 k, pl_i64 s, u64 *line) {
    const pl_i64 other = (pl_i64)k + s;
    if (other < 1 || other > (pl_i64)p.n - 1) return false;
    *line = (u64)other;
    return true;
}

// STEP A, lane of shift s: on line k_Y - s the chain X that ends with g = base - t_e in [-ov, max_gap].  For s > 0 the rows are
// closer (g = gi = t_s - t_e - 1), for s < 0 the columns (g = gi + s).
PRF_WALK_FN bool pl_stretch_a(const pl_params &p, u64 t_s, u64 k_y, u32 lane, pl_stretch *o) {
    const u32 shift = pl_lane_shift(lane);
    const bool neg = pl_lane_neg(lane);
    if (shift > p.max_shift) return false;
    const pl_i64 s = neg ? -(pl_i64)shift : (pl_i64)shift;
    if (!pl_line(p, k_y, -s, &o->k)) return false;
    o->base = (pl_i64)t_s - 1ll + (neg ? s : 0ll);
    const pl_i64 lo = o->base - (pl_i64)p.max_gap, hi = o->base + pl_ov(p.min_seed);
    if (hi < 0 || lo >= (pl_i64)(p.n - o->k)) return false;
    o->lo = lo > 0 ? (u64)lo : 0ull;
    o->hi = (u64)hi;
    return true;
}

// STEP B, lane of shift s': on line k_X + s' the chain Y' that starts with g = t_s' - base in [-ov, max_gap].  The stretch is
// cut where it can only hold keys larger than key(X, Y): gaps above most - |s'|, most = m + |s| of key(X, Y).
PRF_WALK_FN bool pl_stretch_b(const pl_params &p, u64 t_e, u64 k_x, u32 lane, u32 most, pl_stretch *o) {
    const u32 shift = pl_lane_shift(lane);
    const bool neg = pl_lane_neg(lane);
    if (shift > p.max_shift || shift > most) return false;
    const pl_i64 s = neg ? -(pl_i64)shift : (pl_i64)shift;
    if (!pl_line(p, k_x, s, &o->k)) return false;
    o->base = (pl_i64)t_e + 1ll - (neg ? s : 0ll);
    const pl_i64 room = (pl_i64)(most - shift);
    const pl_i64 lo = o->base - pl_ov(p.min_seed), hi = o->base + (room < (pl_i64)p.max_gap ? room : (pl_i64)p.max_gap);
    if (hi < 0 || lo >= (pl_i64)(p.n - o->k)) return false;
    o->lo = lo > 0 ? (u64)lo : 0ull;
    o->hi = (u64)hi;
    return true;
}

// What a lane does in step A: its packed key(X, Y), or PL_NO_KEY; *x_end = X's last cell
template <class L>
PRF_WALK_FN u32 pl_step_a(const pl_params &p, u64 t_s, u64 k_y, u32 lane, L &&line, u64 *x_end) {
    pl_stretch st;
    if (!pl_stretch_a(p, t_s, k_y, lane, &st)) return PL_NO_KEY;
    u64 have = ~0ull, word = 0;                          // the word looked at last
    const u64 e = dl_tail_in_stretch(st.lo, st.hi, p.min_seed, p.max_gap, [&](u64 wk) {
        if (wk != have) word = line(st.k, wk), have = wk;
        return word;
    });
    if (e == ~0ull) return PL_NO_KEY;
    *x_end = e;
    return pl_key(st.base - (pl_i64)e, pl_lane_shift(lane), pl_lane_neg(lane));
}

// ... and in step B, X = (k_x, t_e) and best = key(X, Y) being the same in all lanes: its packed key(X, Y'), or PL_NO_KEY;
// *is_y: Y' starts at cell t_s (on Y's line it is then Y)
template <class L>
PRF_WALK_FN u32 pl_step_b(const pl_params &p, u64 t_e, u64 k_x, u32 lane, u32 best, u64 t_s, L &&line, bool *is_y) {
    pl_stretch st;
    if (!pl_stretch_b(p, t_e, k_x, lane, pl_key_most(best), &st)) return PL_NO_KEY;
    u64 have = ~0ull, word = 0;
    const u64 t = dl_head_in_stretch(st.lo, st.hi, p.min_seed, p.max_gap, [&](u64 wk) {
        if (wk != have) word = line(st.k, wk), have = wk;
        return word;
    });
    if (t == ~0ull) return PL_NO_KEY;
    *is_y = t == t_s;
    return pl_key((pl_i64)t - st.base, pl_lane_shift(lane), pl_lane_neg(lane));
}

}  // namespace
