// alignlocal_word.h -- what one lane of a wave does with one row of the local alignment product (DESIGN 22;
// include/prf_alignlocal.h).  A row is a window (start, end, k) of the range with a motif of k letters; the deal of the k columns to
// the 64 lanes, the motif codes and the host's sort are align_word.h's, unchanged.  Everything that is per lane is here, so that
// the same text runs in the kernel of alignlocal.hip and, compiled for the host, against the recurrence on explicit triples
// (tests/alignlocal_word_check.cpp); what crosses lanes is the kernel's, and the check's, between the calls.
//
// A CELL is the triple (score, p, a) in one u64: the score in 25 bits above p (19 bits) above a (10 bits), 54 bits in all, so that
// the lexicographic maximum is the integer maximum and a step adds to the score field only.  ZERO is any cell of score 0; what
// its labels say is never read.  sub(v, w) keeps the labels and takes w off the score if score > w, else it is 0: it compares
// before it subtracts, so no field borrows.  Per position i with base b, D the cells of the position before (all 0 before the
// first):
//     din   = D[(j - 1) mod k];  if din.score == 0: din = (0, i, j)                a fresh start takes its label here
//     T[j]  = max(match(b, M[j]) ? din + (match, 0, 0) : sub(din, mismatch), sub(D[j], indel))
//     P[j]  = max over j' <= j of sub(T[j'], (j - j') indel)                       deletions inside one turn of the motif
//     D'[j] = max(P[j], sub(P[k - 1], (j + 1) indel))                              ... and across its end, once
//     best: for j ascending, if D'[j].score > best.score (strictly): best = (D'[j], end = i + 1, end_column = j)
// The first pass is a prefix maximum over U[j] = T[j] + j indel (on the score field), with the bias taken off again: U[j] itself
// is among the candidates of P[j], so the result is at least T[j] >= 0 and nothing borrows.  A cell of score 0 may then carry the
// label of another column; that is harmless: the diagonal step replaces it, sub drops it, the best never takes a score of 0.
// D'[k - 1] = P[k - 1], so the cell the diagonal term of column 0 needs is the broadcast value of the position before.
// THE FIELDS DO NOT OVERFLOW at the limits (k <= 1024, n_r <= 2^19, weights <= 16): a score is at most 16 n_r <= 2^23, and the
// bias is at most 1023 x 16 < 2^14 on top: below 2^25.  p < 2^19, a < 2^10.  A PADDED SLOT holds 0, and U of it is 0: the neutral
// element of the maximum; it sits behind the lane's columns and in the lanes behind them, so neither the diagonal term nor the
// prefix carries it into a column.
#pragma once
#include "align_word.h"

#define PRF_ALL_MAX_WEIGHT 16u         // = PRF_ALIGNLOCAL_MAX_WEIGHT

namespace {

// ---- the cells
constexpr u32 ALL_P_SHIFT = 10u, ALL_S_SHIFT = 29u;
constexpr u64 ALL_UNIT = 1ull << ALL_S_SHIFT;                                   // (1, 0, 0)
constexpr u32 ALL_P_MASK = 0x7FFFFu, ALL_A_MASK = 0x3FFu;

PRF_CS_FN u64 all_pack(u32 score, u32 p, u32 a) { return ((u64)score << ALL_S_SHIFT) | ((u64)p << ALL_P_SHIFT) | (u64)a; }
PRF_CS_FN u32 all_score(u64 v) { return (u32)(v >> ALL_S_SHIFT); }
PRF_CS_FN u32 all_p(u64 v) { return (u32)(v >> ALL_P_SHIFT) & ALL_P_MASK; }
PRF_CS_FN u32 all_a(u64 v) { return (u32)v & ALL_A_MASK; }
PRF_CS_FN u64 all_max(u64 a, u64 b) { return a > b ? a : b; }
PRF_CS_FN u64 all_weight(u32 w) { return (u64)w << ALL_S_SHIFT; }               // w on the score field
// v with w (a multiple of ALL_UNIT) off its score if the score is above w's, else 0
PRF_CS_FN u64 all_sub(u64 v, u64 w) { return v >= w + ALL_UNIT ? v - w : 0ull; }
// the label a fresh start takes: position i of the row, column j
PRF_CS_FN u64 all_fresh(u32 i, u32 j) { return ((u64)i << ALL_P_SHIFT) | (u64)j; }

struct all_weights {       // the three weights on the score field
    u64 match, mismatch, indel;
};
PRF_CS_FN all_weights all_weights_of(u32 match, u32 mismatch, u32 indel) {
    return all_weights{all_weight(match), all_weight(mismatch), all_weight(indel)};
}

// First half of a position: U of the lane's columns from D (unchanged) and the cell `diag` of the column in front of the lane's
// first, scanned within the lane.  Returns the lane's total, U of its last slot: the maximum over its columns, 0 if it has none.
// bias0 = col0 x indel on the score field, fresh0 = all_fresh(i, col0).
template <int C>
PRF_CS_FN u64 all_lane_scan(const u64 *D, u64 diag, u32 b, u64 codes, u32 real, u64 bias0, u64 fresh0, const all_weights &w, u64 *U) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        u64 from = c ? D[c - 1] : diag;
        if (from < ALL_UNIT) from = fresh0 + (u64)c;
        const u64 step = ((u32)(codes >> (4 * c)) & 15u) == b ? from + w.match : all_sub(from, w.mismatch);
        const u64 t = all_max(step, all_sub(D[c], w.indel));
        const u64 u = (u32)c < real ? t + (bias0 + (u64)c * w.indel) : 0ull;
        U[c] = c ? all_max(u, U[c - 1]) : u;
    }
    return U[C - 1];
}

// P[k - 1] from the maximum of all totals
PRF_CS_FN u64 all_last(u64 total, u32 k, const all_weights &w) { return total - (u64)(k - 1u) * w.indel; }

// Second half: D' from U, `before` = the maximum of the totals of the lanes in front (0 for lane 0) and `last` = P[k - 1].  A
// padded slot holds 0 again.
template <int C>
PRF_CS_FN void all_lane_wrap(const u64 *U, u64 before, u64 last, u32 real, u64 bias0, const all_weights &w, u64 *D) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        const u64 bias = bias0 + (u64)c * w.indel;
        const u64 p = all_max(U[c], before) - bias;
        D[c] = (u32)c < real ? all_max(p, all_sub(last, bias + w.indel)) : 0ull;
    }
}

// ---- the running best: a key (the score, then the inverted position, then the inverted column, so that the maximum is the
// greatest score, its earliest end and its least column) and the cell that carries the labels
constexpr u64 ALL_WHERE_MASK = ALL_UNIT - 1ull;
PRF_CS_FN u64 all_where(u32 i, u32 j) { return ((u64)(~i & ALL_P_MASK) << ALL_P_SHIFT) | (u64)(~j & ALL_A_MASK); }
PRF_CS_FN u64 all_key(u64 cell, u64 where) { return (cell & ~ALL_WHERE_MASK) | where; }

struct all_best {
    u64 key, cell;
};

// the lane's columns of position i, in ascending order: only a strictly greater score is taken.  where0 = all_where(i, col0); the
// inverted column of slot c is that of col0 less c (col0 + c < 1024: no borrow into the position).
template <int C>
PRF_CS_FN void all_lane_best(const u64 *D, u64 where0, all_best *best) {
#pragma unroll
    for (int c = 0; c < C; c++)
        if (all_score(D[c]) > all_score(best->key)) {
            best->key = all_key(D[c], where0 - (u64)c);
            best->cell = D[c];
        }
}

// between lanes: the keys of two lanes differ unless both are 0
PRF_CS_FN void all_pick(all_best *best, u64 key, u64 cell) {
    if (key > best->key) {
        best->key = key;
        best->cell = cell;
    }
}

struct all_result {    // = prf_local_alignment
    u32 score, first, end, start_column, end_column, reserved;
};

PRF_CS_FN all_result all_finish(const all_best &best) {
    if (!all_score(best.key)) return all_result{0u, 0u, 0u, 0u, 0u, 0u};
    return all_result{all_score(best.key), all_p(best.cell), (~(u32)(best.key >> ALL_P_SHIFT) & ALL_P_MASK) + 1u, all_a(best.cell),
                      ~(u32)best.key & ALL_A_MASK, 0u};
}

}  // namespace
