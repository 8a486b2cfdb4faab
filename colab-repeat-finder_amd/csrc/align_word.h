// align_word.h -- what one lane of a wave does with one row of the alignment product (include/prf_align.h), and how the
// host sorts the rows.  A row is a repeat (start, end, k) of the range with a motif of k letters; its n_r positions are walked one
// after the other, and the k columns of the dynamic programming are dealt to the 64 lanes, C consecutive columns to a lane
// (C = 1, 2, 4, 8, 16: the regime of the row's k), kept in registers.  Everything that is per lane is here, so that the same text
// runs in the kernel of align.hip and, compiled for the host, against a plain dynamic programming (tests/align_word_check.cpp);
// what crosses lanes (the diagonal term of a lane's first column, the prefix minimum over the lanes' totals, the broadcast of
// the last column) is the kernel's, and the check's, between the calls.
//
// A CELL is the triple (edits, indels, consumed) in one u64, 20 / 20 / 21 bits from the top of bit 60 down, so that the
// lexicographic minimum is the integer minimum and adding a step adds its packed form.  Per position with base b, D the cells of
// the position before (all 0 before the first):
//     T[j]  = min(D[(j - 1) mod k] + (sub(b, M[j]), 0, 1), D[j] + (1, 1, 0))
//     P[j]  = min over j' <= j of T[j'] + (j - j') (1, 1, 1)                      deletions inside one turn of the motif
//     D'[j] = min(P[j], P[k - 1] + (j + 1) (1, 1, 1))                             ... and across its end, once
// The first pass is a prefix minimum over U[j] = T[j] + (k - 1 - j) (1, 1, 1), with the bias taken off again: every candidate of
// P[j] carries at least the bias of j in each field, so nothing borrows.  D'[k - 1] = P[k - 1], so the cell the diagonal term of
// column 0 needs is the broadcast value of the position before.
// THE FIELDS DO NOT OVERFLOW at the limits (k <= 1024, n_r <= 2^19): a cell of position i is at most the all-substitutions
// (i, 0, i) in the first field, so edits <= n_r <= 2^19, indels <= edits, and consumed = i - insertions + deletions <= 2 n_r <=
// 2^20.  A candidate adds at most one step and a bias or a wrap of at most 1024 (1, 1, 1) to a cell: edits and indels stay below
// 2^19 + 1026 < 2^20, consumed below 2^20 + 1026 < 2^21.  Bits 61 .. 63 stay free: the SENTINEL of a padded column is 2^62, which
// is above every cell and every candidate and which 2^19 + 1026 additions of steps cannot carry into bit 63.
#pragma once
#include <algorithm>
#include <vector>

#include "consensus_word.h"

#define PRF_AL_MAX_K 1024u             // = PRF_ALIGN_MAX_K
#define PRF_AL_MAX_LEN (1ull << 19)    // = PRF_ALIGN_MAX_LEN
#define PRF_AL_REGIMES 5u              // C = 1, 2, 4, 8, 16

namespace {

// ---- the cells
constexpr u32 AL_I_SHIFT = 21u, AL_E_SHIFT = 41u;
constexpr u64 AL_MATCH = 1ull;                                                  // (0, 0, 1)
constexpr u64 AL_SUB = (1ull << AL_E_SHIFT) | 1ull;                             // (1, 0, 1)
constexpr u64 AL_INS = (1ull << AL_E_SHIFT) | (1ull << AL_I_SHIFT);             // (1, 1, 0)
constexpr u64 AL_DEL = (1ull << AL_E_SHIFT) | (1ull << AL_I_SHIFT) | 1ull;      // (1, 1, 1)
constexpr u64 AL_SENTINEL = 1ull << 62;

PRF_CS_FN u64 al_pack(u32 edits, u32 indels, u32 consumed) { return ((u64)edits << AL_E_SHIFT) | ((u64)indels << AL_I_SHIFT) | (u64)consumed; }
PRF_CS_FN u32 al_edits(u64 v) { return (u32)(v >> AL_E_SHIFT) & 0xFFFFFu; }
PRF_CS_FN u32 al_indels(u64 v) { return (u32)(v >> AL_I_SHIFT) & 0xFFFFFu; }
PRF_CS_FN u32 al_consumed(u64 v) { return (u32)v & 0x1FFFFFu; }
PRF_CS_FN u64 al_min(u64 a, u64 b) { return a < b ? a : b; }

// ---- the deal: column j is slot j % C of lane j / C
PRF_CS_FN u32 al_regime(u32 k) { return k <= 64u ? 0u : k <= 128u ? 1u : k <= 256u ? 2u : k <= 512u ? 3u : 4u; }
PRF_CS_FN u32 al_lane_of(u32 j, u32 C) { return j / C; }
PRF_CS_FN u32 al_slot_of(u32 j, u32 C) { return j % C; }
PRF_CS_FN u32 al_real_lanes(u32 k, u32 C) { return (k + C - 1u) / C; }                  // the lanes that hold a column
PRF_CS_FN u32 al_real_slots(u32 k, u32 C, u32 lane) {                                    // ... and how many this one holds
    const u32 first = lane * C;
    return first >= k ? 0u : k - first < C ? k - first : C;
}
PRF_CS_FN u64 al_bias(u32 k, u32 j) { return (u64)(k - 1u - j) * AL_DEL; }               // j < k
PRF_CS_FN u64 al_wrap(u32 j) { return (u64)(j + 1u) * AL_DEL; }

// ---- the letters: a motif letter's code is 0 .. 3 for A, C, G, T (the bases of cs_base), 5 for N (a base is at most 4: no
// match); 0xFF: not a motif letter
PRF_CS_FN u32 al_motif_code(char ch) {
    switch (ch) {
    case 'A': case 'a': return 0u;
    case 'C': case 'c': return 1u;
    case 'G': case 'g': return 2u;
    case 'T': case 't': return 3u;
    case 'N': case 'n': return 5u;
    default: return 0xFFu;
    }
}

// the codes of a lane's C columns, four bits each; a padded column holds N's
template <int C>
PRF_CS_FN u64 al_lane_codes(const char *motif, u32 k, u32 lane) {
    u64 codes = 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const u32 j = lane * C + (u32)c;
        const u32 code = j < k ? al_motif_code(motif[j]) & 7u : 5u;
        codes |= (u64)code << (4 * c);
    }
    return codes;
}

// the cells before the first position: 0 in a column, the sentinel in a padded slot
template <int C>
PRF_CS_FN void al_lane_open(u64 *D, u32 real) {
#pragma unroll
    for (int c = 0; c < C; c++) D[c] = (u32)c < real ? 0ull : AL_SENTINEL;
}

// First half of a position: U of the lane's columns from D (unchanged) and the cell `diag` of the column in front of the lane's
// first, scanned within the lane.  Returns the lane's total, U of its last slot: the minimum over its columns, the sentinel if it
// has none.  bias0 = al_bias(k, lane * C) (unused by a lane without columns).
template <int C>
PRF_CS_FN u64 al_lane_scan(const u64 *D, u64 diag, u32 b, u64 codes, u32 real, u64 bias0, u64 *U) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        const u64 from = c ? D[c - 1] : diag;
        const u64 t = al_min(from + (((u32)(codes >> (4 * c)) & 15u) == b ? AL_MATCH : AL_SUB), D[c] + AL_INS);
        const u64 u = (u32)c < real ? t + (bias0 - (u64)c * AL_DEL) : AL_SENTINEL;
        U[c] = c ? al_min(u, U[c - 1]) : u;
    }
    return U[C - 1];
}

// Second half: D' from U, `before` = the minimum of the totals of the lanes in front (the sentinel for lane 0) and `last` =
// P[k - 1], the minimum of all totals.  A padded slot holds the sentinel again.
template <int C>
PRF_CS_FN void al_lane_wrap(const u64 *U, u64 before, u64 last, u32 real, u64 bias0, u32 col0, u64 *D) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        const u64 p = al_min(U[c], before) - (bias0 - (u64)c * AL_DEL);
        D[c] = (u32)c < real ? al_min(p, last + al_wrap(col0 + (u32)c)) : AL_SENTINEL;
    }
}

// ---- the final pick: the least cell, the first column that holds it
PRF_CS_FN void al_pick(u64 *best, u32 *best_col, u64 v, u32 col) {
    if (v < *best || (v == *best && col < *best_col)) {
        *best = v;
        *best_col = col;
    }
}

template <int C>
PRF_CS_FN void al_lane_pick(const u64 *D, u32 real, u32 col0, u64 *best, u32 *best_col) {
    *best = AL_SENTINEL;
    *best_col = 0xFFFFFFFFu;
#pragma unroll
    for (int c = 0; c < C; c++)
        if ((u32)c < real) al_pick(best, best_col, D[c], col0 + (u32)c);
}

struct al_result {    // = prf_alignment
    u32 edits, indels, consumed, start_column, end_column, reserved;
};

PRF_CS_FN al_result al_finish(u64 best, u32 col, u32 k) {
    const u32 consumed = al_consumed(best);
    return al_result{al_edits(best), al_indels(best), consumed, ((col + 1u) % k + k - consumed % k) % k, col, 0u};
}

// ---- the rows as the kernel sees them, sorted by the host: by regime and, within a regime, the longest first, so that the rows
// of a block and the last blocks of a launch are of a kind; `index` is where the result goes
struct al_row {
    u64 start, end;            // positions of the range
    u64 offset;                // of the row's letters in the motifs
    u32 k, index;
};

// sorts the rows (host) and counts them per regime
inline void al_sort_rows(std::vector<al_row> &rows, u64 *per_regime) {
    for (u32 i = 0; i < PRF_AL_REGIMES; i++) per_regime[i] = 0;
    for (const al_row &r : rows) ++per_regime[al_regime(r.k)];
    std::stable_sort(rows.begin(), rows.end(), [](const al_row &a, const al_row &b) {
        const u32 ra = al_regime(a.k), rb = al_regime(b.k);
        if (ra != rb) return ra < rb;
        return a.end - a.start > b.end - b.start;
    });
}

}  // namespace
