// alignpath_word.h -- what one lane of a wave does with one row of the alignment-path product (include/prf_alignpath.h),
// and how the host deals the rows into batches.  The forward pass is align_word.h's recurrence, cell for cell, plus TWO BITS per
// cell (position i, column j), D the cells of the position before:
//     from_ins = D[j] + (1, 1, 0) < D[(j - 1) mod k] + (sub, 0, 1)               strictly: ties go to the diagonal
//     from_del = D'[j] < T[j]                                                     strictly: the cell came from the column to its left
// D'[j] = min(T[j], D'[(j - 1) mod k] + (1, 1, 1)) holds at every cell, so a deletion cell's predecessor is the column to its
// left, around the wrap as well.  from_del is had without keeping T: per slot a bit "u was its own prefix minimum within the lane"
// (U[c] == u[c]); then D' < T iff that bit is clear, or the lanes in front hold less (before < U[c]), or the wrap term won.
//
// THE TRACE of a row of n positions in regime R (C = 1 << R columns per lane): 2 C bits per lane and position, 32 / (2 C)
// positions (a GROUP) to one u32 per lane; word [group][lane], so that a wave writes and reads a group as 256 consecutive bytes.
// Bit 2 c of a position's field is from_ins of slot c, bit 2 c + 1 from_del.
//
// THE WALK goes from (n - 1, end_column) down; its state (i, j) is the same in all lanes, and one step of it is ap_walk_step.
// The same text runs in the kernels of alignpath.hip and, compiled for the host, against a full-matrix traceback on explicit
// triples (tests/alignpath_word_check.cpp).
#pragma once
#include "align_word.h"

#define PRF_AP_MAX_POSITIONS (1ull << 30)      // = PRF_ALIGNPATH_MAX_POSITIONS
#define PRF_AP_INS 0x8000u                     // = PRF_PATH_INS
#define PRF_AP_SUB 0x4000u                     // = PRF_PATH_SUB
#define PRF_AP_COLUMN 0x03FFu                  // = PRF_PATH_COLUMN

namespace {

// ---- the trace's layout
PRF_CS_FN u32 ap_group_shift(u32 regime) { return 4u - regime; }                             // log2 of the positions per word
PRF_CS_FN u32 ap_group_positions(u32 regime) { return 16u >> regime; }
PRF_CS_FN u32 ap_n_groups(u32 n, u32 regime) { return (n + ap_group_positions(regime) - 1u) >> ap_group_shift(regime); }
PRF_CS_FN u64 ap_trace_words(u32 n, u32 regime) { return (u64)ap_n_groups(n, regime) * 64ull; }    // u32 words of a row
PRF_CS_FN u64 ap_word_index(u32 i, u32 lane, u32 regime) { return (u64)(i >> ap_group_shift(regime)) * 64ull + lane; }
PRF_CS_FN u32 ap_field_shift(u32 i, u32 regime) { return (i & (ap_group_positions(regime) - 1u)) << (regime + 1u); }
// the two bits of (i, j) from the word of lane j >> regime of i's group
PRF_CS_FN u32 ap_code(u32 word, u32 i, u32 j, u32 regime) {
    return (word >> (ap_field_shift(i, regime) + 2u * (j & ((1u << regime) - 1u)))) & 3u;
}
PRF_CS_FN u32 ap_prev(u32 j, u32 k) { return j ? j - 1u : k - 1u; }

// ---- the forward pass: al_lane_scan and al_lane_wrap with the bits.  `bits` collects the lane's field of this position
// (from_ins here, from_del in the second half), `own` the slots whose u was its own prefix minimum.
template <int C>
PRF_CS_FN u64 ap_lane_scan(const u64 *D, u64 diag, u32 b, u64 codes, u32 real, u64 bias0, u64 *U, u32 *bits, u32 *own) {
    u32 f = 0, o = 1u;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const u64 from = c ? D[c - 1] : diag;
        const u64 across = from + (((u32)(codes >> (4 * c)) & 15u) == b ? AL_MATCH : AL_SUB), down = D[c] + AL_INS;
        const u64 t = al_min(across, down);
        f |= (down < across ? 1u : 0u) << (2 * c);
        const u64 u = (u32)c < real ? t + (bias0 - (u64)c * AL_DEL) : AL_SENTINEL;
        if (c) o |= (u <= U[c - 1] ? 1u : 0u) << c;
        U[c] = c ? al_min(u, U[c - 1]) : u;
    }
    *bits = f;
    *own = o;
    return U[C - 1];
}

template <int C>
PRF_CS_FN void ap_lane_wrap(const u64 *U, u64 before, u64 last, u32 real, u64 bias0, u32 col0, u32 own, u64 *D, u32 *bits) {
    u32 f = *bits;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const u64 p = al_min(U[c], before) - (bias0 - (u64)c * AL_DEL);
        const u64 d = al_min(p, last + al_wrap(col0 + (u32)c));
        const bool del = !((own >> c) & 1u) || before < U[c] || d < p;
        f |= ((u32)c < real && del ? 2u : 0u) << (2 * c);
        D[c] = (u32)c < real ? d : AL_SENTINEL;
    }
    *bits = f;
}

// a position's field into the lane's word of its group; true: the word is full or the row ends, store it and start anew
PRF_CS_FN bool ap_pack(u32 *word, u32 bits, u32 i, u32 n, u32 regime) {
    *word |= bits << ap_field_shift(i, regime);
    return ((i + 1u) & (ap_group_positions(regime) - 1u)) == 0u || i + 1u == n;
}

// ---- the walk.  One step at (i, *j) with the cell's two bits: a deletion moves *j and returns false (the position stays); else
// *entry is the position's path entry without the SUB bit (the counts kernel sets it), *j the column of the position before, and
// the step returns true.
PRF_CS_FN bool ap_walk_step(u32 code, u32 k, u32 *j, u32 *entry) {
    if (code & 2u) {
        *j = ap_prev(*j, k);
        return false;
    }
    *entry = *j | ((code & 1u) ? PRF_AP_INS : 0u);
    if (!(code & 1u)) *j = ap_prev(*j, k);
    return true;
}

// ---- the rows as the kernels see them: al_row (sorted by al_sort_rows) and where the row's trace and path are
struct ap_row {
    u64 start, end;            // positions of the range
    u64 offset;                // of the row's letters in the motifs and (x 6) of its counts
    u32 k, index;              // index: where the result goes
    u64 trace;                 // the row's first u32 of the batch's trace
    u64 path;                  // the row's first entry of the path
};

// ---- the batches: the sorted rows dealt, in their order, into runs whose trace fits `budget` u32 words; a row that alone needs
// more gets a batch of its own.  Sets every row's `trace`; a batch is rows [row0, row0 + n_rows) and holds `words`.
struct ap_batch {
    u64 row0, n_rows, words;
};

inline void ap_deal(std::vector<ap_row> &rows, u64 budget, std::vector<ap_batch> &out) {
    out.clear();
    ap_batch cur{0, 0, 0};
    for (u64 at = 0; at < rows.size(); at++) {
        ap_row &r = rows[at];
        const u64 need = ap_trace_words((u32)(r.end - r.start), al_regime(r.k));
        if (cur.n_rows && cur.words + need > budget) {
            out.push_back(cur);
            cur = ap_batch{at, 0, 0};
        }
        r.trace = cur.words;
        cur.words += need;
        ++cur.n_rows;
    }
    if (cur.n_rows) out.push_back(cur);
}

}  // namespace
