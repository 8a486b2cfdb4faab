// phased_word.h -- what one lane of a wave does with one work item of the consensus over phased segments (DESIGN 19;
// include/prf_phased.h).  A row is k columns; a segment [start, end) of the range belongs to a row and says, with its phase, that
// its position q lies in column (phase + q - start) mod k; an item is a slice [first, end) of a SEGMENT's positions.  Built on
// consensus_word.h: the same window over a source of plane words (every word that holds a position of the item ONCE, in ascending
// order, and no other), the same step and the same three regimes by the row's k.  Only the column of the item's first position
// differs from cs_count_item, so for k <= PRF_CS_REG_K a lane's column is still constant within an item.  The same text runs in
// the kernels of phased.hip and, compiled for the host, against a brute force (tests/phased_word_check.cpp).
#pragma once
#include "consensus_word.h"

namespace {

struct ph_segment {            // = prf_segment
    u64 start, end;            // positions of the range
    u32 row, phase;            // phase < the row's k
};

struct ph_item {
    u64 first, end;            // positions of the range: the segment's start <= first < end <= the segment's end
    u32 segment, reserved;
};

// the column of the item's first position: (phase + first - start) mod k, without a sum that could pass 2^64
PRF_CS_FN u32 ph_first_column(const ph_segment &s, u32 k, const ph_item &it) { return (u32)(((it.first - s.start) % k + s.phase) % k); }

// the column of lane `lane` at the item's first step; for k <= PRF_CS_REG_K at every step (lanes at and behind cs_step(k) have none)
PRF_CS_FN u32 ph_lane_column(const ph_segment &s, u32 k, const ph_item &it, u32 lane) { return (ph_first_column(s, k, it) + lane % k) % k; }

// What lane `lane` of the wave does with an item of a segment of a row of k columns: add(column, base) for every position of the
// item that is the lane's and is A, C, G or T.  Every value that steers the loop is the same in all lanes.  For k > PRF_CS_REG_K
// the 64 lanes of a step call with 64 different columns.
template <class S, class F>
PRF_CS_FN void ph_count_item(S &src, u64 g_begin, u32 k, const ph_segment &s, const ph_item &it, u32 lane, F &&add) {
    const u32 step = cs_step(k);
    u32 col = ph_lane_column(s, k, it, lane);
    cs_window<S> win;
    win.open(src, g_begin + it.first, g_begin + it.end - 1ull);
#pragma unroll 1
    for (u64 cur = it.first; cur < it.end; cur += step) {
        const u64 q = g_begin + cur;
        win.seek(src, q);
        const u32 b = win.base(q, lane);
        if (lane < step && cur + lane < it.end && b < 4u) add(col, b);
        if (k > PRF_CS_REG_K) {                     // 64 positions on: k > 64, so once around at most
            col += 64u;
            if (col >= k) col -= k;
        }
    }
}

}  // namespace
