// consensus_word.h -- what one lane of a wave does with one work item of the consensus product (DESIGN 18;
// include/prf_consensus.h), and how the host cuts rows into items.  A row is a repeat (start, end, k) of the range that begins at
// global position g_begin of linear planes; an item is a slice [first, end) of a row's positions; column p of the row holds the
// positions start + p + j k.  Written over a source of plane words
//     void take(u64 w, u64 out[3])      word w of the planes H, L, X
// so that the same text runs in the kernels of consensus.hip and, compiled for the host, against a brute force
// (tests/consensus_word_check.cpp).  The source is asked for the words that hold the item's positions, each ONCE, in ascending
// order, and for no other word; only H, L and X are read.
#pragma once
#ifdef __HIPCC__
#include "prf_device.h"
#define PRF_CS_FN __host__ __device__ __forceinline__
#else
#include <stdint.h>
typedef uint32_t u32;
typedef unsigned long long u64;
#define PRF_CS_FN inline
#endif

#define PRF_CS_REG_K 64u       // k up to here: a lane's column never changes, four counters per lane
#define PRF_CS_LDS_K 1024u     // k up to here: the counters of an item live in the wave's LDS region; above: adds go to the global counts

namespace {

// ---- the rows as the kernels see them, and the items the host cuts them into
struct cs_row {
    u64 start, end;            // positions of the range
    u64 offset;                // of the row's columns in the counts and the motifs
    u32 k, reserved;
};

struct cs_item {
    u64 first, end;            // positions of the range: start <= first < end <= the row's end
    u32 row, reserved;
};

enum { PRF_CS_REG = 0, PRF_CS_LDS = 1, PRF_CS_GLOBAL = 2, PRF_CS_REGIMES = 3 };

PRF_CS_FN u32 cs_regime(u32 k) { return k <= PRF_CS_REG_K ? PRF_CS_REG : k <= PRF_CS_LDS_K ? PRF_CS_LDS : PRF_CS_GLOBAL; }

// the items of a row of `len` positions at `slice` positions each (slice >= 1), and item j of them, relative to the row's start
PRF_CS_FN u64 cs_n_items(u64 len, u64 slice) { return len / slice + (len % slice ? 1ull : 0ull); }
PRF_CS_FN void cs_item_span(u64 len, u64 slice, u64 j, u64 *first, u64 *end) {
    *first = j * slice;
    *end = len - *first > slice ? *first + slice : len;
}

// positions per step: whole copies of the motif as long as 64 lanes hold one, so that a lane's column never changes; else 64
PRF_CS_FN u32 cs_step(u32 k) { return k <= PRF_CS_REG_K ? (64u / k) * k : 64u; }

PRF_CS_FN u64 cs_fsr(u64 lo, u64 hi, u32 s) { return s ? (lo >> s) | (hi << (64u - s)) : lo; }

// the base of bit `bit` of 64 positions given by their planes: 0 .. 3 for A, C, G, T (the planes' code is A, C, T, G); 4: none of them
PRF_CS_FN u32 cs_base(u64 h, u64 l, u64 x, u32 bit) {
    const u32 code = (u32)(((h >> bit) & 1ull) << 1) | (u32)((l >> bit) & 1ull);
    return ((x >> bit) & 1ull) ? 4u : code ^ (code >> 1);
}

// 64 positions of H, L, X from a global position that moves forward by at most 64 per step, over the words first .. last of the
// planes (those that hold the item): every word is taken once, in ascending order; a word behind `last` reads as 0 and is not taken
template <class S>
struct cs_window {
    u64 w, last;
    u64 lo[3], hi[3];
    PRF_CS_FN void fetch(S &src, u64 word, u64 *out) {
        if (word <= last) src.take(word, out);
        else out[0] = out[1] = out[2] = 0ull;
    }
    PRF_CS_FN void open(S &src, u64 q, u64 q_last) {
        w = q >> 6;
        last = q_last >> 6;
        fetch(src, w, lo);
        fetch(src, w + 1ull, hi);
    }
    PRF_CS_FN void seek(S &src, u64 q) {            // q >> 6 is w or w + 1
        if ((q >> 6) == w) return;
        ++w;
#pragma unroll
        for (int p = 0; p < 3; p++) lo[p] = hi[p];
        fetch(src, w + 1ull, hi);
    }
    PRF_CS_FN u32 base(u64 q, u32 lane) const {
        const u32 s = (u32)(q & 63ull);
        return cs_base(cs_fsr(lo[0], hi[0], s), cs_fsr(lo[1], hi[1], s), cs_fsr(lo[2], hi[2], s), lane);
    }
};

// What lane `lane` of the wave does with an item: add(column, base) for every position of the item that is the lane's and is
// A, C, G or T.  Every value that steers the loop is the same in all lanes (the source may shuffle).  For k <= PRF_CS_REG_K the
// lane's column is the same at every call (cs_lane_column); for larger k the 64 lanes of a step call with 64 different columns.
template <class S, class F>
PRF_CS_FN void cs_count_item(S &src, u64 g_begin, const cs_row &r, const cs_item &it, u32 lane, F &&add) {
    const u32 step = cs_step(r.k);
    u32 col = (u32)((it.first - r.start + lane) % r.k);
    cs_window<S> win;
    win.open(src, g_begin + it.first, g_begin + it.end - 1ull);
#pragma unroll 1
    for (u64 cur = it.first; cur < it.end; cur += step) {
        const u64 q = g_begin + cur;
        win.seek(src, q);
        const u32 b = win.base(q, lane);
        if (lane < step && cur + lane < it.end && b < 4u) add(col, b);
        if (r.k > PRF_CS_REG_K) {                   // 64 positions on: k > 64, so once around at most
            col += 64u;
            if (col >= r.k) col -= r.k;
        }
    }
}

// the column of a lane of an item of k <= PRF_CS_REG_K (lanes at and behind cs_step(k) have none and count nothing)
PRF_CS_FN u32 cs_lane_column(const cs_row &r, const cs_item &it, u32 lane) { return (u32)((it.first - r.start + lane) % r.k); }

// the letter and the count of a column's consensus: the largest count, ties to the first of A, C, G, T; 'N' if there is none
PRF_CS_FN char cs_consensus(const u32 *count, u32 *best) {
    u32 at = 0;
#pragma unroll
    for (u32 b = 1; b < 4; b++)
        if (count[b] > count[at]) at = b;
    *best = count[at];
    return count[at] ? "ACGT"[at] : 'N';
}

}  // namespace
