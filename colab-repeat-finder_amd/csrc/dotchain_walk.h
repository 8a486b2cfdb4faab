// dotchain_walk.h -- the two walks of dotchain.hip along one line of the dot plot, over a source of 64-cell words of
// raw cells: the head test (backwards from a seed) and the follow (forwards from its end).  They form no address and know nothing
// of the planes, so the same text runs in the kernels and, compiled for the host, against a brute force
// (tests/dotchain_walk_check.cpp).  Cells of a line are numbered t = 0, 1, ... from the cell with the smallest row.
#pragma once
#ifdef __HIPCC__
#include "prf_device.h"
#define PRF_WALK_FN __host__ __device__ __forceinline__
#else
#include <stdint.h>
typedef uint32_t u32;
typedef unsigned long long u64;
#define PRF_WALK_FN inline
#endif

namespace {

// No seed ends in [t0 - 1 - max_gap, t0 - 2].  p: the cells below p are still to be looked at; in a run, e is its last cell and
// cells p .. e are raw.
// word(k): bit b = cell 64 k + b of the line is raw.
template <class F>
PRF_WALK_FN bool dc_is_head(u64 t0, u64 min_seed, u32 max_gap, F &&word) {
    if (t0 < 2) return true;
    const u64 lo = t0 - 1 > max_gap ? t0 - 1 - max_gap : 0;
    u64 p = t0 - 1, e = 0;
    bool in_run = false;
#pragma unroll 1
    for (;;) {
        if (in_run) {
            if (e - p + 1 >= min_seed) return false;
            if (!p) return true;                        // the run begins with the line and is too short
        } else if (p <= lo) {
            return true;
        }
        const u64 k = (p - 1) >> 6;
        const u64 w = word(k);
        const u32 n = (u32)(p - 64ull * k);             // 1 .. 64 bits of this word lie below p
        const u64 m = (in_run ? ~w : w) & (n == 64 ? ~0ull : (1ull << n) - 1ull);
        if (!m) {
            p = 64ull * k;
            continue;
        }
        const u64 at = 64ull * k + 63ull - (u64)__builtin_clzll(m);
        if (in_run) {                                   // a mismatch: the run is at + 1 .. e
            if (e - at >= min_seed) return false;
            in_run = false;
        } else {                                        // the last cell of a run
            if (at < lo) return true;
            e = at;
            in_run = true;
        }
        p = at;
    }
}

struct dc_state {
    u64 end;                // the last committed seed's last cell
    u64 matches, pending;   // raw cells up to `end`; raw cells of the runs shorter than min_seed behind it
    u64 p;                  // the next cell to look at
    u64 run_start;          // in_run: the first cell of the run that holds cell p - 1
    u32 seeds;
    bool in_run;
};

// the state behind a chain's first seed, cells t0 .. t0 + len - 1: cell t0 + len is a mismatch or the line's end
PRF_WALK_FN dc_state dc_first_seed(u64 t0, u64 len) { return dc_state{t0 + len - 1ull, len, 0ull, t0 + len + 1ull, 0ull, 1u, false}; }

// Walks forward until the chain is complete (true) or the cursor has reached `stop` (false: the state says where to go on).
// word(k) as above; cells behind the line's end are not raw.
template <class F>
PRF_WALK_FN bool dc_follow(dc_state &s, u64 min_seed, u32 max_gap, u64 stop, F &&word) {
#pragma unroll 1
    for (;;) {
        if (!s.in_run && s.p > s.end + max_gap + 1ull) return true;          // a run from here on starts too far behind the end
        if (s.p >= stop) return false;
        const u64 k = s.p >> 6;
        const u64 w = word(k);
        const u64 m = (s.in_run ? ~w : w) & (~0ull << (s.p & 63));
        if (!m) {
            s.p = 64ull * (k + 1ull);
            continue;
        }
        const u64 at = 64ull * k + (u64)__builtin_ctzll(m);
        if (s.in_run) {                                                        // a mismatch (or the line's end): the run is run_start .. at - 1
            const u64 n = at - s.run_start;
            if (n >= min_seed) {
                s.matches += s.pending + n;
                s.pending = 0;
                s.end = at - 1ull;
                s.seeds++;
            } else {
                s.pending += n;
            }
            s.in_run = false;
        } else {
            if (at > s.end + max_gap + 1ull) return true;
            s.run_start = at;
            s.in_run = true;
        }
        s.p = at + 1ull;
    }
}

}  // namespace
