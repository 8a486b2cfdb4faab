// periodchain_stage.h -- the stage of the list products of the period lines of a range (periodchain_host.cpp, DESIGN 16;
// periodlink_host.cpp; nobody else includes it): the window of a request and its refusals, the clipped range, the
// arguments of the kernels of periodchain.hip, and the stage that runs them and leaves the rows on the device:
//   1. the find kernel over the words of the window, cut into launches of at most launch_cells cells: rows, or entries of the
//      long list;
//   2. the long kernel for the first runs and chains the find kernel left, one wave each.
#pragma once
#include "list_host.h"

namespace {

struct pchain_room {
    u64 n;              // positions of the clipped range
    u64 pos0, pos1;     // the clipped window
};

// The window of a request of one range, start positions x a range of k, and what the frame of list_host.h asks of it
struct period_window {
    static constexpr bool pair = false;
    using room = pchain_room;
    u64 begin, end;
    u64 pos0, pos1;
    u32 kmin, kmax, n_matches;

    int check_window(const char *name) const {
        if (begin > end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (pos0 > pos1) return fail(PRF_EINVAL, "%s: pos0 %llu is behind pos1 %llu", name, (unsigned long long)pos0, (unsigned long long)pos1);
        if (!kmin) return fail(PRF_EINVAL, "%s: kmin is 0. It must be at least 1.", name);
        if (kmin > kmax) return fail(PRF_EINVAL, "%s: kmin %u is above kmax %u", name, kmin, kmax);
        if (n_matches > 1) return fail(PRF_EINVAL, "%s: n_matches is %u. It must be 0 (N never matches) or 1 (N == N matches).", name, n_matches);
        return PRF_OK;
    }

    int check_room(const char *name, u64 seq_len, room *o) const {
        const int rc = matrix_clip(name, begin, end, seq_len, &o->n);
        if (rc) return rc;
        o->pos1 = pos1 < o->n ? pos1 : o->n;
        o->pos0 = pos0 < o->pos1 ? pos0 : o->pos1;
        const u64 starts = o->pos1 - o->pos0, nk = (u64)kmax - kmin + 1;
        if (starts && nk > PRF_DOT_MAX_CELLS / starts)
            return fail(PRF_EUNSUPPORTED, "%s: a window of %llu positions x %llu lines is above the limit of 2^42 cells per call (PRF_DOT_MAX_CELLS)",
                        name, (unsigned long long)starts, (unsigned long long)nk);
        return PRF_OK;
    }

    // a window with starts and lines: a line k >= n is empty
    bool any(const room &o) const { return o.pos1 > o.pos0 && (u64)kmin < o.n; }
    u64 positions(const room &o) const { return o.n; }

    template <class Row>
    static bool less(const Row &x, const Row &y) {
        return x.start != y.start ? x.start < y.start : x.k < y.k;
    }
};

// the kernels' arguments for a window that is not empty; dst, capacity, longs and counters are the stage's
prf_periodchain_args pchain_args(const prf_contig_view &v, const pchain_room &o, const period_window &w, u64 min_seed, u32 max_gap,
                                 u64 min_len) {
    prf_periodchain_args a{};
    a.pl = v.planes;
    a.g_begin = v.base + w.begin;
    a.n = o.n;
    a.n_words = (o.n + 63) / 64;
    a.pos0 = o.pos0;
    a.pos1 = o.pos1;
    a.kmin = w.kmin;
    a.kmax = (u64)w.kmax < o.n ? w.kmax : (u32)(o.n - 1);
    a.n_matches = w.n_matches;
    a.max_gap = max_gap;
    a.min_seed = min_seed;
    a.min_len = min_len;
    const u64 nk = (u64)a.kmax - a.kmin + 1, starts = o.pos1 - o.pos0;
    // two heads of one line lie more than PRF_DOTCHAIN_FOLLOW cells apart if the first one is still going there
    const u64 most_long = nk * (starts / PRF_DOTCHAIN_FOLLOW + 2);
    a.long_cap = most_long < PRF_PCHAIN_LONG_ROWS ? most_long : PRF_PCHAIN_LONG_ROWS;
    return a;
}

// The chains of the window into d_out (room for `cap` rows), which stay on the device: cnt[PRF_PC_CHAINS] is their number, and
// they were all written only if it is at most cap.  *ms (the find kernel's), *ms_long and *launches are added to.
int pchain_rows(const char *name, prf_ctx *c, prf_periodchain_args a, u64 launch_cells, u64 cap, dev_array<prf_pchain_dev> &d_out,
                dev_array<prf_pchain_long> &d_long, dev_array<u64> &d_cnt, u64 *cnt, float *ms, float *ms_long, u32 *launches) {
    int rc;
    a.capacity = cap;
    if ((rc = d_out.alloc(a.capacity)) || (rc = d_long.alloc(a.long_cap)) || (rc = d_cnt.alloc(PRF_PC_N))) return rc;
    a.dst = d_out.p;
    a.longs = d_long.p;
    a.counters = d_cnt.p;
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, PRF_PC_N * sizeof(u64), c->stream));
    // ---- 1. the words of the window, whole spans per launch
    const u64 nk = (u64)a.kmax - a.kmin + 1;
    u32 span_words, kslice, stride;
    prf_periodchain_shape(a.pl.E[0] != nullptr, &span_words, &kslice, &stride);
    const u64 cells = launch_cells ? launch_cells : PRF_DOT_LAUNCH_CELLS;
    u64 spans = cells / nk / 64 / span_words;
    if (spans < 1) spans = 1;
    if (spans > (1ull << 30)) spans = 1ull << 30;
    const u64 w_end = (a.pos1 + 63) / 64;
    rc = timed_step(c, [&]() -> int {
        for (u64 w = a.pos0 / 64; w < w_end; w += spans * span_words) {
            a.word0 = w;
            a.word1 = w_end - w > spans * span_words ? w + spans * span_words : w_end;
            HIPCHK(prf_launch_periodchain_find(c->stream, a));
            ++*launches;
        }
        return PRF_OK;
    }, cnt, d_cnt.p, PRF_PC_N, ms);
    if (rc) return rc;
    if (cnt[PRF_PC_LONG] > a.long_cap)
        return fail(PRF_EUNSUPPORTED, "%s: %llu runs and chains are still going %u cells (PRF_DOTCHAIN_FOLLOW) behind their start, the call keeps room for %llu: ask for a smaller window",
                    name, (unsigned long long)cnt[PRF_PC_LONG], PRF_DOTCHAIN_FOLLOW, (unsigned long long)a.long_cap);
    // ---- 2. what the find kernel left
    if (cnt[PRF_PC_LONG])
        return timed_step(c, [&]() -> int {
            HIPCHK(prf_launch_periodchain_long(c->stream, a, cnt[PRF_PC_LONG]));
            ++*launches;
            return PRF_OK;
        }, cnt, d_cnt.p, PRF_PC_N, ms_long);
    return PRF_OK;
}

}  // namespace
