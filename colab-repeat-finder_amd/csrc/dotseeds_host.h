// dotseeds_host.h -- the stage of the list products of the dot plot of two ranges (dotruns_host.cpp; dotchain_host.cpp,
// DESIGN 14; dotlink_host.cpp; nobody else includes it): the window of a request and its refusals, the clipped
// rectangle, the arguments of the seed kernels of dotruns.hip, and the seeds themselves, left on the device.  A run of
// prf_dotpair_runs is a seed at min_len; the chains and the links start from the seeds at min_seed.
#pragma once
#include "list_host.h"

namespace {

constexpr u64 first_seed_rows = 1ull << 20;

struct seeds_room {
    u64 b_base, b_len;
    u64 na, nb;
    u64 row0, row1, col0, col1;      // the clipped window
};

// The window of a request of two ranges, and what the frame of list_host.h asks of it
struct pair_window {
    static constexpr bool pair = true;
    using room = seeds_room;
    u64 begin, end;     // A's range
    u32 b_contig;
    u64 b_begin, b_end;
    u32 strand;
    u64 row0, row1, col0, col1;
    u32 directions;

    int check_window(const char *name) const {
        if (begin > end) return fail(PRF_EINVAL, "%s: a_begin %llu is behind a_end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (b_begin > b_end)
            return fail(PRF_EINVAL, "%s: b_begin %llu is behind b_end %llu", name, (unsigned long long)b_begin, (unsigned long long)b_end);
        if (row0 > row1) return fail(PRF_EINVAL, "%s: row0 %llu is behind row1 %llu", name, (unsigned long long)row0, (unsigned long long)row1);
        if (col0 > col1) return fail(PRF_EINVAL, "%s: col0 %llu is behind col1 %llu", name, (unsigned long long)col0, (unsigned long long)col1);
        if (strand > 1) return fail(PRF_EINVAL, "%s: strand is %u. It must be 0 (plus) or 1 (minus).", name, strand);
        if (!directions || directions > 3)
            return fail(PRF_EINVAL, "%s: directions is %u. It must be 1 (main), 2 (anti) or 3 (both).", name, directions);
        return PRF_OK;
    }

    // o->b_len is set: from B's contig view, or by the one-shot form from its second sequence
    int check_room(const char *name, u64 a_len, room *o) const {
        int rc = matrix_clip(name, begin, end, a_len, &o->na);
        if (!rc) rc = matrix_clip(name, b_begin, b_end, o->b_len, &o->nb);
        if (rc) return rc;
        o->row1 = row1 < o->na ? row1 : o->na;
        o->row0 = row0 < o->row1 ? row0 : o->row1;
        o->col1 = col1 < o->nb ? col1 : o->nb;
        o->col0 = col0 < o->col1 ? col0 : o->col1;
        const u64 rows = o->row1 - o->row0, cols = o->col1 - o->col0;
        if (rows && cols > PRF_DOT_MAX_CELLS / rows)
            return fail(PRF_EUNSUPPORTED, "%s: a window of %llu x %llu cells is above the limit of 2^42 per call (PRF_DOT_MAX_CELLS)", name,
                        (unsigned long long)rows, (unsigned long long)cols);
        return PRF_OK;
    }

    bool any(const room &o) const { return o.row1 > o.row0 && o.col1 > o.col0; }
    u64 positions(const room &o) const { return o.na + o.nb; }

    template <class Row>
    static bool less(const Row &x, const Row &y) {
        return x.row != y.row ? x.row < y.row : x.col != y.col ? x.col < y.col : x.dir < y.dir;
    }
};

// Entries of the seed kernels' long list.  Long runs of one direction are disjoint and each holds at least PRF_DOTRUN_FOLLOW cells
// of the rectangle, and each starts in its own cell of the window: at most directions x min(na nb / FOLLOW, cells of the window)
// of them exist, of which the call keeps room for PRF_DOTRUN_LONG_ROWS.
u64 seeds_long_rows(const seeds_room &o, u32 directions) {
    const u64 window = (o.row1 - o.row0) * (o.col1 - o.col0);                        // <= 2^42
    const unsigned __int128 fit = (unsigned __int128)o.na * o.nb / PRF_DOTRUN_FOLLOW;   // na, nb < 2^40
    const u64 per_direction = fit < window ? (u64)fit : window;
    const u64 n = (directions == 3 ? 2 : 1) * per_direction;
    return n < PRF_DOTRUN_LONG_ROWS ? n : PRF_DOTRUN_LONG_ROWS;
}

// the seed kernels' arguments for a window that is not empty; dst, capacity, longs and counters are find_seeds'
prf_dotruns_args seeds_args(const prf_contig_view &v, const seeds_room &o, const pair_window &w, u64 min_len) {
    prf_dotruns_args a{};
    a.pl = v.planes;
    a.a_g_begin = v.base + w.begin;
    a.na = o.na;
    a.b_g_begin = o.b_base + w.b_begin;
    a.nb = o.nb;
    a.col0 = o.col0;
    a.col1 = o.col1;
    a.words_per_row = (o.col1 - o.col0 + 63) / 64;
    a.min_len = min_len;
    a.strand = w.strand;
    a.directions = w.directions;
    a.p = min_len < PRF_DOTRUN_PROBE ? (u32)min_len : PRF_DOTRUN_PROBE;
    a.long_cap = seeds_long_rows(o, w.directions);
    return a;
}

// The seeds of the window into d_seeds (room for `cap` rows): *found is the number of seeds, which were all written only if it
// is at most cap.  The window's rows are cut into launches of the find kernel as dotpair_host.cpp cuts them, the long kernel
// finishes the runs the find kernel left.  *ms and *launches are added to.
int find_seeds(const char *name, prf_ctx *c, prf_dotruns_args a, u64 launch_cells, const seeds_room &o, u64 cap,
               dev_array<prf_dotrun_dev> &d_seeds, dev_array<prf_dotrun_dev> &d_long, u64 *d_cnt, u64 *found, float *ms, u32 *launches) {
    int rc = d_seeds.alloc(cap);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d_cnt, 0, PRF_DR_N * sizeof(u64), c->stream));
    a.dst = d_seeds.p;
    a.capacity = cap;
    a.longs = d_long.p;
    a.counters = d_cnt;
    // rows per launch: whole tiles, at most launch_cells cells and 2^30 workgroups, at least one tile; the default shrinks with the
    // probe's looks per word
    const u64 cols = o.col1 - o.col0;
    const u64 tile_rows = 64, span_words = 62;
    const u64 cells = launch_cells ? launch_cells : PRF_DOT_LAUNCH_CELLS / ((a.p + 3) / 4);
    const u64 n_spans = (a.words_per_row + span_words - 1) / span_words;
    u64 tiles = cells / cols / tile_rows;
    if (tiles > (1ull << 30) / n_spans) tiles = (1ull << 30) / n_spans;
    if (tiles < 1) tiles = 1;
    u64 cnt[PRF_DR_N] = {0, 0};
    rc = timed_step(c, [&]() -> int {
        for (u64 lr = o.row0; lr < o.row1; lr += tiles * tile_rows) {
            a.lrow0 = lr;
            a.lrow1 = o.row1 - lr > tiles * tile_rows ? lr + tiles * tile_rows : o.row1;
            HIPCHK(prf_launch_dotruns_find(c->stream, a));
            ++*launches;
        }
        return PRF_OK;
    }, cnt, d_cnt, PRF_DR_N, ms);
    if (rc) return rc;
    if (cnt[PRF_DR_LONG] > a.long_cap)
        return fail(PRF_EUNSUPPORTED, "%s: %llu runs longer than %u cells (PRF_DOTRUN_FOLLOW) start in the window, the call keeps room for %llu: ask for smaller windows",
                    name, (unsigned long long)cnt[PRF_DR_LONG], PRF_DOTRUN_FOLLOW, (unsigned long long)a.long_cap);
    if (cnt[PRF_DR_LONG]) {
        rc = timed_step(c, [&]() -> int {
            HIPCHK(prf_launch_dotruns_long(c->stream, a, cnt[PRF_DR_LONG]));
            ++*launches;
            return PRF_OK;
        }, cnt, d_cnt, PRF_DR_N, ms);
        if (rc) return rc;
    }
    *found = cnt[PRF_DR_RUNS];
    return PRF_OK;
}

// Every seed of the window, on the device: at most one per cell of the window and direction; 2^20 rows at first, the exact number
// (up to PRF_DOTCHAIN_MAX_ROWS) if there were more.
int all_seeds(const char *name, prf_ctx *c, const prf_dotruns_args &a, u64 launch_cells, const seeds_room &o,
              dev_array<prf_dotrun_dev> &d_seeds, dev_array<prf_dotrun_dev> &d_long, u64 *d_cnt, u64 *n_seeds, float *ms, u32 *launches) {
    const u64 most = (a.directions == 3 ? 2 : 1) * (o.row1 - o.row0) * (o.col1 - o.col0);
    return grow_once(name, most < first_seed_rows ? most : first_seed_rows, PRF_DOTCHAIN_MAX_ROWS, "PRF_DOTCHAIN_MAX_ROWS", "seeds",
                     "smaller windows or a larger min_seed", [&](u64 cap, u64 *n) {
                         return find_seeds(name, c, a, launch_cells, o, cap, d_seeds, d_long, d_cnt, n, ms, launches);
                     }, n_seeds);
}

}  // namespace
