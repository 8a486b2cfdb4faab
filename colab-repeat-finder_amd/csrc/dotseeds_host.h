// dotseeds_host.h -- what the two host paths that work on the SEEDS of a window share (dotchain_host.cpp, DESIGN 14;
// dotlink_host.cpp; nobody else includes it): the clipped rectangle and window, the arguments of the seed kernels of
// dotruns.hip at min_len = min_seed, and the seeds themselves, left on the device.  Moved here unchanged from dotchain_host.cpp.
#pragma once
#include "matrix_host.h"

namespace {

constexpr u64 first_seed_rows = 1ull << 20;

struct seeds_room {
    u64 b_base, b_len;
    u64 na, nb;
    u64 row0, row1, col0, col1;      // the clipped window
};

// o->b_len is set: from B's contig view, or by the one-shot form from its second sequence
int seeds_check_room(const char *name, u64 begin, u64 end, u64 b_begin, u64 b_end, u64 row0, u64 row1, u64 col0, u64 col1, u64 a_len,
                     seeds_room *o) {
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

// entries of the seed kernels' long list: runs_request::long_rows of dotruns_host.cpp
u64 seeds_long_rows(const seeds_room &o, u32 directions) {
    const u64 window = (o.row1 - o.row0) * (o.col1 - o.col0);                        // <= 2^42
    const unsigned __int128 fit = (unsigned __int128)o.na * o.nb / PRF_DOTRUN_FOLLOW;   // na, nb < 2^40
    const u64 per_direction = fit < window ? (u64)fit : window;
    const u64 n = (directions == 3 ? 2 : 1) * per_direction;
    return n < PRF_DOTRUN_LONG_ROWS ? n : PRF_DOTRUN_LONG_ROWS;
}

// the seed kernels' arguments for a window that is not empty
prf_dotruns_args seeds_args(const prf_contig_view &v, const seeds_room &o, u64 begin, u64 b_begin, u32 strand, u32 directions, u64 min_seed) {
    prf_dotruns_args a{};
    a.pl = v.planes;
    a.a_g_begin = v.base + begin;
    a.na = o.na;
    a.b_g_begin = o.b_base + b_begin;
    a.nb = o.nb;
    a.col0 = o.col0;
    a.col1 = o.col1;
    a.words_per_row = (o.col1 - o.col0 + 63) / 64;
    a.min_len = min_seed;
    a.strand = strand;
    a.directions = directions;
    a.p = min_seed < PRF_DOTRUN_PROBE ? (u32)min_seed : PRF_DOTRUN_PROBE;
    a.long_cap = seeds_long_rows(o, directions);
    return a;
}

// The seeds of the window into d_seeds (room for `cap` rows): *found is the number of seeds, which were all written only if it
// is at most cap.  *ms and *launches are added to.
int find_seeds(const char *name, prf_ctx *c, prf_dotruns_args a, u64 launch_cells, const seeds_room &o, u64 cap,
               dev_array<prf_dotrun_dev> &d_seeds, dev_array<prf_dotrun_dev> &d_long, u64 *d_cnt, u64 *found, float *ms, u32 *launches) {
    int rc = d_seeds.alloc(cap);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d_cnt, 0, PRF_DR_N * sizeof(u64), c->stream));
    a.dst = d_seeds.p;
    a.capacity = cap;
    a.longs = d_long.p;
    a.counters = d_cnt;
    // rows per launch, as runs_run (dotruns_host.cpp) cuts them
    const u64 cols = o.col1 - o.col0;
    const u64 tile_rows = 64, span_words = 62;
    const u64 cells = launch_cells ? launch_cells : PRF_DOT_LAUNCH_CELLS / ((a.p + 3) / 4);
    const u64 n_spans = (a.words_per_row + span_words - 1) / span_words;
    u64 tiles = cells / cols / tile_rows;
    if (tiles > (1ull << 30) / n_spans) tiles = (1ull << 30) / n_spans;
    if (tiles < 1) tiles = 1;
    float part = 0;
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    for (u64 lr = o.row0; lr < o.row1; lr += tiles * tile_rows) {
        a.lrow0 = lr;
        a.lrow1 = o.row1 - lr > tiles * tile_rows ? lr + tiles * tile_rows : o.row1;
        HIPCHK(prf_launch_dotruns_find(c->stream, a));
        ++*launches;
    }
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    u64 cnt[PRF_DR_N] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&part, c->ev[0], c->ev[1]));
    *ms += part;
    if (cnt[PRF_DR_LONG] > a.long_cap)
        return fail(PRF_EUNSUPPORTED, "%s: %llu runs longer than %u cells (PRF_DOTRUN_FOLLOW) start in the window, the call keeps room for %llu: ask for smaller windows",
                    name, (unsigned long long)cnt[PRF_DR_LONG], PRF_DOTRUN_FOLLOW, (unsigned long long)a.long_cap);
    if (cnt[PRF_DR_LONG]) {
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        HIPCHK(prf_launch_dotruns_long(c->stream, a, cnt[PRF_DR_LONG]));
        ++*launches;
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&part, c->ev[0], c->ev[1]));
        *ms += part;
    }
    *found = cnt[PRF_DR_RUNS];
    return PRF_OK;
}

// Every seed of the window, on the device: at most one per cell of the window and direction; 2^20 rows at first, the exact number
// (up to PRF_DOTCHAIN_MAX_ROWS) if there were more.
int all_seeds(const char *name, prf_ctx *c, const prf_dotruns_args &a, u64 launch_cells, const seeds_room &o,
              dev_array<prf_dotrun_dev> &d_seeds, dev_array<prf_dotrun_dev> &d_long, u64 *d_cnt, u64 *n_seeds, float *ms, u32 *launches) {
    const u64 most = (a.directions == 3 ? 2 : 1) * (o.row1 - o.row0) * (o.col1 - o.col0);
    u64 cap = most < first_seed_rows ? most : first_seed_rows;
    int rc = find_seeds(name, c, a, launch_cells, o, cap, d_seeds, d_long, d_cnt, n_seeds, ms, launches);
    if (rc) return rc;
    if (*n_seeds > cap) {
        if (*n_seeds > PRF_DOTCHAIN_MAX_ROWS)
            return fail(PRF_EUNSUPPORTED, "%s: %llu seeds start in the window, a call links at most %llu (PRF_DOTCHAIN_MAX_ROWS): ask for smaller windows or a larger min_seed",
                        name, (unsigned long long)*n_seeds, (unsigned long long)PRF_DOTCHAIN_MAX_ROWS);
        cap = *n_seeds;
        if ((rc = find_seeds(name, c, a, launch_cells, o, cap, d_seeds, d_long, d_cnt, n_seeds, ms, launches))) return rc;
        if (*n_seeds != cap) return fail(PRF_EHIP, "%s: the second pass found %llu seeds, the first %llu", name, (unsigned long long)*n_seeds, (unsigned long long)cap);
    }
    return PRF_OK;
}

}  // namespace
