// dotruns_host.cpp -- the host path of the list of diagonal runs of the dot plot of two ranges (prf_dotpair_runs, its _ex and
// one-shot forms; kernels: dotruns.hip).  It uses the helpers of matrix_host.h and judges its arguments in the order of
// dotpair_host.cpp, but runs its own output: a list with a count does not fit matrix_run's words-or-counts.  One call = one window
// of start cells of the na x nb rectangle: the window's rows are cut into launches of the find kernel as dotpair_host.cpp cuts
// them, the two counters are read, the long kernel finishes the runs the find kernel left, the rows are copied and sorted here.
// Like the other matrix products it reads no selection, writes no row sink and leaves the last scan's rows alone.
#include <algorithm>
#include <vector>

#include "matrix_host.h"

namespace {

struct runs_request {
    static constexpr u32 path = 7;
    u64 begin, end;     // A's range
    u32 b_contig;
    u64 b_begin, b_end;
    u32 strand;
    u64 row0, row1, col0, col1;
    u32 directions;
    u64 min_len;
    prf_dotrun *dst;
    u64 capacity;
    uint64_t *n_runs;
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS
    struct room {
        u64 b_base, b_len;
        u64 na, nb;
        u64 row0, row1, col0, col1;      // the clipped window
    };

    int check(const char *name) const {
        if (begin > end) return fail(PRF_EINVAL, "%s: a_begin %llu is behind a_end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (b_begin > b_end)
            return fail(PRF_EINVAL, "%s: b_begin %llu is behind b_end %llu", name, (unsigned long long)b_begin, (unsigned long long)b_end);
        if (row0 > row1) return fail(PRF_EINVAL, "%s: row0 %llu is behind row1 %llu", name, (unsigned long long)row0, (unsigned long long)row1);
        if (col0 > col1) return fail(PRF_EINVAL, "%s: col0 %llu is behind col1 %llu", name, (unsigned long long)col0, (unsigned long long)col1);
        if (strand > 1) return fail(PRF_EINVAL, "%s: strand is %u. It must be 0 (plus) or 1 (minus).", name, strand);
        if (!directions || directions > 3)
            return fail(PRF_EINVAL, "%s: directions is %u. It must be 1 (main), 2 (anti) or 3 (both).", name, directions);
        if (!min_len) return fail(PRF_EINVAL, "%s: min_len is 0. It must be at least 1.", name);
        if (capacity > PRF_DOTRUN_MAX_ROWS)
            return fail(PRF_EUNSUPPORTED, "%s: a capacity of %llu rows is above %llu (PRF_DOTRUN_MAX_ROWS)", name,
                        (unsigned long long)capacity, (unsigned long long)PRF_DOTRUN_MAX_ROWS);
        if (!n_runs) return fail(PRF_EINVAL, "%s: NULL n_runs", name);
        if (!dst && capacity) return fail(PRF_EINVAL, "%s: NULL destination with a capacity of %llu rows", name, (unsigned long long)capacity);
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

    // Entries of the long list.  Long runs of one direction are disjoint and each holds at least PRF_DOTRUN_FOLLOW cells of the
    // rectangle, and each starts in its own cell of the window: at most directions x min(na nb / FOLLOW, cells of the window) of
    // them exist, of which the call keeps room for PRF_DOTRUN_LONG_ROWS.
    u64 long_rows(const room &o) const {
        const u64 window = (o.row1 - o.row0) * (o.col1 - o.col0);                        // <= 2^42
        const unsigned __int128 fit = (unsigned __int128)o.na * o.nb / PRF_DOTRUN_FOLLOW;   // na, nb < 2^40
        const u64 per_direction = fit < window ? (u64)fit : window;
        const u64 n = (directions == 3 ? 2 : 1) * per_direction;
        return n < PRF_DOTRUN_LONG_ROWS ? n : PRF_DOTRUN_LONG_ROWS;
    }
};

int runs_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const runs_request &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v, vb;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = prf_genome_contig_view(g, r.b_contig, &vb))) return rc;
    runs_request::room o{};
    o.b_base = vb.base;
    o.b_len = vb.len;
    if ((rc = r.check_room(name, v.len, &o))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    HIPCHK(hipSetDevice(c->dev));
    float ms = 0;
    u32 launches = 0;
    u64 n_runs = 0;
    const u64 rows = o.row1 - o.row0, cols = o.col1 - o.col0;
    if (rows && cols) {
        const u64 long_cap = r.long_rows(o);
        dev_array<prf_dotrun_dev> d_out, d_long;
        dev_array<u64> d_cnt;
        if ((rc = d_out.alloc(r.capacity)) || (rc = d_long.alloc(long_cap)) || (rc = d_cnt.alloc(PRF_DR_N))) return rc;
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, PRF_DR_N * sizeof(u64), c->stream));
        prf_dotruns_args a{};
        a.pl = v.planes;
        a.a_g_begin = v.base + r.begin;
        a.na = o.na;
        a.b_g_begin = o.b_base + r.b_begin;
        a.nb = o.nb;
        a.col0 = o.col0;
        a.col1 = o.col1;
        a.words_per_row = (cols + 63) / 64;
        a.min_len = r.min_len;
        a.strand = r.strand;
        a.directions = r.directions;
        a.p = r.min_len < PRF_DOTRUN_PROBE ? (u32)r.min_len : PRF_DOTRUN_PROBE;
        a.dst = d_out.p;
        a.capacity = r.capacity;
        a.longs = d_long.p;
        a.long_cap = long_cap;
        a.counters = d_cnt.p;
        // rows per launch, as pair_request::launch (dotpair_host.cpp) cuts them: whole tiles, at most launch_cells cells and 2^30
        // workgroups, at least one tile; the default shrinks with the probe's looks per word
        const u64 tile_rows = 64, span_words = 62;
        const u64 cells = r.launch_cells ? r.launch_cells : PRF_DOT_LAUNCH_CELLS / ((a.p + 3) / 4);
        const u64 n_spans = (a.words_per_row + span_words - 1) / span_words;
        u64 tiles = cells / cols / tile_rows;
        if (tiles > (1ull << 30) / n_spans) tiles = (1ull << 30) / n_spans;
        if (tiles < 1) tiles = 1;
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        for (u64 lr = o.row0; lr < o.row1; lr += tiles * tile_rows) {
            a.lrow0 = lr;
            a.lrow1 = o.row1 - lr > tiles * tile_rows ? lr + tiles * tile_rows : o.row1;
            HIPCHK(prf_launch_dotruns_find(c->stream, a));
            ++launches;
        }
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        u64 cnt[PRF_DR_N] = {0, 0};
        HIPCHK(hipMemcpyAsync(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        if (cnt[PRF_DR_LONG] > long_cap)
            return fail(PRF_EUNSUPPORTED, "%s: %llu runs longer than %u cells (PRF_DOTRUN_FOLLOW) start in the window, the call keeps room for %llu: ask for smaller windows",
                        name, (unsigned long long)cnt[PRF_DR_LONG], PRF_DOTRUN_FOLLOW, (unsigned long long)long_cap);
        if (cnt[PRF_DR_LONG]) {
            float ms_long = 0;
            HIPCHK(hipEventRecord(c->ev[2], c->stream));
            HIPCHK(prf_launch_dotruns_long(c->stream, a, cnt[PRF_DR_LONG]));
            ++launches;
            HIPCHK(hipEventRecord(c->ev[3], c->stream));
            HIPCHK(hipMemcpyAsync(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipEventElapsedTime(&ms_long, c->ev[2], c->ev[3]));
            ms += ms_long;
        }
        n_runs = cnt[PRF_DR_RUNS];
        if (n_runs && n_runs <= r.capacity) {
            std::vector<prf_dotrun> got(n_runs);
            static_assert(sizeof(prf_dotrun) == sizeof(prf_dotrun_dev), "one layout");
            HIPCHK(hipMemcpy(got.data(), d_out.p, n_runs * sizeof(prf_dotrun), hipMemcpyDeviceToHost));
            std::sort(got.begin(), got.end(), [](const prf_dotrun &x, const prf_dotrun &y) {
                return x.row != y.row ? x.row < y.row : x.col != y.col ? x.col < y.col : x.dir < y.dir;
            });
            memcpy(r.dst, got.data(), n_runs * sizeof(prf_dotrun));
        }
    }
    *r.n_runs = n_runs;
    lane_stats(stats, runs_request::path, ms, o.na + o.nb, (o.na + o.nb + 3) / 4, launches);
    if (stats) stats->n_hits = n_runs;
    return PRF_OK;
}

int runs_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const runs_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = r.check(name);
        return rc ? rc : runs_run(name, c, g, contig, r, stats);
    });
}

// two sequences become contigs 0 (A) and 1 (B) of a genome that lives for the call, as pair_one_shot (dotpair_host.cpp) loads
// them.  Everything that can be refused from the arguments and the bytes is refused before the context is looked at.
int runs_one_shot(const char *name, prf_ctx *c, const prf_contig *seq_a, const prf_contig *seq_b, const runs_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        for (const prf_contig *seq : {seq_a, seq_b})
            if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        runs_request::room o{};
        o.b_len = seq_b->len;
        if ((rc = r.check_room(name, seq_a->len, &o))) return rc;
        if ((rc = matrix_check_letters(name, seq_a)) || (rc = matrix_check_letters(name, seq_b))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        const prf_contig both[2] = {*seq_a, *seq_b};
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, both, 2, 64, &g))) return rc;
        rc = runs_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_dotpair_runs_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                        uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                        uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                        prf_scan_stats *stats, uint64_t launch_cells) {
    return runs_on_genome("prf_dotpair_runs", c, g, a_contig,
                          runs_request{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions, min_len, dst,
                                       capacity, n_runs, launch_cells},
                          stats);
}

int prf_dotpair_runs(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                     uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                     uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                     prf_scan_stats *stats) {
    return prf_dotpair_runs_ex(c, g, a_contig, a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions,
                               min_len, dst, capacity, n_runs, stats, 0);
}

int prf_dotpair_runs_seq(prf_ctx *c, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b, uint64_t b_begin,
                         uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                         uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                         prf_scan_stats *stats) {
    return runs_one_shot("prf_dotpair_runs_seq", c, seq_a, seq_b,
                         runs_request{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, directions, min_len, dst,
                                      capacity, n_runs, 0},
                         stats);
}

}  // extern "C"
