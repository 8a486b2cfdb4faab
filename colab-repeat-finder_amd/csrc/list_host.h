// list_host.h -- the host path that the list products share (dotruns_host.cpp, dotchain_host.cpp, dotlink_host.cpp,
// periodchain_host.cpp, periodlink_host.cpp, through the two stages dotseeds_host.h and periodchain_stage.h; nobody else includes
// it): the counterpart of matrix_host.h for an output that is a sorted list of rows with a count.
//
// One call = one window of one range (or of the rectangle of two ranges) of a resident genome: judge the arguments (before the
// context or the genome is looked at), take the contig's planes, clip the window, run the product's kernels, which leave the rows
// on the device, copy and sort them here, hand them over if the caller has room for all of them, publish the count and the stats.
// Like the matrix products a list product reads no selection, writes no row sink and leaves the last scan's rows alone.  The order
// of the refusals is part of the interface (the test_refusals_in_the_documented_order tables of the five products' CPU tests).
//
// A product is its request R:
//   static constexpr u32 path                      prf_scan_stats.path
//   static constexpr bool pair                     two ranges: u32 b_contig names B's contig, the room has b_base and b_len
//   using room                                     the clipped window (pair_window of dotseeds_host.h, period_window of periodchain_stage.h)
//   using row, dev_row;  row *dst;  u64 capacity;  uint64_t *n_out
//                                                  the public row and the kernels' row, one layout; the caller's room and count
//                                                  (list_output)
//   static bool less(const row &, const row &)     the order of the list
//   int check(name) const                          what can be said without a genome
//   int check_room(name, a_len, room *) const      what needs the length of the sequence (and, of a pair, o->b_len)
//   bool any(room) const                           the window holds a cell
//   u64 positions(room) const                      the stats' positions
//   int body(name, c, view, room, dev_array<dev_row> &, list_result &) const
//                                                  the kernels of a window that holds a cell: the rows, on the device, and the result
#pragma once
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "matrix_host.h"

// what a body reports: the stats' n_hits (and the caller's count), n_candidates, phase1_ms, phase2_ms and n_launches
struct list_result {
    u64 n = 0, n_candidates = 0;
    float ms1 = 0, ms2 = 0;
    u32 launches = 0;
};

// The output of a request: the rows the caller has room for, the count, and the cells per launch of the _ex forms
template <class Row, class DevRow>
struct list_output {
    using row = Row;
    using dev_row = DevRow;
    Row *dst;
    u64 capacity;
    uint64_t *n_out;
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS
};

// One timed step of a body: `launch` (which counts its launches) between ev[0] and ev[1], then the `n` counter words at d_cnt to
// cnt, once the stream is done.  *ms is added to.
template <class F>
static int timed_step(prf_ctx *c, F &&launch, u64 *cnt, const u64 *d_cnt, u32 n, float *ms) {
    float part = 0;
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    const int rc = launch();
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&part, c->ev[0], c->ev[1]));
    *ms += part;
    return PRF_OK;
}

// Rows whose number is not known before they are written: `pass(cap, &n)` writes them into room for cap rows and counts them.
// `first` rows of room at first, the exact number (up to `limit`, whose name is limit_name) if there were more.
template <class F>
static int grow_once(const char *name, u64 first, u64 limit, const char *limit_name, const char *noun, const char *advice, F &&pass, u64 *n) {
    int rc = pass(first, n);
    if (rc || *n <= first) return rc;
    if (*n > limit)
        return fail(PRF_EUNSUPPORTED, "%s: %llu %s start in the window, a call links at most %llu (%s): ask for %s", name,
                    (unsigned long long)*n, noun, (unsigned long long)limit, limit_name, advice);
    const u64 cap = *n;
    if ((rc = pass(cap, n))) return rc;
    if (*n != cap)
        return fail(PRF_EHIP, "%s: the second pass found %llu %s, the first %llu", name, (unsigned long long)*n, noun, (unsigned long long)cap);
    return PRF_OK;
}

// ---- the refusals that products share; each request calls them in its documented order
static int list_check_seed_gap(const char *name, u64 min_seed, u32 max_gap) {
    if (!min_seed) return fail(PRF_EINVAL, "%s: min_seed is 0. It must be at least 1.", name);
    if (max_gap > PRF_DOTCHAIN_MAX_GAP)
        return fail(PRF_EUNSUPPORTED, "%s: a max_gap of %u cells is above %u (PRF_DOTCHAIN_MAX_GAP)", name, max_gap, PRF_DOTCHAIN_MAX_GAP);
    return PRF_OK;
}

static int list_check_shift(const char *name, u32 max_shift) {
    if (!max_shift) return fail(PRF_EINVAL, "%s: max_shift is 0. It must be at least 1: chains of one line are joined by max_gap.", name);
    if (max_shift > PRF_DOTLINK_MAX_SHIFT)
        return fail(PRF_EUNSUPPORTED, "%s: a max_shift of %u lines is above %u (PRF_DOTLINK_MAX_SHIFT)", name, max_shift, PRF_DOTLINK_MAX_SHIFT);
    return PRF_OK;
}

// the caller's room: `limit` is the product's row limit, n_name what the header calls the count
static int list_check_output(const char *name, const void *dst, u64 capacity, const void *n_out, const char *n_name, u64 limit,
                             const char *limit_name) {
    if (capacity > limit)
        return fail(PRF_EUNSUPPORTED, "%s: a capacity of %llu rows is above %llu (%s)", name, (unsigned long long)capacity,
                    (unsigned long long)limit, limit_name);
    if (!n_out) return fail(PRF_EINVAL, "%s: NULL %s", name, n_name);
    if (!dst && capacity) return fail(PRF_EINVAL, "%s: NULL destination with a capacity of %llu rows", name, (unsigned long long)capacity);
    return PRF_OK;
}

// The n rows at d_rows, sorted, to dst: only if the caller has room for all of them.
template <class R>
static int list_fetch_sorted(const R &r, const typename R::dev_row *d_rows, u64 n) {
    using row = typename R::row;
    static_assert(sizeof(row) == sizeof(typename R::dev_row), "one layout");
    if (!n || n > r.capacity) return PRF_OK;
    std::vector<row> got(n);
    HIPCHK(hipMemcpy(got.data(), d_rows, n * sizeof(row), hipMemcpyDeviceToHost));
    std::sort(got.begin(), got.end(), [](const row &x, const row &y) { return R::less(x, y); });
    memcpy(r.dst, got.data(), n * sizeof(row));
    return PRF_OK;
}

template <class R>
static int list_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const R &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    typename R::room o{};
    if constexpr (R::pair) {
        prf_contig_view vb;
        if ((rc = prf_genome_contig_view(g, r.b_contig, &vb))) return rc;
        o.b_base = vb.base;
        o.b_len = vb.len;
    }
    if ((rc = r.check_room(name, v.len, &o))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    HIPCHK(hipSetDevice(c->dev));
    list_result res;
    if (r.any(o)) {
        dev_array<typename R::dev_row> d_out;
        if ((rc = r.body(name, c, v, o, d_out, res))) return rc;
        if ((rc = list_fetch_sorted(r, d_out.p, res.n))) return rc;
    }
    *r.n_out = res.n;
    const u64 positions = r.positions(o);
    lane_stats(stats, R::path, res.ms1 + res.ms2, positions, (positions + 3) / 4, res.launches);
    if (stats) {
        stats->n_hits = res.n;
        stats->n_candidates = res.n_candidates;
        stats->phase1_ms = res.ms1;
        stats->phase2_ms = res.ms2;
    }
    return PRF_OK;
}

template <class R>
static int list_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const R &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = r.check(name);
        return rc ? rc : list_run(name, c, g, contig, r, stats);
    });
}

// load + call + free: the sequences (one, or A and B of a pair) become contigs 0 and 1 of a genome that lives for the call.
// Everything that can be refused from the arguments and the bytes is refused before the context is looked at.  Nothing behind a
// range is read, so the sequences are loaded with the smallest guard gap.
template <class R>
static int list_one_shot(const char *name, prf_ctx *c, std::initializer_list<const prf_contig *> seqs, const R &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        for (const prf_contig *seq : seqs)
            if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        const prf_contig *const *s = seqs.begin();
        typename R::room o{};
        if constexpr (R::pair) o.b_len = s[1]->len;
        if ((rc = r.check_room(name, s[0]->len, &o))) return rc;
        for (const prf_contig *seq : seqs)
            if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_contig contigs[2] = {*s[0], *s[seqs.size() - 1]};
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, contigs, (int)seqs.size(), 64, &g))) return rc;
        rc = list_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}
