// consensus_frame.h -- the host path that the two consensus products share (consensus_host.cpp: rows (start, end, k), DESIGN 18;
// phased_host.cpp: segments with a phase; align_host.cpp, DESIGN 20, takes the refusals of the head and of the letters
// from here and runs on its own; nobody else includes it).  "Rows in, rows out, in the order they came": a
// small frame of its own on the helpers the matrix and the list products share, not list_run's copy-and-sort.
//
// One call: judge the arguments (before the context or the genome is looked at), take the contig's planes, clip `end`, cut the
// input into work items sorted by regime, zero the counts, run the product's count kernels and the shared finish kernel between
// events, copy rows, letters and (if wanted) counts out.  No selection is read, no row sink written, the rows of the last scan
// stay where they are.
//
// A product is its request R:
//   static constexpr u32 path                      prf_scan_stats.path
//   u64 begin                                      the range's first position in the contig (its `end` is the request's own business)
//   u64 n_rows;  prf_consensus *dst;  char *motifs;  u32 *counts (NULL: not wanted)
//   int check(name, u64 *letters) const            what can be said without a genome; *letters = the sum of k
//   int check_room(name, seq_len) const            what needs the length of the sequence
//   struct work                                    the items on the host and what the count kernels read on the device
//   int cut(name, cs_cut &, work &) const          the rows with their offsets, the items regime by regime, the positions
//   int upload(stream, work &) const               the items (and what else the count kernels read) to the device
//   int count(stream, args, work, regime, item0, n) const
//                                                  the count kernel of one regime over items item0 .. item0 + n - 1
#pragma once
#include <vector>

#include "consensus_launch.h"
#include "list_host.h"

// what cut() reports: the rows as the kernels see them, the items per regime, the stats' positions
struct cs_cut {
    std::vector<cs_row> rows;
    u64 per_regime[PRF_CS_REGIMES] = {0, 0, 0};
    u64 positions = 0;
    u64 n_items() const { return per_regime[0] + per_regime[1] + per_regime[2]; }
};

// one more stretch of `len` positions of a row of k columns cut at `slice`: its items, counted against the limit
static int cs_count_items(const char *name, cs_cut &cut, u32 k, u64 len, u64 slice, const char *what) {
    cut.per_regime[cs_regime(k)] += cs_n_items(len, slice);
    cut.positions += len;
    if (cut.n_items() > PRF_CONSENSUS_MAX_ITEMS)
        return fail(PRF_EUNSUPPORTED, "%s: the %s cut into more than %llu work items of %llu positions (PRF_CONSENSUS_MAX_ITEMS): ask for a larger slice or fewer %s",
                    name, what, (unsigned long long)PRF_CONSENSUS_MAX_ITEMS, (unsigned long long)slice, what);
    return PRF_OK;
}

// the refusals of the head that the two products share: the range, the rows' limit
static int cs_check_head(const char *name, u64 begin, u64 end, u64 n_rows) {
    if (begin > end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)begin, (unsigned long long)end);
    if (n_rows > PRF_CONSENSUS_MAX_ROWS)
        return fail(PRF_EUNSUPPORTED, "%s: %llu rows are above %llu (PRF_CONSENSUS_MAX_ROWS)", name, (unsigned long long)n_rows,
                    (unsigned long long)PRF_CONSENSUS_MAX_ROWS);
    return PRF_OK;
}

// ... and of the letters: the sum of k against the limit and the caller's room
static int cs_check_letters(const char *name, u64 sum, u64 letters_capacity) {
    if (sum > PRF_CONSENSUS_MAX_LETTERS)
        return fail(PRF_EUNSUPPORTED, "%s: the k of the rows add up to %llu letters, above %llu (PRF_CONSENSUS_MAX_LETTERS)", name,
                    (unsigned long long)sum, (unsigned long long)PRF_CONSENSUS_MAX_LETTERS);
    if (sum > letters_capacity)
        return fail(PRF_EINVAL, "%s: the destination holds %llu letters, the k of the rows add up to %llu", name,
                    (unsigned long long)letters_capacity, (unsigned long long)sum);
    return PRF_OK;
}

template <class R>
static int cs_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const R &r, u64 letters, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = r.check_room(name, v.len))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    cs_cut cut;
    typename R::work w;
    if ((rc = r.cut(name, cut, w))) return rc;
    const u64 n_items = cut.n_items();
    const u64 item0[PRF_CS_REGIMES] = {0, cut.per_regime[0], cut.per_regime[0] + cut.per_regime[1]};
    // ---- the device's side
    HIPCHK(hipSetDevice(c->dev));
    dev_array<cs_row> d_rows;
    dev_array<u32> d_counts;
    dev_array<char> d_motifs;
    dev_array<prf_consensus_dev> d_out;
    dev_array<u64> d_spare;    // timed_step copies counter words; these products have none, so one word that stays 0
    if ((rc = d_rows.alloc(r.n_rows)) || (rc = d_counts.alloc(4 * letters)) || (rc = d_motifs.alloc(letters)) || (rc = d_out.alloc(r.n_rows)) ||
        (rc = d_spare.alloc(1)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_rows.p, cut.rows.data(), r.n_rows * sizeof(cs_row), hipMemcpyHostToDevice, c->stream));
    if ((rc = r.upload(c->stream, w))) return rc;
    HIPCHK(hipMemsetAsync(d_counts.p, 0, 4 * letters * sizeof(u32), c->stream));
    HIPCHK(hipMemsetAsync(d_spare.p, 0, sizeof(u64), c->stream));
    prf_consensus_args a{};
    a.pl = v.planes;
    a.g_begin = v.base + r.begin;
    a.rows = d_rows.p;
    a.n_rows = r.n_rows;
    a.counts = d_counts.p;
    a.motifs = d_motifs.p;
    a.dst = d_out.p;
    float ms1 = 0, ms2 = 0;
    u32 launches = 0;
    u64 spare = 0;
    rc = timed_step(c, [&]() -> int {
        for (u32 regime = 0; regime < PRF_CS_REGIMES; regime++) {
            if (!cut.per_regime[regime]) continue;
            const int lrc = r.count(c->stream, a, w, regime, item0[regime], cut.per_regime[regime]);
            if (lrc) return lrc;
            ++launches;
        }
        return PRF_OK;
    }, &spare, d_spare.p, 1, &ms1);
    if (rc) return rc;
    rc = timed_step(c, [&]() -> int {
        HIPCHK(prf_launch_consensus_finish(c->stream, a));
        ++launches;
        return PRF_OK;
    }, &spare, d_spare.p, 1, &ms2);
    if (rc) return rc;
    static_assert(sizeof(prf_consensus) == sizeof(prf_consensus_dev), "one layout");
    HIPCHK(hipMemcpyAsync(r.dst, d_out.p, r.n_rows * sizeof(prf_consensus), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(r.motifs, d_motifs.p, letters, hipMemcpyDeviceToHost, c->stream));
    if (r.counts) HIPCHK(hipMemcpyAsync(r.counts, d_counts.p, 4 * letters * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lane_stats(stats, R::path, ms1 + ms2, cut.positions, (cut.positions + 3) / 4, launches);
    if (stats) {
        stats->n_hits = r.n_rows;
        stats->n_candidates = n_items;
        stats->phase1_ms = ms1;
        stats->phase2_ms = ms2;
    }
    return PRF_OK;
}

template <class R>
static int cs_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const R &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        u64 letters;
        const int rc = r.check(name, &letters);
        if (rc || !r.n_rows) return rc;
        return cs_run(name, c, g, contig, r, letters, stats);
    });
}

// load + call + free; everything that can be refused from the arguments and the bytes is refused before the context is looked at
template <class R>
static int cs_one_shot(const char *name, prf_ctx *c, const prf_contig *seq, const R &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        u64 letters;
        int rc = r.check(name, &letters);
        if (rc || !r.n_rows) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        if ((rc = r.check_room(name, seq->len))) return rc;
        if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, 64, &g))) return rc;    // nothing behind a range is read: the smallest guard gap
        rc = cs_run(name, c, g, 0, r, letters, stats);
        prf_genome_free(g);
        return rc;
    });
}
