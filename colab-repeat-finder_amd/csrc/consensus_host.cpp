// consensus_host.cpp -- the consensus motifs of a list of tandem repeats of a range (prf_period_consensus, its _ex and one-shot
// forms; kernels: consensus.hip).  "Rows in, rows out, in the order they came": a small frame of its own on the
// helpers the matrix and the list products share, not list_run's copy-and-sort.  One call: judge the arguments (before the
// context or the genome is looked at), take the contig's planes, clip `end`, cut the rows into work items sorted by regime,
// zero the counts, run the count kernels and the finish kernel between events, copy rows, letters and (if wanted) counts out.
// No selection is read, no row sink written, the rows of the last scan stay where they are.  The order of the refusals is part
// of the interface (include/prf_consensus.h; tests/test_consensus_cpu.py).
#include <vector>

#include "consensus_launch.h"
#include "list_host.h"

namespace {

struct consensus_request {
    static constexpr u32 path = 12;
    u64 begin, end;
    const prf_repeat *rows;
    u64 n_rows;
    prf_consensus *dst;
    char *motifs;
    u64 letters_capacity;
    u32 *counts;               // NULL: not wanted
    u64 slice;                 // 0: PRF_CONSENSUS_SLICE

    // what can be said without a genome; *letters = the sum of k
    int check(const char *name, u64 *letters) const {
        *letters = 0;
        if (begin > end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (n_rows > PRF_CONSENSUS_MAX_ROWS)
            return fail(PRF_EUNSUPPORTED, "%s: %llu rows are above %llu (PRF_CONSENSUS_MAX_ROWS)", name, (unsigned long long)n_rows,
                        (unsigned long long)PRF_CONSENSUS_MAX_ROWS);
        if (!n_rows) return PRF_OK;
        if (!rows) return fail(PRF_EINVAL, "%s: NULL rows", name);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        if (!motifs) return fail(PRF_EINVAL, "%s: NULL motifs", name);
        u64 sum = 0;
        for (u64 i = 0; i < n_rows; i++) {
            const prf_repeat &r = rows[i];
            const unsigned long long at = i;
            if (!r.k) return fail(PRF_EINVAL, "%s: row %llu: k is 0. It must be at least 1.", name, at);
            if (r.start >= r.end)
                return fail(PRF_EINVAL, "%s: row %llu: start %llu is not in front of end %llu", name, at, (unsigned long long)r.start,
                            (unsigned long long)r.end);
            if (r.reserved) return fail(PRF_EINVAL, "%s: row %llu: reserved is %u. It must be 0.", name, at, r.reserved);
            if ((r.end - r.start - 1) / r.k >= 0xFFFFFFFFull)
                return fail(PRF_EUNSUPPORTED, "%s: row %llu: a column of more than 2^32 - 1 positions (%llu positions at k = %u)", name, at,
                            (unsigned long long)(r.end - r.start), r.k);
            sum += r.k;        // 2^24 rows x 2^32: no overflow
        }
        if (sum > PRF_CONSENSUS_MAX_LETTERS)
            return fail(PRF_EUNSUPPORTED, "%s: the k of the rows add up to %llu letters, above %llu (PRF_CONSENSUS_MAX_LETTERS)", name,
                        (unsigned long long)sum, (unsigned long long)PRF_CONSENSUS_MAX_LETTERS);
        if (sum > letters_capacity)
            return fail(PRF_EINVAL, "%s: the destination holds %llu letters, the k of the rows add up to %llu", name,
                        (unsigned long long)letters_capacity, (unsigned long long)sum);
        *letters = sum;
        return PRF_OK;
    }

    // what needs the length of the sequence
    int check_room(const char *name, u64 seq_len) const {
        u64 n;
        const int rc = matrix_clip(name, begin, end, seq_len, &n);
        if (rc) return rc;
        for (u64 i = 0; i < n_rows; i++)
            if (rows[i].end > n)
                return fail(PRF_EINVAL, "%s: row %llu: end %llu is behind the range's %llu positions", name, (unsigned long long)i,
                            (unsigned long long)rows[i].end, (unsigned long long)n);
        return PRF_OK;
    }
};

int consensus_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const consensus_request &r, u64 letters,
                  prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = r.check_room(name, v.len))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    // ---- the rows with their offsets, and the items, regime by regime
    const u64 slice = r.slice ? r.slice : PRF_CONSENSUS_SLICE;
    std::vector<cs_row> rows(r.n_rows);
    u64 per_regime[PRF_CS_REGIMES] = {0, 0, 0}, offset = 0, positions = 0, n_items = 0;
    for (u64 i = 0; i < r.n_rows; i++) {
        const prf_repeat &in = r.rows[i];
        rows[i] = cs_row{in.start, in.end, offset, in.k, 0u};
        offset += in.k;
        positions += in.end - in.start;
        const u64 n = cs_n_items(in.end - in.start, slice);
        per_regime[cs_regime(in.k)] += n;
        n_items += n;
        if (n_items > PRF_CONSENSUS_MAX_ITEMS)
            return fail(PRF_EUNSUPPORTED, "%s: the rows cut into more than %llu work items of %llu positions (PRF_CONSENSUS_MAX_ITEMS): ask for a larger slice or fewer rows",
                        name, (unsigned long long)PRF_CONSENSUS_MAX_ITEMS, (unsigned long long)slice);
    }
    u64 item0[PRF_CS_REGIMES] = {0, per_regime[0], per_regime[0] + per_regime[1]};
    std::vector<cs_item> items(n_items);
    {
        u64 next[PRF_CS_REGIMES] = {item0[0], item0[1], item0[2]};
        for (u64 i = 0; i < r.n_rows; i++) {
            const prf_repeat &in = r.rows[i];
            const u64 len = in.end - in.start, n = cs_n_items(len, slice);
            u64 &at = next[cs_regime(in.k)];
            for (u64 j = 0; j < n; j++) {
                u64 first, end;
                cs_item_span(len, slice, j, &first, &end);
                items[at++] = cs_item{in.start + first, in.start + end, (u32)i, 0u};
            }
        }
    }
    // ---- the device's side
    HIPCHK(hipSetDevice(c->dev));
    dev_array<cs_row> d_rows;
    dev_array<cs_item> d_items;
    dev_array<u32> d_counts;
    dev_array<char> d_motifs;
    dev_array<prf_consensus_dev> d_out;
    dev_array<u64> d_spare;    // timed_step copies counter words; this product has none, so one word that stays 0
    if ((rc = d_rows.alloc(r.n_rows)) || (rc = d_items.alloc(n_items)) || (rc = d_counts.alloc(4 * letters)) || (rc = d_motifs.alloc(letters)) ||
        (rc = d_out.alloc(r.n_rows)) || (rc = d_spare.alloc(1)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_rows.p, rows.data(), r.n_rows * sizeof(cs_row), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_items.p, items.data(), n_items * sizeof(cs_item), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_counts.p, 0, 4 * letters * sizeof(u32), c->stream));
    HIPCHK(hipMemsetAsync(d_spare.p, 0, sizeof(u64), c->stream));
    prf_consensus_args a{};
    a.pl = v.planes;
    a.g_begin = v.base + r.begin;
    a.rows = d_rows.p;
    a.n_rows = r.n_rows;
    a.items = d_items.p;
    a.counts = d_counts.p;
    a.motifs = d_motifs.p;
    a.dst = d_out.p;
    float ms1 = 0, ms2 = 0;
    u32 launches = 0;
    u64 spare = 0;
    rc = timed_step(c, [&]() -> int {
        for (u32 regime = 0; regime < PRF_CS_REGIMES; regime++) {
            if (!per_regime[regime]) continue;
            HIPCHK(prf_launch_consensus_count(c->stream, a, regime, item0[regime], per_regime[regime]));
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
    lane_stats(stats, consensus_request::path, ms1 + ms2, positions, (positions + 3) / 4, launches);
    if (stats) {
        stats->n_hits = r.n_rows;
        stats->n_candidates = n_items;
        stats->phase1_ms = ms1;
        stats->phase2_ms = ms2;
    }
    return PRF_OK;
}

}  // namespace

extern "C" {

int prf_period_consensus_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                            uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                            prf_scan_stats *stats, uint64_t slice_positions) {
    const char *name = "prf_period_consensus";
    return guarded(name, [&] {
        const consensus_request r{begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, slice_positions};
        u64 letters;
        const int rc = r.check(name, &letters);
        if (rc || !n_rows) return rc;
        return consensus_run(name, c, g, contig, r, letters, stats);
    });
}

int prf_period_consensus(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                         uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                         prf_scan_stats *stats) {
    return prf_period_consensus_ex(c, g, contig, begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, stats, 0);
}

int prf_period_consensus_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows, uint64_t n_rows,
                             prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats) {
    const char *name = "prf_period_consensus_seq";
    return guarded(name, [&] {
        const consensus_request r{begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, 0};
        u64 letters;
        int rc = r.check(name, &letters);
        if (rc || !n_rows) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        if ((rc = r.check_room(name, seq->len))) return rc;
        if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, 64, &g))) return rc;    // nothing behind a range is read: the smallest guard gap
        rc = consensus_run(name, c, g, 0, r, letters, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // extern "C"
