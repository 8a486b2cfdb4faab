// alignpath_host.cpp -- the alignment of a list of tandem repeats of a range to their motifs with its path (prf_motif_align_path,
// its _ex and its one-shot form; kernels: alignpath.hip).  The frame is align_host.cpp's: judge the arguments (before
// the context or the genome is looked at), take the contig's planes, clip `end`, sort the rows by regime and length
// (al_sort_rows).  Then the rows are dealt into batches whose trace fits the scratch (ap_deal); per batch one forward launch per
// regime and one walk, the trace of a batch being read before the next batch overwrites it; at the end one counts launch over
// the whole path.  No selection is read, no row sink written, the rows of the last scan stay where they are.  The order of the
// refusals is part of the interface (include/prf_alignpath.h; tests/test_alignpath_cpu.py).
#include "alignpath_launch.h"
#include "consensus_frame.h"

namespace {

struct alignpath_request {
    static constexpr u32 path_id = 15;
    u64 begin, end;
    const prf_repeat *rows;
    u64 n_rows;
    const char *motifs;
    u64 letters_length;
    prf_alignment *dst;
    uint16_t *path;
    u64 path_capacity;
    u32 *counts;
    u64 trace_bytes;           // 0: PRF_ALIGNPATH_TRACE_BYTES

    // what can be said without a genome; *letters = the sum of k, *positions = the sum of n_r
    int check(const char *name, u64 *letters, u64 *positions) const {
        *letters = *positions = 0;
        const int rc = cs_check_head(name, begin, end, n_rows);
        if (rc || !n_rows) return rc;
        if (!rows) return fail(PRF_EINVAL, "%s: NULL rows", name);
        if (!motifs) return fail(PRF_EINVAL, "%s: NULL motifs", name);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        if (!path) return fail(PRF_EINVAL, "%s: NULL path", name);
        u64 sum = 0, entries = 0;
        for (u64 i = 0; i < n_rows; i++) {
            const prf_repeat &r = rows[i];
            const unsigned long long at = i;
            if (!r.k) return fail(PRF_EINVAL, "%s: row %llu: k is 0. It must be at least 1.", name, at);
            if (r.start >= r.end)
                return fail(PRF_EINVAL, "%s: row %llu: start %llu is not in front of end %llu", name, at, (unsigned long long)r.start,
                            (unsigned long long)r.end);
            if (r.reserved) return fail(PRF_EINVAL, "%s: row %llu: reserved is %u. It must be 0.", name, at, r.reserved);
            if (r.k > PRF_ALIGN_MAX_K)
                return fail(PRF_EUNSUPPORTED, "%s: row %llu: k = %u is above %u (PRF_ALIGN_MAX_K)", name, at, r.k, PRF_ALIGN_MAX_K);
            if (r.end - r.start > PRF_ALIGN_MAX_LEN)
                return fail(PRF_EUNSUPPORTED, "%s: row %llu: %llu positions are above %llu (PRF_ALIGN_MAX_LEN)", name, at,
                            (unsigned long long)(r.end - r.start), (unsigned long long)PRF_ALIGN_MAX_LEN);
            sum += r.k;                    // 2^24 rows x 2^10: no overflow
            entries += r.end - r.start;    // 2^24 rows x 2^19: no overflow
        }
        const int lrc = cs_check_letters(name, sum, letters_length);
        if (lrc) return lrc;
        if (entries > PRF_ALIGNPATH_MAX_POSITIONS)
            return fail(PRF_EUNSUPPORTED, "%s: the rows add up to %llu positions, above %llu (PRF_ALIGNPATH_MAX_POSITIONS)", name,
                        (unsigned long long)entries, (unsigned long long)PRF_ALIGNPATH_MAX_POSITIONS);
        if (entries > path_capacity)
            return fail(PRF_EINVAL, "%s: the path holds %llu entries, the rows add up to %llu positions", name,
                        (unsigned long long)path_capacity, (unsigned long long)entries);
        u64 offset = 0;
        for (u64 i = 0; i < n_rows; offset += rows[i++].k)
            for (u32 j = 0; j < rows[i].k; j++)
                if (al_motif_code(motifs[offset + j]) == 0xFFu)
                    return fail(PRF_EINVAL, "%s: row %llu: column %u of the motif is the byte 0x%02x, not one of A C G T N", name,
                                (unsigned long long)i, j, (unsigned)(unsigned char)motifs[offset + j]);
        *letters = sum;
        *positions = entries;
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

int ap_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const alignpath_request &r, u64 letters, u64 positions,
           prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = r.check_room(name, v.len))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    // ---- the rows: in input order for the counts kernel, sorted for the other two
    std::vector<al_row> order(r.n_rows);
    std::vector<u64> first(r.n_rows + 1), start(r.n_rows), offsets(r.n_rows);
    u64 offset = 0, entries = 0, cells = 0;
    for (u64 i = 0; i < r.n_rows; i++) {
        const prf_repeat &in = r.rows[i];
        order[i] = al_row{in.start, in.end, offset, in.k, (u32)i};
        first[i] = entries;
        start[i] = in.start;
        offsets[i] = offset;
        offset += in.k;
        entries += in.end - in.start;
        cells += (in.end - in.start) * in.k;   // 2^24 rows x 2^19 x 2^10: no overflow
    }
    first[r.n_rows] = entries;
    u64 per_regime[PRF_AL_REGIMES];
    al_sort_rows(order, per_regime);
    std::vector<ap_row> sorted(r.n_rows);
    for (u64 i = 0; i < r.n_rows; i++) {
        const al_row &o = order[i];
        sorted[i] = ap_row{o.start, o.end, o.offset, o.k, o.index, 0ull, first[o.index]};
    }
    std::vector<ap_batch> batches;
    ap_deal(sorted, (r.trace_bytes ? r.trace_bytes : PRF_ALIGNPATH_TRACE_BYTES) / sizeof(u32), batches);
    u64 trace_words = 0;
    for (const ap_batch &b : batches) trace_words = std::max(trace_words, b.words);
    // ---- the device's side
    HIPCHK(hipSetDevice(c->dev));
    dev_array<ap_row> d_rows;
    dev_array<char> d_motifs;
    dev_array<al_result> d_out;
    dev_array<u32> d_trace, d_counts;
    dev_array<unsigned short> d_path;
    dev_array<u64> d_first, d_start, d_offset;
    dev_array<u64> d_spare;    // timed_step copies counter words; this product has none, so one word that stays 0
    if ((rc = d_rows.alloc(r.n_rows)) || (rc = d_motifs.alloc(letters)) || (rc = d_out.alloc(r.n_rows)) || (rc = d_trace.alloc(trace_words)) ||
        (rc = d_path.alloc(positions)) || (rc = d_first.alloc(r.n_rows + 1)) || (rc = d_start.alloc(r.n_rows)) ||
        (rc = d_offset.alloc(r.n_rows)) || (rc = d_spare.alloc(1)))
        return rc;
    if (r.counts && (rc = d_counts.alloc(6 * letters))) return rc;
    HIPCHK(hipMemcpyAsync(d_rows.p, sorted.data(), r.n_rows * sizeof(ap_row), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_motifs.p, r.motifs, letters, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_first.p, first.data(), (r.n_rows + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_start.p, start.data(), r.n_rows * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_offset.p, offsets.data(), r.n_rows * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_out.p, 0, r.n_rows * sizeof(al_result), c->stream));
    HIPCHK(hipMemsetAsync(d_path.p, 0, positions * sizeof(unsigned short), c->stream));
    if (r.counts) HIPCHK(hipMemsetAsync(d_counts.p, 0, 6 * letters * sizeof(u32), c->stream));
    HIPCHK(hipMemsetAsync(d_spare.p, 0, sizeof(u64), c->stream));
    prf_alignpath_args a{};
    a.pl = v.planes;
    a.g_begin = v.base + r.begin;
    a.rows = d_rows.p;
    a.motifs = d_motifs.p;
    a.dst = d_out.p;
    a.n_results = r.n_rows;
    a.trace = d_trace.p;
    a.trace_words = trace_words;
    a.path = d_path.p;
    a.n_path = positions;
    a.counts = r.counts ? d_counts.p : nullptr;
    prf_alignpath_count_args ca{};
    ca.pl = v.planes;
    ca.g_begin = a.g_begin;
    ca.first = d_first.p;
    ca.start = d_start.p;
    ca.offset = d_offset.p;
    ca.n_rows = r.n_rows;
    ca.motifs = d_motifs.p;
    ca.path = d_path.p;
    ca.n_path = positions;
    ca.counts = a.counts;
    float ms1 = 0, ms2 = 0;
    u32 launches = 0;
    u64 spare = 0;
    // a batch's walk reads the trace before the next batch's forward pass overwrites it, so the two phases alternate, each
    // between events of its own
    for (const ap_batch &b : batches) {
        rc = timed_step(c, [&]() -> int {
            u64 row0 = b.row0;
            const u64 row_end = b.row0 + b.n_rows;
            while (row0 < row_end) {                                           // the runs of one regime
                const u32 regime = al_regime(sorted[row0].k);
                u64 n = 1;
                while (row0 + n < row_end && al_regime(sorted[row0 + n].k) == regime) ++n;
                HIPCHK(prf_launch_alignpath_forward(c->stream, a, regime, row0, n));
                ++launches;
                row0 += n;
            }
            return PRF_OK;
        }, &spare, d_spare.p, 1, &ms1);
        if (rc) return rc;
        rc = timed_step(c, [&]() -> int {
            HIPCHK(prf_launch_alignpath_walk(c->stream, a, b.row0, b.n_rows));
            ++launches;
            return PRF_OK;
        }, &spare, d_spare.p, 1, &ms2);
        if (rc) return rc;
    }
    rc = timed_step(c, [&]() -> int {
        HIPCHK(prf_launch_alignpath_counts(c->stream, ca));
        ++launches;
        return PRF_OK;
    }, &spare, d_spare.p, 1, &ms2);
    if (rc) return rc;
    static_assert(sizeof(prf_alignment) == sizeof(al_result) && sizeof(uint16_t) == sizeof(unsigned short), "one layout");
    HIPCHK(hipMemcpyAsync(r.dst, d_out.p, r.n_rows * sizeof(prf_alignment), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(r.path, d_path.p, positions * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    if (r.counts) HIPCHK(hipMemcpyAsync(r.counts, d_counts.p, 6 * letters * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lane_stats(stats, alignpath_request::path_id, ms1 + ms2, positions, (positions + 3) / 4, launches);
    if (stats) {
        stats->n_hits = r.n_rows;
        stats->n_candidates = cells;
        stats->phase1_ms = ms1;
        stats->phase2_ms = ms2;
    }
    return PRF_OK;
}

int ap_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const alignpath_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        u64 letters, positions;
        const int rc = r.check(name, &letters, &positions);
        if (rc || !r.n_rows) return rc;
        return ap_run(name, c, g, contig, r, letters, positions, stats);
    });
}

}  // namespace

extern "C" {

int prf_motif_align_path(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                         uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, uint16_t *path,
                         uint64_t path_capacity, uint32_t *counts, prf_scan_stats *stats) {
    return ap_on_genome("prf_motif_align_path", c, g, contig,
                        alignpath_request{begin, end, rows, n_rows, motifs, letters_length, dst, path, path_capacity, counts, 0}, stats);
}

int prf_motif_align_path_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                            uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, uint16_t *path,
                            uint64_t path_capacity, uint32_t *counts, prf_scan_stats *stats, uint64_t trace_bytes) {
    return ap_on_genome("prf_motif_align_path_ex", c, g, contig,
                        alignpath_request{begin, end, rows, n_rows, motifs, letters_length, dst, path, path_capacity, counts, trace_bytes}, stats);
}

// load + call + free, as prf_motif_align_seq does it: everything that can be refused from the arguments and the bytes is refused
// before the context is looked at
int prf_motif_align_path_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows, uint64_t n_rows,
                             const char *motifs, uint64_t letters_length, prf_alignment *dst, uint16_t *path, uint64_t path_capacity,
                             uint32_t *counts, prf_scan_stats *stats) {
    const char *name = "prf_motif_align_path_seq";
    const alignpath_request r{begin, end, rows, n_rows, motifs, letters_length, dst, path, path_capacity, counts, 0};
    return guarded(name, [&] {
        u64 letters, positions;
        int rc = r.check(name, &letters, &positions);
        if (rc || !r.n_rows) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        if ((rc = r.check_room(name, seq->len))) return rc;
        if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, 64, &g))) return rc;    // nothing behind a range is read: the smallest guard gap
        rc = ap_run(name, c, g, 0, r, letters, positions, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // extern "C"
