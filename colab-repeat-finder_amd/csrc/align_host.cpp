// align_host.cpp -- the alignment of a list of tandem repeats of a range to their motifs (prf_motif_align and its one-shot form;
// kernel: align.hip).  "Rows in, rows out, in the order they came", like the consensus products, whose head refusals
// (consensus_frame.h) and whose row type it shares; the motifs go IN here, and nothing is counted, so the run is its own: judge
// the arguments (before the context or the genome is looked at), take the contig's planes, clip `end`, sort the rows by regime
// and length, run one launch per regime between events, copy the rows out.  No selection is read, no row sink written, the rows
// of the last scan stay where they are.  The order of the refusals is part of the interface (include/prf_align.h;
// tests/test_align_cpu.py).
#include "align_launch.h"
#include "consensus_frame.h"

namespace {

struct align_request {
    static constexpr u32 path = 14;
    u64 begin, end;
    const prf_repeat *rows;
    u64 n_rows;
    const char *motifs;
    u64 letters_length;
    prf_alignment *dst;

    // what can be said without a genome; *letters = the sum of k
    int check(const char *name, u64 *letters) const {
        *letters = 0;
        const int rc = cs_check_head(name, begin, end, n_rows);
        if (rc || !n_rows) return rc;
        if (!rows) return fail(PRF_EINVAL, "%s: NULL rows", name);
        if (!motifs) return fail(PRF_EINVAL, "%s: NULL motifs", name);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        u64 sum = 0;
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
            sum += r.k;        // 2^24 rows x 2^10: no overflow
        }
        const int lrc = cs_check_letters(name, sum, letters_length);
        if (lrc) return lrc;
        u64 offset = 0;
        for (u64 i = 0; i < n_rows; offset += rows[i++].k)
            for (u32 j = 0; j < rows[i].k; j++)
                if (al_motif_code(motifs[offset + j]) == 0xFFu)
                    return fail(PRF_EINVAL, "%s: row %llu: column %u of the motif is the byte 0x%02x, not one of A C G T N", name,
                                (unsigned long long)i, j, (unsigned)(unsigned char)motifs[offset + j]);
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

int al_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const align_request &r, u64 letters, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = r.check_room(name, v.len))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    std::vector<al_row> sorted(r.n_rows);
    u64 offset = 0, positions = 0, cells = 0;
    for (u64 i = 0; i < r.n_rows; i++) {
        const prf_repeat &in = r.rows[i];
        sorted[i] = al_row{in.start, in.end, offset, in.k, (u32)i};
        offset += in.k;
        positions += in.end - in.start;
        cells += (in.end - in.start) * in.k;   // 2^24 rows x 2^19 x 2^10: no overflow
    }
    u64 per_regime[PRF_AL_REGIMES];
    al_sort_rows(sorted, per_regime);
    // ---- the device's side
    HIPCHK(hipSetDevice(c->dev));
    dev_array<al_row> d_rows;
    dev_array<char> d_motifs;
    dev_array<al_result> d_out;
    dev_array<u64> d_spare;    // timed_step copies counter words; this product has none, so one word that stays 0
    if ((rc = d_rows.alloc(r.n_rows)) || (rc = d_motifs.alloc(letters)) || (rc = d_out.alloc(r.n_rows)) || (rc = d_spare.alloc(1))) return rc;
    HIPCHK(hipMemcpyAsync(d_rows.p, sorted.data(), r.n_rows * sizeof(al_row), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_motifs.p, r.motifs, letters, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_out.p, 0, r.n_rows * sizeof(al_result), c->stream));
    HIPCHK(hipMemsetAsync(d_spare.p, 0, sizeof(u64), c->stream));
    prf_align_args a{};
    a.pl = v.planes;
    a.g_begin = v.base + r.begin;
    a.rows = d_rows.p;
    a.motifs = d_motifs.p;
    a.dst = d_out.p;
    a.n_results = r.n_rows;
    float ms = 0;
    u32 launches = 0;
    u64 spare = 0;
    rc = timed_step(c, [&]() -> int {
        u64 row0 = 0;
        for (u32 regime = 0; regime < PRF_AL_REGIMES; row0 += per_regime[regime++]) {
            if (!per_regime[regime]) continue;
            HIPCHK(prf_launch_align(c->stream, a, regime, row0, per_regime[regime]));
            ++launches;
        }
        return PRF_OK;
    }, &spare, d_spare.p, 1, &ms);
    if (rc) return rc;
    static_assert(sizeof(prf_alignment) == sizeof(al_result), "one layout");
    HIPCHK(hipMemcpyAsync(r.dst, d_out.p, r.n_rows * sizeof(prf_alignment), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lane_stats(stats, align_request::path, ms, positions, (positions + 3) / 4, launches);
    if (stats) {
        stats->n_hits = r.n_rows;
        stats->n_candidates = cells;
    }
    return PRF_OK;
}

}  // namespace

extern "C" {

int prf_motif_align(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                    uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, prf_scan_stats *stats) {
    const align_request r{begin, end, rows, n_rows, motifs, letters_length, dst};
    return guarded("prf_motif_align", [&] {
        u64 letters;
        const int rc = r.check("prf_motif_align", &letters);
        if (rc || !r.n_rows) return rc;
        return al_run("prf_motif_align", c, g, contig, r, letters, stats);
    });
}

// load + call + free, as cs_one_shot does it: everything that can be refused from the arguments and the bytes is refused before
// the context is looked at
int prf_motif_align_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows, uint64_t n_rows,
                        const char *motifs, uint64_t letters_length, prf_alignment *dst, prf_scan_stats *stats) {
    const char *name = "prf_motif_align_seq";
    const align_request r{begin, end, rows, n_rows, motifs, letters_length, dst};
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
        rc = al_run(name, c, g, 0, r, letters, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // extern "C"
