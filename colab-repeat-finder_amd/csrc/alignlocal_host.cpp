// alignlocal_host.cpp -- the local alignment of a list of windows of a range to motifs under (match, mismatch, indel) weights
// (prf_motif_align_local and its one-shot form; kernel: alignlocal.hip).  The host path is align_host.cpp's: judge the
// arguments (before the context or the genome is looked at), take the contig's planes, clip `end`, sort the rows by regime and
// length, run one launch per regime between events, copy the rows out.  No selection is read, no row sink written, the rows of
// the last scan stay where they are.  The order of the refusals is part of the interface (include/prf_alignlocal.h;
// tests/test_alignlocal_cpu.py): the weights are judged behind the range and in front of the rows' limit.
#include "alignlocal_launch.h"
#include "consensus_frame.h"

namespace {

struct alignlocal_request {
    static constexpr u32 path = 16;
    u64 begin, end;
    const prf_repeat *rows;
    u64 n_rows;
    const char *motifs;
    u64 letters_length;
    u32 match, mismatch, indel;
    prf_local_alignment *dst;

    // a weight of 0 first, then a weight above the limit; match, mismatch, indel in this order
    int check_weights(const char *name) const {
        const struct {
            const char *what;
            u32 w;
        } all[3] = {{"match", match}, {"mismatch", mismatch}, {"indel", indel}};
        for (const auto &x : all)
            if (!x.w) return fail(PRF_EINVAL, "%s: %s is 0. A weight must be at least 1.", name, x.what);
        for (const auto &x : all)
            if (x.w > PRF_ALIGNLOCAL_MAX_WEIGHT)
                return fail(PRF_EUNSUPPORTED, "%s: %s = %u is above %u (PRF_ALIGNLOCAL_MAX_WEIGHT)", name, x.what, x.w, PRF_ALIGNLOCAL_MAX_WEIGHT);
        return PRF_OK;
    }

    // what can be said without a genome; *letters = the sum of k
    int check(const char *name, u64 *letters) const {
        *letters = 0;
        int rc = cs_check_head(name, begin, end, 0);                          // the range
        if (rc || (rc = check_weights(name)) || (rc = cs_check_head(name, begin, end, n_rows)) || !n_rows) return rc;
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

int all_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const alignlocal_request &r, u64 letters, prf_scan_stats *stats) {
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
    dev_array<all_result> d_out;
    dev_array<u64> d_spare;    // timed_step copies counter words; this product has none, so one word that stays 0
    if ((rc = d_rows.alloc(r.n_rows)) || (rc = d_motifs.alloc(letters)) || (rc = d_out.alloc(r.n_rows)) || (rc = d_spare.alloc(1))) return rc;
    HIPCHK(hipMemcpyAsync(d_rows.p, sorted.data(), r.n_rows * sizeof(al_row), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_motifs.p, r.motifs, letters, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_out.p, 0, r.n_rows * sizeof(all_result), c->stream));
    HIPCHK(hipMemsetAsync(d_spare.p, 0, sizeof(u64), c->stream));
    prf_alignlocal_args a{};
    a.pl = v.planes;
    a.g_begin = v.base + r.begin;
    a.rows = d_rows.p;
    a.motifs = d_motifs.p;
    a.dst = d_out.p;
    a.n_results = r.n_rows;
    a.match = r.match;
    a.mismatch = r.mismatch;
    a.indel = r.indel;
    float ms = 0;
    u32 launches = 0;
    u64 spare = 0;
    rc = timed_step(c, [&]() -> int {
        u64 row0 = 0;
        for (u32 regime = 0; regime < PRF_AL_REGIMES; row0 += per_regime[regime++]) {
            if (!per_regime[regime]) continue;
            HIPCHK(prf_launch_alignlocal(c->stream, a, regime, row0, per_regime[regime]));
            ++launches;
        }
        return PRF_OK;
    }, &spare, d_spare.p, 1, &ms);
    if (rc) return rc;
    static_assert(sizeof(prf_local_alignment) == sizeof(all_result), "one layout");
    HIPCHK(hipMemcpyAsync(r.dst, d_out.p, r.n_rows * sizeof(prf_local_alignment), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lane_stats(stats, alignlocal_request::path, ms, positions, (positions + 3) / 4, launches);
    if (stats) {
        stats->n_hits = r.n_rows;
        stats->n_candidates = cells;
    }
    return PRF_OK;
}

}  // namespace

extern "C" {

int prf_motif_align_local(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                          uint64_t n_rows, const char *motifs, uint64_t letters_length, uint32_t match, uint32_t mismatch,
                          uint32_t indel, prf_local_alignment *dst, prf_scan_stats *stats) {
    const alignlocal_request r{begin, end, rows, n_rows, motifs, letters_length, match, mismatch, indel, dst};
    return guarded("prf_motif_align_local", [&] {
        u64 letters;
        const int rc = r.check("prf_motif_align_local", &letters);
        if (rc || !r.n_rows) return rc;
        return all_run("prf_motif_align_local", c, g, contig, r, letters, stats);
    });
}

// load + call + free, as prf_motif_align_seq does it: everything that can be refused from the arguments and the bytes is refused
// before the context is looked at
int prf_motif_align_local_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows, uint64_t n_rows,
                              const char *motifs, uint64_t letters_length, uint32_t match, uint32_t mismatch, uint32_t indel,
                              prf_local_alignment *dst, prf_scan_stats *stats) {
    const char *name = "prf_motif_align_local_seq";
    const alignlocal_request r{begin, end, rows, n_rows, motifs, letters_length, match, mismatch, indel, dst};
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
        rc = all_run(name, c, g, 0, r, letters, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // extern "C"
