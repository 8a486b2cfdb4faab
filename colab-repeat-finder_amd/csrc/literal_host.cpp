// literal_host.cpp -- the literal lane (scan_literal.hip): regimes outside the closed form of the packed kernels (min_repeats == 1).
// One sequence at a time, straight from its ASCII bytes (upper-cased on the device): one thread per (position, motif size)
// evaluates the reference's flush call as written; the rows are then sorted like reference :81 and reduced to the shortest
// motif per (start, end) -- what the reference's dictionary holds at the end (utils/perfect_repeat_tracker.py:93-101) -- on the
// device as well (prf_lit_sort_unique).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "genome.h"

// d_seq: L bytes on the device (16-byte aligned: the 64-positions kernel reads whole 16-byte groups, 16 readable bytes behind them); upper: not upper-cased / validated yet
// front: the N trimmed off the front of the contig -- the rows and the position of an unsupported symbol are shifted by it
static int literal_device(prf_ctx *c, uint8_t *d_seq, u64 L, bool upper, u32 contig_index, const scan_params &p, u64 stop,
                          std::vector<prf_hit> &rows_out, float *ms, u32 *launches, u64 front) {
    if (stop > L) stop = L;
    dev_array<prf_hit_dev> rows;
    u64 cap = L / 16 + 4096;
    u64 *h = c->h_counters;
    for (int attempt = 0;; attempt++) {
        if (const int rc = rows.alloc(cap)) return rc;
        HIPCHK(hipMemsetAsync(c->d_counters, 0, PRF_CNT_N * sizeof(u64), c->stream));
        HIPCHK(hipMemsetAsync(c->d_counters + PRF_CNT_BADPOS, 0xFF, sizeof(u64), c->stream));
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        if (attempt == 0 && upper) HIPCHK(prf_launch_lit_upper(c->stream, d_seq, L, c->d_counters + PRF_CNT_BADPOS));
        HIPCHK(prf_launch_lit_events(c->stream, d_seq, L, p.kmin, p.kmax, p.min_repeats, p.min_span, stop, contig_index, rows.p, cap,
                                     c->d_counters));
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(h, c->d_counters, PRF_CNT_N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        *ms += t;
        *launches += attempt == 0 && upper ? 2 : 1;
        if (h[PRF_CNT_BADPOS] != ~0ull)
            return fail(PRF_ESYMBOL,
                        "unsupported symbol at contig %u position %llu: only letters are accepted (A, C, G, T, N and -- as ordinary "
                        "symbols, like the reference -- any other letter, in either case); libprf refuses other bytes instead of guessing",
                        contig_index, (unsigned long long)(h[PRF_CNT_BADPOS] + front));
        if (h[PRF_CNT_CAND])
            return fail(PRF_EINDEX, "string index out of range");  // the message of Python's IndexError (tracker :87)
        const u64 n = h[PRF_CNT_HITS];
        if (n <= cap) {
            // sorted by (start, end) and reduced to the shortest motif per (start, end) on the device (scan_literal.hip)
            if (n) {
                dev_array<prf_hit_dev> uniq;
                if (const int rc = uniq.alloc(n)) return rc;
                u64 *d_n = c->d_counters + PRF_CNT_HITS;  // read above; reused for the number of rows that stay
                HIPCHK(prf_lit_sort_unique(c->stream, rows.p, n, uniq.p, d_n, &c->lit_scratch, &c->lit_scratch_bytes));
                HIPCHK(hipMemcpyAsync(h, d_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                const u64 kept = h[0];
                if (kept > n) return fail(PRF_EHIP, "prf_scan_literal: row compaction returned %llu of %llu rows", (unsigned long long)kept,
                                          (unsigned long long)n);
                const size_t at = rows_out.size();
                rows_out.resize(at + kept);
                if (kept) {
                    HIPCHK(hipMemcpyAsync(rows_out.data() + at, uniq.p, kept * sizeof(prf_hit), hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(hipStreamSynchronize(c->stream));
                }
                for (size_t r = at; r < rows_out.size(); r++) {
                    rows_out[r].start += front;
                    rows_out[r].end += front;
                }
                *launches += 5;
            }
            return PRF_OK;
        }
        if (attempt >= 2) return fail(PRF_EHIP, "prf_scan_literal: the row count changed between two runs");
        cap = n;
    }
}

static int literal_one(prf_ctx *c, const prf_contig &ct, u32 contig_index, const scan_params &p, u64 stop,
                       std::vector<prf_hit> &rows_out, float *ms, u32 *launches, u64 front) {
    const u64 L = ct.len;
    if (L && !ct.ascii) return fail(PRF_EINVAL, "prf_scan_literal: NULL sequence");
    if (L >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "prf_scan_literal: input too large (2^40 positions)");
    dev_array<uint8_t> seq;
    if (const int rc = seq.alloc(L + 16)) return rc;
    if (L) HIPCHK(hipMemcpyAsync(seq.p, ct.ascii, L, hipMemcpyHostToDevice, c->stream));
    return literal_device(c, seq.p, L, true, contig_index, p, stop, rows_out, ms, launches, front);
}

// what the literal lane refuses on a context: a row sink, pipelined scans in flight
static int literal_preamble(const prf_ctx *c, const char *api) {
    if (c->sink) return fail(PRF_EUNSUPPORTED, "min_repeats == 1: not with a row sink (the rows of the literal lane are handed over on the host)");
    return refuse_in_flight(c, api);
}

static int literal_finish(prf_ctx *c, std::vector<prf_hit> &rows, float ms, u32 launches, u64 positions, prf_hits *out,
                          prf_scan_stats *stats) {
    c->last.nhits = 0;  // the rows of this lane live on the host only
    c->last.rows = nullptr;
    lane_stats(stats, 2, ms, positions, positions, launches);  // packed_bytes: this lane reads the bytes themselves
    if (stats) stats->n_candidates = stats->n_hits = rows.size();
    if (!out || rows.empty()) return PRF_OK;
    prf_hit *r = (prf_hit *)malloc(rows.size() * sizeof(prf_hit));
    if (!r) return fail(PRF_ENOMEM, "prf_scan_literal: cannot allocate %zu rows", rows.size());
    memcpy(r, rows.data(), rows.size() * sizeof(prf_hit));
    out->rows = r;
    out->n = rows.size();
    return PRF_OK;
}

// min_repeats == 1 on a RESIDENT genome: the upper-cased bytes of every contig are rebuilt on the device from the linear
// planes (H, L, X and the code planes of the symbols outside ACGTN), trimmed of the N at both ends (reference
// perfect_repeat_finder.py:40-46) and handed to the literal lane -- nothing crosses PCIe but the rows.
int prf_literal_genome(prf_ctx *c, const prf_genome *g, const scan_params &p, prf_hits *out, prf_scan_stats *stats) {
    if (g->sel_on)
        return fail(PRF_EUNSUPPORTED, "min_repeats == 1 scans whole contigs (its rows depend on where a sequence begins and ends): "
                                      "clear the selection of parts (prf_genome_select with n_parts == 0)");
    const int rc = literal_preamble(c, "prf_scan_genome");
    if (rc) return rc;
    std::vector<prf_hit> rows;
    float ms = 0;
    u32 launches = 0;
    for (size_t ci = 0; ci < g->len.size(); ci++) {
        const u64 len = g->len[ci];
        u64 lo = len, hi = len;  // nothing but N (or empty): the reference's window is seq[len:len]
        if (len) {
            u64 fl[2] = {~0ull, 0ull};
            HIPCHK(hipMemcpyAsync(c->d_counters, fl, sizeof fl, hipMemcpyHostToDevice, c->stream));
            HIPCHK(prf_launch_lit_trim(c->stream, g->X, g->E, g->base[ci] >> 6, len, c->d_counters));
            HIPCHK(hipMemcpyAsync(c->h_counters, c->d_counters, sizeof fl, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            launches++;
            if (c->h_counters[0] != ~0ull) { lo = c->h_counters[0]; hi = c->h_counters[1]; }
        }
        const u64 n = hi - lo;
        dev_array<uint8_t> seq;
        if (const int rc = seq.alloc(n + 16)) return rc;
        if (n) {
            HIPCHK(prf_launch_lit_unpack(c->stream, g->H, g->L, g->X, g->E, g->base[ci] + lo, n, seq.p));
            launches++;
        }
        const int rc = literal_device(c, seq.p, n, false, (u32)ci, p, n, rows, &ms, &launches, lo);
        if (rc) return rc;
    }
    return literal_finish(c, rows, ms, launches, g->positions, out, stats);
}

int prf_literal_impl(prf_ctx *c, const prf_contig *contigs, int n_contigs, const u64 *stops, const scan_params &p, prf_hits *out,
                     prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "prf_scan_literal: NULL context");
    if (out) { out->rows = nullptr; out->n = 0; }
    if (n_contigs < 0 || (n_contigs && !contigs)) return fail(PRF_EINVAL, "prf_scan_literal: bad contig array");
    int rc = check_params(p.kmin, p.kmax, p.min_repeats, p.min_span, 0);
    if (!rc) rc = literal_preamble(c, "prf_scan_literal");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->dev));
    std::vector<prf_hit> rows;
    float ms = 0;
    u32 launches = 0;
    u64 positions = 0;
    for (int i = 0; i < n_contigs; i++) {
        prf_contig w = contigs[i];
        u64 lo = 0;
        if (!stops && w.len) {
            // prf_scan: the whole of reference detect_repeats() without an interval, whose :40-46 drop the N at both ends
            // first -- not a no-op in this regime, the rows depend on where the sequence begins and ends
            if (!w.ascii) return fail(PRF_EINVAL, "prf_scan: NULL sequence");
            u64 hi = w.len;
            while (lo < hi && (w.ascii[lo] | 0x20) == 'n') lo++;
            while (hi > lo && (w.ascii[hi - 1] | 0x20) == 'n') hi--;
            w.ascii += lo;
            w.len = hi - lo;
        }
        rc = literal_one(c, w, (u32)i, p, stops ? stops[i] : w.len, rows, &ms, &launches, lo);
        if (rc) return rc;
        positions += contigs[i].len;
    }
    return literal_finish(c, rows, ms, launches, positions, out, stats);
}

extern "C" {

int prf_scan_literal(prf_ctx *c, const prf_contig *contig, uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span,
                     uint64_t stop, prf_hits *out, prf_scan_stats *stats) {
    if (!contig) return fail(PRF_EINVAL, "prf_scan_literal: NULL contig");
    const u64 stop_ = stop;
    return guarded("prf_scan_literal", [&] {
        return prf_literal_impl(c, contig, 1, &stop_, scan_params{kmin, kmax, min_repeats, min_span}, out, stats);
    });
}

}  // extern "C"
