// consensus_host.cpp -- the consensus motifs of a list of tandem repeats of a range (prf_period_consensus, its _ex and one-shot
// forms; kernels: consensus.hip), on the frame of consensus_frame.h: here are what the product refuses, how its rows
// are cut into work items and which kernel counts them.  The order of the refusals is part of the interface
// (include/prf_consensus.h; tests/test_consensus_cpu.py).
#include "consensus_frame.h"

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

    struct work {
        std::vector<cs_item> items;
        dev_array<cs_item> d_items;
    };

    // what can be said without a genome; *letters = the sum of k
    int check(const char *name, u64 *letters) const {
        *letters = 0;
        const int rc = cs_check_head(name, begin, end, n_rows);
        if (rc || !n_rows) return rc;
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
        const int lrc = cs_check_letters(name, sum, letters_capacity);
        if (lrc) return lrc;
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

    // the rows with their offsets, and the items, regime by regime
    int cut(const char *name, cs_cut &cut, work &w) const {
        const u64 at_most = slice ? slice : PRF_CONSENSUS_SLICE;
        cut.rows.resize(n_rows);
        u64 offset = 0;
        for (u64 i = 0; i < n_rows; i++) {
            const prf_repeat &in = rows[i];
            cut.rows[i] = cs_row{in.start, in.end, offset, in.k, 0u};
            offset += in.k;
            const int rc = cs_count_items(name, cut, in.k, in.end - in.start, at_most, "rows");
            if (rc) return rc;
        }
        w.items.resize(cut.n_items());
        u64 next[PRF_CS_REGIMES] = {0, cut.per_regime[0], cut.per_regime[0] + cut.per_regime[1]};
        for (u64 i = 0; i < n_rows; i++) {
            const prf_repeat &in = rows[i];
            const u64 len = in.end - in.start, n = cs_n_items(len, at_most);
            u64 &at = next[cs_regime(in.k)];
            for (u64 j = 0; j < n; j++) {
                u64 first, last;
                cs_item_span(len, at_most, j, &first, &last);
                w.items[at++] = cs_item{in.start + first, in.start + last, (u32)i, 0u};
            }
        }
        return PRF_OK;
    }

    int upload(hipStream_t st, work &w) const {
        const int rc = w.d_items.alloc(w.items.size());
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(w.d_items.p, w.items.data(), w.items.size() * sizeof(cs_item), hipMemcpyHostToDevice, st));
        return PRF_OK;
    }

    int count(hipStream_t st, prf_consensus_args a, const work &w, u32 regime, u64 item0, u64 n) const {
        a.items = w.d_items.p;
        HIPCHK(prf_launch_consensus_count(st, a, regime, item0, n));
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_period_consensus_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                            uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                            prf_scan_stats *stats, uint64_t slice_positions) {
    const consensus_request r{begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, slice_positions};
    return cs_on_genome("prf_period_consensus", c, g, contig, r, stats);
}

int prf_period_consensus(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                         uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                         prf_scan_stats *stats) {
    return prf_period_consensus_ex(c, g, contig, begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, stats, 0);
}

int prf_period_consensus_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows, uint64_t n_rows,
                             prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats) {
    const consensus_request r{begin, end, rows, n_rows, dst, motifs, letters_capacity, counts, 0};
    return cs_one_shot("prf_period_consensus_seq", c, seq, r, stats);
}

}  // extern "C"
