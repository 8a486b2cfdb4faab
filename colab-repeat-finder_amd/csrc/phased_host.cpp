// phased_host.cpp -- the consensus motifs of rows whose positions come as segments with a phase (prf_phased_consensus, its _ex
// and one-shot forms; kernels: phased.hip for the counts, consensus.hip's finish kernel for the letters), on the frame
// of consensus_frame.h: here are what the product refuses, how its SEGMENTS are cut into work items and which kernel counts them.
// The order of the refusals is part of the interface (include/prf_phased.h; tests/test_phased_cpu.py).
#include "consensus_frame.h"
#include "phased_launch.h"

namespace {

struct phased_request {
    static constexpr u32 path = 13;
    u64 begin, end;
    const uint32_t *ks;
    u64 n_rows;
    const prf_segment *segments;
    u64 n_segments;
    prf_consensus *dst;
    char *motifs;
    u64 letters_capacity;
    u32 *counts;               // NULL: not wanted
    u64 slice;                 // 0: PRF_CONSENSUS_SLICE

    struct work {
        std::vector<ph_item> items;
        dev_array<ph_item> d_items;
        dev_array<ph_segment> d_segments;
    };

    // what can be said without a genome; *letters = the sum of k
    int check(const char *name, u64 *letters) const {
        *letters = 0;
        const int rc = cs_check_head(name, begin, end, n_rows);
        if (rc) return rc;
        if (n_segments > PRF_PHASED_MAX_SEGMENTS)
            return fail(PRF_EUNSUPPORTED, "%s: %llu segments are above %llu (PRF_PHASED_MAX_SEGMENTS)", name, (unsigned long long)n_segments,
                        (unsigned long long)PRF_PHASED_MAX_SEGMENTS);
        if (!n_rows) return PRF_OK;
        if (!ks) return fail(PRF_EINVAL, "%s: NULL ks", name);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        if (!motifs) return fail(PRF_EINVAL, "%s: NULL motifs", name);
        if (n_segments && !segments) return fail(PRF_EINVAL, "%s: NULL segments", name);
        u64 sum = 0;
        for (u64 i = 0; i < n_rows; i++) {
            if (!ks[i]) return fail(PRF_EINVAL, "%s: row %llu: k is 0. It must be at least 1.", name, (unsigned long long)i);
            sum += ks[i];      // 2^24 rows x 2^32: no overflow
        }
        u64 positions = 0;     // the sum of end - start, saturating: no column of any row can hold more
        for (u64 i = 0; i < n_segments; i++) {
            const prf_segment &s = segments[i];
            const unsigned long long at = i;
            if (s.start >= s.end)
                return fail(PRF_EINVAL, "%s: segment %llu: start %llu is not in front of end %llu", name, at, (unsigned long long)s.start,
                            (unsigned long long)s.end);
            if (s.row >= n_rows)
                return fail(PRF_EINVAL, "%s: segment %llu: row %u is not one of the %llu rows", name, at, s.row, (unsigned long long)n_rows);
            if (s.phase >= ks[s.row])
                return fail(PRF_EINVAL, "%s: segment %llu: phase %u is not below the k = %u of row %u", name, at, s.phase, ks[s.row], s.row);
            const u64 len = s.end - s.start;
            positions = positions + len < positions ? ~0ull : positions + len;
        }
        // the most a column of a row can hold: a 32-bit count must do.  Only segments that add up to 2^32 positions can break
        // that; then the rows are looked at one by one (2^24 segments x 2^64 / k: the sums saturate)
        if (positions > 0xFFFFFFFFull) {
            std::vector<u64> most(n_rows, 0);
            for (u64 i = 0; i < n_segments; i++) {
                const prf_segment &s = segments[i];
                const u64 add = (s.end - s.start - 1) / ks[s.row] + 1, have = most[s.row];
                most[s.row] = have + add < have ? ~0ull : have + add;
            }
            for (u64 i = 0; i < n_rows; i++)
                if (most[i] > 0xFFFFFFFFull)
                    return fail(PRF_EUNSUPPORTED, "%s: row %llu: a column of more than 2^32 - 1 positions (its segments at k = %u)", name,
                                (unsigned long long)i, ks[i]);
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
        for (u64 i = 0; i < n_segments; i++)
            if (segments[i].end > n)
                return fail(PRF_EINVAL, "%s: segment %llu: end %llu is behind the range's %llu positions", name, (unsigned long long)i,
                            (unsigned long long)segments[i].end, (unsigned long long)n);
        return PRF_OK;
    }

    // the rows with their offsets, and the items of the segments, regime by regime
    int cut(const char *name, cs_cut &cut, work &w) const {
        const u64 at_most = slice ? slice : PRF_CONSENSUS_SLICE;
        cut.rows.resize(n_rows);
        u64 offset = 0;
        for (u64 i = 0; i < n_rows; i++) {
            cut.rows[i] = cs_row{0, 0, offset, ks[i], 0u};     // the positions of a row are its segments'
            offset += ks[i];
        }
        for (u64 i = 0; i < n_segments; i++) {
            const prf_segment &s = segments[i];
            const int rc = cs_count_items(name, cut, ks[s.row], s.end - s.start, at_most, "segments");
            if (rc) return rc;
        }
        w.items.resize(cut.n_items());
        u64 next[PRF_CS_REGIMES] = {0, cut.per_regime[0], cut.per_regime[0] + cut.per_regime[1]};
        for (u64 i = 0; i < n_segments; i++) {
            const prf_segment &s = segments[i];
            const u64 len = s.end - s.start, n = cs_n_items(len, at_most);
            u64 &at = next[cs_regime(ks[s.row])];
            for (u64 j = 0; j < n; j++) {
                u64 first, last;
                cs_item_span(len, at_most, j, &first, &last);
                w.items[at++] = ph_item{s.start + first, s.start + last, (u32)i, 0u};
            }
        }
        return PRF_OK;
    }

    int upload(hipStream_t st, work &w) const {
        static_assert(sizeof(ph_segment) == sizeof(prf_segment), "one layout");
        int rc;
        if ((rc = w.d_items.alloc(w.items.size())) || (rc = w.d_segments.alloc(n_segments))) return rc;
        if (!n_segments) return PRF_OK;
        HIPCHK(hipMemcpyAsync(w.d_items.p, w.items.data(), w.items.size() * sizeof(ph_item), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(w.d_segments.p, segments, n_segments * sizeof(prf_segment), hipMemcpyHostToDevice, st));
        return PRF_OK;
    }

    int count(hipStream_t st, const prf_consensus_args &a, const work &w, u32 regime, u64 item0, u64 n) const {
        prf_phased_args p{};
        p.pl = a.pl;
        p.g_begin = a.g_begin;
        p.rows = a.rows;
        p.n_rows = a.n_rows;
        p.segments = w.d_segments.p;
        p.n_segments = n_segments;
        p.items = w.d_items.p;
        p.counts = a.counts;
        HIPCHK(prf_launch_phased_count(st, p, regime, item0, n));
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_phased_consensus_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const uint32_t *ks,
                            uint64_t n_rows, const prf_segment *segments, uint64_t n_segments, prf_consensus *dst, char *motifs,
                            uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats, uint64_t slice_positions) {
    const phased_request r{begin, end, ks, n_rows, segments, n_segments, dst, motifs, letters_capacity, counts, slice_positions};
    return cs_on_genome("prf_phased_consensus", c, g, contig, r, stats);
}

int prf_phased_consensus(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const uint32_t *ks,
                         uint64_t n_rows, const prf_segment *segments, uint64_t n_segments, prf_consensus *dst, char *motifs,
                         uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats) {
    return prf_phased_consensus_ex(c, g, contig, begin, end, ks, n_rows, segments, n_segments, dst, motifs, letters_capacity, counts, stats, 0);
}

int prf_phased_consensus_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, const uint32_t *ks, uint64_t n_rows,
                             const prf_segment *segments, uint64_t n_segments, prf_consensus *dst, char *motifs,
                             uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats) {
    const phased_request r{begin, end, ks, n_rows, segments, n_segments, dst, motifs, letters_capacity, counts, 0};
    return cs_one_shot("prf_phased_consensus_seq", c, seq, r, stats);
}

}  // extern "C"
