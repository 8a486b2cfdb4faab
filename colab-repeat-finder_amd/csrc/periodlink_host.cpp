// periodlink_host.cpp -- the host path of the list of junctions between the chains of the period lines of a range
// (prf_period_links, its _ex and one-shot forms; kernels: periodchain.hip for the heads, periodlink.hip for the join).
// Modelled on dotlink_host.cpp and periodchain_host.cpp, whose order of refusals it keeps and whose stage it shares
// (periodchain_stage.h).  One call = one window of start positions x one range of k of the successors:
//   1. the heads of the window: the rows of prf_period_chains at min_len = 0, by its find and long kernels; they stay on the
//      device.  2^20 rows of room at first, the exact number (up to PRF_PCHAIN_MAX_ROWS) if there were more.
//   2. the join kernel, one wave per head: at most one link each, judged against all lines 1 .. n - 1.
// The rows are copied and sorted here.  No selection is read, no row sink written, the last scan's rows stay.
#include <algorithm>
#include <vector>

#include "periodchain_stage.h"

namespace {

constexpr u64 first_head_rows = 1ull << 20;

struct plinks_request {
    static constexpr u32 path = 11;
    u64 begin, end;
    u64 pos0, pos1;
    u32 kmin, kmax, n_matches;
    u64 min_seed;
    u32 max_gap, max_shift;
    prf_plink *dst;
    u64 capacity;
    uint64_t *n_links;
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS
    using room = pchain_room;

    int check(const char *name) const {
        if (begin > end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (pos0 > pos1) return fail(PRF_EINVAL, "%s: pos0 %llu is behind pos1 %llu", name, (unsigned long long)pos0, (unsigned long long)pos1);
        if (!kmin) return fail(PRF_EINVAL, "%s: kmin is 0. It must be at least 1.", name);
        if (kmin > kmax) return fail(PRF_EINVAL, "%s: kmin %u is above kmax %u", name, kmin, kmax);
        if (n_matches > 1) return fail(PRF_EINVAL, "%s: n_matches is %u. It must be 0 (N never matches) or 1 (N == N matches).", name, n_matches);
        if (!min_seed) return fail(PRF_EINVAL, "%s: min_seed is 0. It must be at least 1.", name);
        if (max_gap > PRF_DOTCHAIN_MAX_GAP)
            return fail(PRF_EUNSUPPORTED, "%s: a max_gap of %u cells is above %u (PRF_DOTCHAIN_MAX_GAP)", name, max_gap, PRF_DOTCHAIN_MAX_GAP);
        if (!max_shift) return fail(PRF_EINVAL, "%s: max_shift is 0. It must be at least 1: chains of one line are joined by max_gap.", name);
        if (max_shift > PRF_DOTLINK_MAX_SHIFT)
            return fail(PRF_EUNSUPPORTED, "%s: a max_shift of %u lines is above %u (PRF_DOTLINK_MAX_SHIFT)", name, max_shift, PRF_DOTLINK_MAX_SHIFT);
        if (capacity > PRF_PCHAIN_MAX_ROWS)
            return fail(PRF_EUNSUPPORTED, "%s: a capacity of %llu rows is above %llu (PRF_PCHAIN_MAX_ROWS)", name,
                        (unsigned long long)capacity, (unsigned long long)PRF_PCHAIN_MAX_ROWS);
        if (!n_links) return fail(PRF_EINVAL, "%s: NULL n_links", name);
        if (!dst && capacity) return fail(PRF_EINVAL, "%s: NULL destination with a capacity of %llu rows", name, (unsigned long long)capacity);
        return PRF_OK;
    }

    int check_room(const char *name, u64 seq_len, room *o) const {
        return pchain_check_room(name, begin, end, pos0, pos1, kmin, kmax, seq_len, o);
    }
};

int plinks_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const plinks_request &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    plinks_request::room o{};
    if ((rc = r.check_room(name, v.len, &o))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    HIPCHK(hipSetDevice(c->dev));
    float ms_find = 0, ms_long = 0, ms_join = 0;
    u32 launches = 0;
    u64 n_heads = 0, n_links = 0;
    if (pchain_any(o, r.kmin)) {
        // ---- 1. the heads: every chain that starts in the window, whatever its length
        const prf_periodchain_args a = pchain_args(v, o, r.begin, r.kmin, r.kmax, r.n_matches, r.min_seed, r.max_gap, 0);
        dev_array<prf_pchain_dev> d_heads;
        dev_array<prf_pchain_long> d_long;
        dev_array<u64> d_cnt;
        u64 cnt[PRF_PC_N] = {0, 0, 0};
        const u64 most = ((u64)a.kmax - a.kmin + 1) * (o.pos1 - o.pos0);           // <= 2^42
        u64 cap = most < first_head_rows ? most : first_head_rows;
        if ((rc = pchain_rows(name, c, a, r.launch_cells, cap, d_heads, d_long, d_cnt, cnt, &ms_find, &ms_long, &launches))) return rc;
        n_heads = cnt[PRF_PC_CHAINS];
        if (n_heads > cap) {
            if (n_heads > PRF_PCHAIN_MAX_ROWS)
                return fail(PRF_EUNSUPPORTED, "%s: %llu chains start in the window, a call links at most %llu (PRF_PCHAIN_MAX_ROWS): ask for a smaller window, fewer periods or a larger min_seed",
                            name, (unsigned long long)n_heads, (unsigned long long)PRF_PCHAIN_MAX_ROWS);
            cap = n_heads;
            if ((rc = pchain_rows(name, c, a, r.launch_cells, cap, d_heads, d_long, d_cnt, cnt, &ms_find, &ms_long, &launches))) return rc;
            if (cnt[PRF_PC_CHAINS] != cap)
                return fail(PRF_EHIP, "%s: the second pass found %llu chains, the first %llu", name, (unsigned long long)cnt[PRF_PC_CHAINS], (unsigned long long)cap);
        }
        // ---- 2. the join: every head is at most one link
        if (n_heads) {
            dev_array<prf_plink_dev> d_out;
            dev_array<u64> d_links;
            if ((rc = d_out.alloc(r.capacity)) || (rc = d_links.alloc(1))) return rc;
            prf_periodlink_args k{};
            k.pl = a.pl;
            k.g_begin = a.g_begin;
            k.n = a.n;
            k.n_matches = r.n_matches;
            k.max_gap = r.max_gap;
            k.max_shift = r.max_shift;
            k.min_seed = r.min_seed;
            k.heads = d_heads.p;
            k.n_heads = n_heads;
            k.dst = d_out.p;
            k.capacity = r.capacity;
            k.counter = d_links.p;
            HIPCHK(hipMemsetAsync(d_links.p, 0, sizeof(u64), c->stream));
            HIPCHK(hipEventRecord(c->ev[0], c->stream));
            HIPCHK(prf_launch_periodlink_join(c->stream, k));
            ++launches;
            HIPCHK(hipEventRecord(c->ev[1], c->stream));
            HIPCHK(hipMemcpyAsync(&n_links, d_links.p, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipEventElapsedTime(&ms_join, c->ev[0], c->ev[1]));
            if (n_links > n_heads)
                return fail(PRF_EHIP, "%s: %llu links into %llu chain heads", name, (unsigned long long)n_links, (unsigned long long)n_heads);
            if (n_links && n_links <= r.capacity) {
                std::vector<prf_plink> got(n_links);
                static_assert(sizeof(prf_plink) == sizeof(prf_plink_dev), "one layout");
                HIPCHK(hipMemcpy(got.data(), d_out.p, n_links * sizeof(prf_plink), hipMemcpyDeviceToHost));
                std::sort(got.begin(), got.end(), [](const prf_plink &x, const prf_plink &y) { return x.start != y.start ? x.start < y.start : x.k < y.k; });
                memcpy(r.dst, got.data(), n_links * sizeof(prf_plink));
            }
        }
    }
    *r.n_links = n_links;
    lane_stats(stats, plinks_request::path, ms_find + ms_long + ms_join, o.n, (o.n + 3) / 4, launches);
    if (stats) {
        stats->n_hits = n_links;
        stats->n_candidates = n_heads;       // the chain heads of the window; the time of the chain kernels and of the join kernel
        stats->phase1_ms = ms_find + ms_long;
        stats->phase2_ms = ms_join;
    }
    return PRF_OK;
}

int plinks_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const plinks_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = r.check(name);
        return rc ? rc : plinks_run(name, c, g, contig, r, stats);
    });
}

// Everything that can be refused from the arguments and the bytes is refused before the context is looked at.  Nothing behind the
// range is read, so the sequence is loaded with the smallest guard gap.
int plinks_one_shot(const char *name, prf_ctx *c, const prf_contig *seq, const plinks_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        plinks_request::room o{};
        if ((rc = r.check_room(name, seq->len, &o))) return rc;
        if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, 64, &g))) return rc;
        rc = plinks_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_period_links_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                        uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                        prf_plink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats, uint64_t launch_cells) {
    return plinks_on_genome("prf_period_links", c, g, contig,
                            plinks_request{begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, max_shift, dst, capacity, n_links,
                                           launch_cells},
                            stats);
}

int prf_period_links(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                     uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                     prf_plink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats) {
    return prf_period_links_ex(c, g, contig, begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, max_shift, dst, capacity,
                               n_links, stats, 0);
}

int prf_period_links_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1, uint32_t kmin,
                         uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift, prf_plink *dst,
                         uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats) {
    return plinks_one_shot("prf_period_links_seq", c, seq,
                           plinks_request{begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, max_shift, dst, capacity, n_links, 0},
                           stats);
}

}  // extern "C"
