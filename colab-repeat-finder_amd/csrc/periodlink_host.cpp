// periodlink_host.cpp -- the list of junctions between the chains of the period lines of a range (prf_period_links, its _ex and
// one-shot forms; kernels: periodchain.hip for the heads, periodlink.hip for the join) as a request on the frame of
// list_host.h.  One call = one window of start positions x one range of k of the successors:
//   1. the heads of the window: the rows of the stage of periodchain_stage.h at min_len = 0; they stay on the device.  2^20 rows
//      of room at first, the exact number (up to PRF_PCHAIN_MAX_ROWS) if there were more.
//   2. the join kernel, one wave per head: at most one link each, judged against all lines 1 .. n - 1.
#include "periodchain_stage.h"

namespace {

constexpr u64 first_head_rows = 1ull << 20;

struct plinks_request : period_window, list_output<prf_plink, prf_plink_dev> {
    static constexpr u32 path = 11;
    u64 min_seed;
    u32 max_gap, max_shift;

    int check(const char *name) const {
        int rc = check_window(name);
        if (!rc) rc = list_check_seed_gap(name, min_seed, max_gap);
        if (!rc) rc = list_check_shift(name, max_shift);
        if (!rc) rc = list_check_output(name, dst, capacity, n_out, "n_links", PRF_PCHAIN_MAX_ROWS, "PRF_PCHAIN_MAX_ROWS");
        return rc;
    }

    // n_candidates: the chain heads of the window; the phases: the chain kernels, the join kernel
    int body(const char *name, prf_ctx *c, const prf_contig_view &v, const room &o, dev_array<prf_plink_dev> &d_out, list_result &res) const {
        // ---- 1. the heads: every chain that starts in the window, whatever its length
        const prf_periodchain_args a = pchain_args(v, o, *this, min_seed, max_gap, 0);
        dev_array<prf_pchain_dev> d_heads;
        dev_array<prf_pchain_long> d_long;
        dev_array<u64> d_cnt, d_links;
        const u64 most = ((u64)a.kmax - a.kmin + 1) * (o.pos1 - o.pos0);           // <= 2^42
        int rc = grow_once(name, most < first_head_rows ? most : first_head_rows, PRF_PCHAIN_MAX_ROWS, "PRF_PCHAIN_MAX_ROWS", "chains",
                           "a smaller window, fewer periods or a larger min_seed", [&](u64 cap, u64 *n) {
                               u64 cnt[PRF_PC_N] = {0, 0, 0};
                               const int rc = pchain_rows(name, c, a, launch_cells, cap, d_heads, d_long, d_cnt, cnt, &res.ms1, &res.ms1, &res.launches);
                               *n = cnt[PRF_PC_CHAINS];
                               return rc;
                           }, &res.n_candidates);
        if (rc || !res.n_candidates) return rc;
        // ---- 2. the join: every head is at most one link
        if ((rc = d_out.alloc(capacity)) || (rc = d_links.alloc(1))) return rc;
        prf_periodlink_args k{};
        k.pl = a.pl;
        k.g_begin = a.g_begin;
        k.n = a.n;
        k.n_matches = n_matches;
        k.max_gap = max_gap;
        k.max_shift = max_shift;
        k.min_seed = min_seed;
        k.heads = d_heads.p;
        k.n_heads = res.n_candidates;
        k.dst = d_out.p;
        k.capacity = capacity;
        k.counter = d_links.p;
        HIPCHK(hipMemsetAsync(d_links.p, 0, sizeof(u64), c->stream));
        rc = timed_step(c, [&]() -> int {
            HIPCHK(prf_launch_periodlink_join(c->stream, k));
            ++res.launches;
            return PRF_OK;
        }, &res.n, d_links.p, 1, &res.ms2);
        if (rc) return rc;
        if (res.n > k.n_heads)
            return fail(PRF_EHIP, "%s: %llu links into %llu chain heads", name, (unsigned long long)res.n, (unsigned long long)k.n_heads);
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_period_links_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                        uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                        prf_plink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats, uint64_t launch_cells) {
    return list_on_genome("prf_period_links", c, g, contig,
                          plinks_request{{begin, end, pos0, pos1, kmin, kmax, n_matches}, {dst, capacity, n_links, launch_cells},
                                         min_seed, max_gap, max_shift},
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
    return list_one_shot("prf_period_links_seq", c, {seq},
                         plinks_request{{begin, end, pos0, pos1, kmin, kmax, n_matches}, {dst, capacity, n_links, 0}, min_seed, max_gap,
                                        max_shift},
                         stats);
}

}  // extern "C"
