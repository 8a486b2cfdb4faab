// dotlink_host.cpp -- the list of junctions between the chains of the dot plot of two ranges (prf_dotpair_links, its _ex and
// one-shot forms; kernels: dotruns.hip for the seeds, dotlink.hip for the heads and the join) as a request on the frame
// of list_host.h.  One call = one window of start cells of the successors:
//   1. the seeds of the window at min_len = min_seed (dotseeds_host.h); they stay on the device.
//   2. the heads kernel, one thread per seed: the indices of the seeds that start a chain.
//   3. the join kernel, one wave per head: at most one link each.
#include "dotseeds_host.h"

namespace {

struct links_request : pair_window, list_output<prf_dotlink, prf_dotlink_dev> {
    static constexpr u32 path = 9;
    u64 min_seed;
    u32 max_gap, max_shift;

    int check(const char *name) const {
        int rc = check_window(name);
        if (!rc) rc = list_check_seed_gap(name, min_seed, max_gap);
        if (!rc) rc = list_check_shift(name, max_shift);
        if (!rc) rc = list_check_output(name, dst, capacity, n_out, "n_links", PRF_DOTCHAIN_MAX_ROWS, "PRF_DOTCHAIN_MAX_ROWS");
        return rc;
    }

    // n_candidates: the chain heads of the window; the phases: the seed kernels, the link kernels
    int body(const char *name, prf_ctx *c, const prf_contig_view &v, const room &o, dev_array<prf_dotlink_dev> &d_out, list_result &res) const {
        dev_array<prf_dotrun_dev> d_seeds, d_long;
        dev_array<u64> d_cnt;
        const prf_dotruns_args a = seeds_args(v, o, *this, min_seed);
        u64 n_seeds = 0;
        int rc;
        if ((rc = d_long.alloc(a.long_cap)) || (rc = d_cnt.alloc(PRF_DR_N + PRF_DL_N))) return rc;
        // ---- 1. the seeds
        if ((rc = all_seeds(name, c, a, launch_cells, o, d_seeds, d_long, d_cnt.p, &n_seeds, &res.ms1, &res.launches))) return rc;
        if (!n_seeds) return PRF_OK;
        // ---- 2. the heads: every seed is at most one entry
        dev_array<u32> d_heads;
        prf_dotlink_args k{};
        k.seed_rows = d_seeds.p;
        k.n_seeds = n_seeds;
        k.min_seed = min_seed;
        k.max_gap = max_gap;
        k.max_shift = max_shift;
        k.capacity = capacity;
        k.counters = d_cnt.p + PRF_DR_N;
        if ((rc = d_heads.alloc(n_seeds)) || (rc = d_out.alloc(k.capacity))) return rc;
        k.heads = d_heads.p;
        k.dst = d_out.p;
        u64 cnt[PRF_DL_N] = {0, 0};
        HIPCHK(hipMemsetAsync(k.counters, 0, PRF_DL_N * sizeof(u64), c->stream));
        rc = timed_step(c, [&]() -> int {
            HIPCHK(prf_launch_dotlink_heads(c->stream, a, k));
            ++res.launches;
            return PRF_OK;
        }, cnt, k.counters, PRF_DL_N, &res.ms2);
        if (rc) return rc;
        const u64 n_heads = res.n_candidates = cnt[PRF_DL_HEADS];
        if (n_heads > n_seeds)
            return fail(PRF_EHIP, "%s: %llu chain heads among %llu seeds", name, (unsigned long long)n_heads, (unsigned long long)n_seeds);
        // ---- 3. the join: every head is at most one link
        if (n_heads) {
            rc = timed_step(c, [&]() -> int {
                HIPCHK(prf_launch_dotlink_join(c->stream, a, k, n_heads));
                ++res.launches;
                return PRF_OK;
            }, cnt, k.counters, PRF_DL_N, &res.ms2);
            if (rc) return rc;
        }
        res.n = cnt[PRF_DL_LINKS];
        if (res.n > n_heads)
            return fail(PRF_EHIP, "%s: %llu links into %llu chain heads", name, (unsigned long long)res.n, (unsigned long long)n_heads);
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_dotpair_links_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                         uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                         uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift, prf_dotlink *dst,
                         uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats, uint64_t launch_cells) {
    return list_on_genome("prf_dotpair_links", c, g, a_contig,
                          links_request{{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions},
                                        {dst, capacity, n_links, launch_cells}, min_seed, max_gap, max_shift},
                          stats);
}

int prf_dotpair_links(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                      uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                      uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift, prf_dotlink *dst, uint64_t capacity,
                      uint64_t *n_links, prf_scan_stats *stats) {
    return prf_dotpair_links_ex(c, g, a_contig, a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions,
                                min_seed, max_gap, max_shift, dst, capacity, n_links, stats, 0);
}

int prf_dotpair_links_seq(prf_ctx *c, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                          uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                          uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift, prf_dotlink *dst,
                          uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats) {
    return list_one_shot("prf_dotpair_links_seq", c, {seq_a, seq_b},
                         links_request{{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, directions},
                                       {dst, capacity, n_links, 0}, min_seed, max_gap, max_shift},
                         stats);
}

}  // extern "C"
