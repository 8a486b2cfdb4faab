// dotchain_host.cpp -- the list of chained diagonal runs of the dot plot of two ranges (prf_dotpair_chains, its _ex and one-shot
// forms; kernels: dotruns.hip for the seeds, dotchain.hip for the chains) as a request on the frame of list_host.h.
// One call = one window of start cells:
//   1. the seeds of the window at min_len = min_seed (dotseeds_host.h); they stay on the device.
//   2. the link kernel, one thread per seed: head test, follow, rows or entries of the long list.
//   3. the long kernel for the chains the link kernel left, one wave each.
#include "dotseeds_host.h"

namespace {

struct chains_request : pair_window, list_output<prf_dotchain, prf_dotchain_dev> {
    static constexpr u32 path = 8;
    u64 min_seed;
    u32 max_gap;
    u64 min_len;

    int check(const char *name) const {
        int rc = check_window(name);
        if (!rc) rc = list_check_seed_gap(name, min_seed, max_gap);
        if (!rc) rc = list_check_output(name, dst, capacity, n_out, "n_chains", PRF_DOTCHAIN_MAX_ROWS, "PRF_DOTCHAIN_MAX_ROWS");
        return rc;
    }

    // n_candidates: the seeds of the window; the phases: the seed kernels, the chain kernels
    int body(const char *name, prf_ctx *c, const prf_contig_view &v, const room &o, dev_array<prf_dotchain_dev> &d_out, list_result &res) const {
        dev_array<prf_dotrun_dev> d_seeds, d_long;
        dev_array<u64> d_cnt;
        const prf_dotruns_args a = seeds_args(v, o, *this, min_seed);
        int rc;
        if ((rc = d_long.alloc(a.long_cap)) || (rc = d_cnt.alloc(PRF_DR_N + PRF_DC_N))) return rc;
        // ---- 1. the seeds
        if ((rc = all_seeds(name, c, a, launch_cells, o, d_seeds, d_long, d_cnt.p, &res.n_candidates, &res.ms1, &res.launches))) return rc;
        if (!res.n_candidates) return PRF_OK;
        // ---- 2. link: every seed is at most one row or one entry of the long list
        dev_array<prf_dotchain_long> d_clong;
        prf_dotchain_args k{};
        k.seed_rows = d_seeds.p;
        k.n_seeds = res.n_candidates;
        k.min_seed = min_seed;
        k.min_len = min_len;
        k.max_gap = max_gap;
        k.capacity = capacity;
        k.long_cap = k.n_seeds < PRF_DOTCHAIN_LONG_ROWS ? k.n_seeds : PRF_DOTCHAIN_LONG_ROWS;
        k.counters = d_cnt.p + PRF_DR_N;
        if ((rc = d_out.alloc(k.capacity)) || (rc = d_clong.alloc(k.long_cap))) return rc;
        k.dst = d_out.p;
        k.longs = d_clong.p;
        u64 cnt[PRF_DC_N] = {0, 0};
        HIPCHK(hipMemsetAsync(k.counters, 0, PRF_DC_N * sizeof(u64), c->stream));
        rc = timed_step(c, [&]() -> int {
            HIPCHK(prf_launch_dotchain_link(c->stream, a, k));
            ++res.launches;
            return PRF_OK;
        }, cnt, k.counters, PRF_DC_N, &res.ms2);
        if (rc) return rc;
        if (cnt[PRF_DC_LONG] > k.long_cap)
            return fail(PRF_EUNSUPPORTED, "%s: %llu chains are still going %u cells (PRF_DOTCHAIN_FOLLOW) behind their first seed, the call keeps room for %llu: ask for smaller windows",
                        name, (unsigned long long)cnt[PRF_DC_LONG], PRF_DOTCHAIN_FOLLOW, (unsigned long long)k.long_cap);
        // ---- 3. the chains the link kernel left
        if (cnt[PRF_DC_LONG]) {
            rc = timed_step(c, [&]() -> int {
                HIPCHK(prf_launch_dotchain_long(c->stream, a, k, cnt[PRF_DC_LONG]));
                ++res.launches;
                return PRF_OK;
            }, cnt, k.counters, PRF_DC_N, &res.ms2);
            if (rc) return rc;
        }
        res.n = cnt[PRF_DC_CHAINS];
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_dotpair_chains_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                          uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                          uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint64_t min_len, prf_dotchain *dst,
                          uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats, uint64_t launch_cells) {
    return list_on_genome("prf_dotpair_chains", c, g, a_contig,
                          chains_request{{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions},
                                         {dst, capacity, n_chains, launch_cells}, min_seed, max_gap, min_len},
                          stats);
}

int prf_dotpair_chains(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                       uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                       uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint64_t min_len, prf_dotchain *dst, uint64_t capacity,
                       uint64_t *n_chains, prf_scan_stats *stats) {
    return prf_dotpair_chains_ex(c, g, a_contig, a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions,
                                 min_seed, max_gap, min_len, dst, capacity, n_chains, stats, 0);
}

int prf_dotpair_chains_seq(prf_ctx *c, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                           uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                           uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint64_t min_len, prf_dotchain *dst,
                           uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats) {
    return list_one_shot("prf_dotpair_chains_seq", c, {seq_a, seq_b},
                         chains_request{{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, directions},
                                        {dst, capacity, n_chains, 0}, min_seed, max_gap, min_len},
                         stats);
}

}  // extern "C"
