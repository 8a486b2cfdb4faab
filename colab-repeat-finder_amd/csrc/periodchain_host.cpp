// periodchain_host.cpp -- the list of diverged tandem repeats of a range (prf_period_chains, its _ex and one-shot forms; kernels:
// periodchain.hip) as a request on the frame of list_host.h.  One call = one window of start positions x one range of
// k; the rows are those of the stage of periodchain_stage.h at the caller's capacity and min_len.
#include "periodchain_stage.h"

namespace {

struct pchains_request : period_window, list_output<prf_pchain, prf_pchain_dev> {
    static constexpr u32 path = 10;
    u64 min_seed;
    u32 max_gap;
    u64 min_len;

    int check(const char *name) const {
        int rc = check_window(name);
        if (!rc) rc = list_check_seed_gap(name, min_seed, max_gap);
        if (!rc) rc = list_check_output(name, dst, capacity, n_out, "n_chains", PRF_PCHAIN_MAX_ROWS, "PRF_PCHAIN_MAX_ROWS");
        return rc;
    }

    // n_candidates: the seeds that start in the window; the phases: the find kernel, the long kernel
    int body(const char *name, prf_ctx *c, const prf_contig_view &v, const room &o, dev_array<prf_pchain_dev> &d_out, list_result &res) const {
        dev_array<prf_pchain_long> d_long;
        dev_array<u64> d_cnt;
        u64 cnt[PRF_PC_N] = {0, 0, 0};
        const int rc = pchain_rows(name, c, pchain_args(v, o, *this, min_seed, max_gap, min_len), launch_cells, capacity, d_out, d_long, d_cnt,
                                   cnt, &res.ms1, &res.ms2, &res.launches);
        res.n = cnt[PRF_PC_CHAINS];
        res.n_candidates = cnt[PRF_PC_SEEDS];
        return rc;
    }
};

}  // namespace

extern "C" {

int prf_period_chains_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                         uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                         prf_pchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats, uint64_t launch_cells) {
    return list_on_genome("prf_period_chains", c, g, contig,
                          pchains_request{{begin, end, pos0, pos1, kmin, kmax, n_matches}, {dst, capacity, n_chains, launch_cells},
                                          min_seed, max_gap, min_len},
                          stats);
}

int prf_period_chains(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                      uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                      prf_pchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats) {
    return prf_period_chains_ex(c, g, contig, begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, min_len, dst, capacity,
                                n_chains, stats, 0);
}

int prf_period_chains_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1, uint32_t kmin,
                          uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint64_t min_len, prf_pchain *dst,
                          uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats) {
    return list_one_shot("prf_period_chains_seq", c, {seq},
                         pchains_request{{begin, end, pos0, pos1, kmin, kmax, n_matches}, {dst, capacity, n_chains, 0}, min_seed, max_gap,
                                         min_len},
                         stats);
}

}  // extern "C"
