// dotruns_host.cpp -- the list of diagonal runs of the dot plot of two ranges (prf_dotpair_runs, its _ex and one-shot forms;
// kernels: dotruns.hip) as a request on the frame of list_host.h.  One call = one window of start cells of the
// na x nb rectangle; the runs are the seeds of dotseeds_host.h at min_len, written straight into the output array.
#include "dotseeds_host.h"

namespace {

struct runs_request : pair_window, list_output<prf_dotrun, prf_dotrun_dev> {
    static constexpr u32 path = 7;
    u64 min_len;

    int check(const char *name) const {
        const int rc = check_window(name);
        if (rc) return rc;
        if (!min_len) return fail(PRF_EINVAL, "%s: min_len is 0. It must be at least 1.", name);
        return list_check_output(name, dst, capacity, n_out, "n_runs", PRF_DOTRUN_MAX_ROWS, "PRF_DOTRUN_MAX_ROWS");
    }

    int body(const char *name, prf_ctx *c, const prf_contig_view &v, const room &o, dev_array<prf_dotrun_dev> &d_out, list_result &res) const {
        const prf_dotruns_args a = seeds_args(v, o, *this, min_len);
        dev_array<prf_dotrun_dev> d_long;
        dev_array<u64> d_cnt;
        int rc;
        if ((rc = d_long.alloc(a.long_cap)) || (rc = d_cnt.alloc(PRF_DR_N))) return rc;
        return find_seeds(name, c, a, launch_cells, o, capacity, d_out, d_long, d_cnt.p, &res.n, &res.ms1, &res.launches);
    }
};

}  // namespace

extern "C" {

int prf_dotpair_runs_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                        uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                        uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                        prf_scan_stats *stats, uint64_t launch_cells) {
    return list_on_genome("prf_dotpair_runs", c, g, a_contig,
                          runs_request{{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions},
                                       {dst, capacity, n_runs, launch_cells}, min_len},
                          stats);
}

int prf_dotpair_runs(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                     uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                     uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                     prf_scan_stats *stats) {
    return prf_dotpair_runs_ex(c, g, a_contig, a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions,
                               min_len, dst, capacity, n_runs, stats, 0);
}

int prf_dotpair_runs_seq(prf_ctx *c, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b, uint64_t b_begin,
                         uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                         uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                         prf_scan_stats *stats) {
    return list_one_shot("prf_dotpair_runs_seq", c, {seq_a, seq_b},
                         runs_request{{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, directions},
                                      {dst, capacity, n_runs, 0}, min_len},
                         stats);
}

}  // extern "C"
