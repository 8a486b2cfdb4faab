// periodchain_host.cpp -- the host path of the list of diverged tandem repeats of a range (prf_period_chains, its _ex and one-shot
// forms; kernels: periodchain.hip).  Modelled on dotchain_host.cpp, whose order of refusals it keeps, with the helpers
// of matrix_host.h.  One call = one window of start positions x one range of k:
//   1. the find kernel over the words of the window, cut into launches of at most launch_cells cells: rows, or entries of the
//      long list;
//   2. the long kernel for the first runs and chains the find kernel left, one wave each.
// Both are the stage of periodchain_stage.h, which leaves the rows on the device (periodlink_host.cpp goes on from there).  The
// rows are copied and sorted here.  No selection is read, no row sink written, the last scan's rows stay.
#include <algorithm>
#include <vector>

#include "periodchain_stage.h"

namespace {

struct pchains_request {
    static constexpr u32 path = 10;
    u64 begin, end;
    u64 pos0, pos1;
    u32 kmin, kmax, n_matches;
    u64 min_seed;
    u32 max_gap;
    u64 min_len;
    prf_pchain *dst;
    u64 capacity;
    uint64_t *n_chains;
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
        if (capacity > PRF_PCHAIN_MAX_ROWS)
            return fail(PRF_EUNSUPPORTED, "%s: a capacity of %llu rows is above %llu (PRF_PCHAIN_MAX_ROWS)", name,
                        (unsigned long long)capacity, (unsigned long long)PRF_PCHAIN_MAX_ROWS);
        if (!n_chains) return fail(PRF_EINVAL, "%s: NULL n_chains", name);
        if (!dst && capacity) return fail(PRF_EINVAL, "%s: NULL destination with a capacity of %llu rows", name, (unsigned long long)capacity);
        return PRF_OK;
    }

    int check_room(const char *name, u64 seq_len, room *o) const {
        return pchain_check_room(name, begin, end, pos0, pos1, kmin, kmax, seq_len, o);
    }
};

int pchains_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const pchains_request &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    pchains_request::room o{};
    if ((rc = r.check_room(name, v.len, &o))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    HIPCHK(hipSetDevice(c->dev));
    float ms = 0, ms_long = 0;
    u32 launches = 0;
    u64 cnt[PRF_PC_N] = {0, 0, 0};
    if (pchain_any(o, r.kmin)) {
        const prf_periodchain_args a = pchain_args(v, o, r.begin, r.kmin, r.kmax, r.n_matches, r.min_seed, r.max_gap, r.min_len);
        dev_array<prf_pchain_dev> d_out;
        dev_array<prf_pchain_long> d_long;
        dev_array<u64> d_cnt;
        if ((rc = pchain_rows(name, c, a, r.launch_cells, r.capacity, d_out, d_long, d_cnt, cnt, &ms, &ms_long, &launches))) return rc;
        const u64 n_chains = cnt[PRF_PC_CHAINS];
        if (n_chains && n_chains <= r.capacity) {
            std::vector<prf_pchain> got(n_chains);
            static_assert(sizeof(prf_pchain) == sizeof(prf_pchain_dev), "one layout");
            HIPCHK(hipMemcpy(got.data(), d_out.p, n_chains * sizeof(prf_pchain), hipMemcpyDeviceToHost));
            std::sort(got.begin(), got.end(), [](const prf_pchain &x, const prf_pchain &y) { return x.start != y.start ? x.start < y.start : x.k < y.k; });
            memcpy(r.dst, got.data(), n_chains * sizeof(prf_pchain));
        }
    }
    *r.n_chains = cnt[PRF_PC_CHAINS];
    lane_stats(stats, pchains_request::path, ms + ms_long, o.n, (o.n + 3) / 4, launches);
    if (stats) {
        stats->n_hits = cnt[PRF_PC_CHAINS];
        stats->n_candidates = cnt[PRF_PC_SEEDS];   // the seeds that start in the window
        stats->phase1_ms = ms;
        stats->phase2_ms = ms_long;
    }
    return PRF_OK;
}

int pchains_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const pchains_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = r.check(name);
        return rc ? rc : pchains_run(name, c, g, contig, r, stats);
    });
}

// Everything that can be refused from the arguments and the bytes is refused before the context is looked at.  Nothing behind the
// range is read, so the sequence is loaded with the smallest guard gap.
int pchains_one_shot(const char *name, prf_ctx *c, const prf_contig *seq, const pchains_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        pchains_request::room o{};
        if ((rc = r.check_room(name, seq->len, &o))) return rc;
        if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, 64, &g))) return rc;
        rc = pchains_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_period_chains_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                         uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                         prf_pchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats, uint64_t launch_cells) {
    return pchains_on_genome("prf_period_chains", c, g, contig,
                             pchains_request{begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, min_len, dst, capacity, n_chains,
                                             launch_cells},
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
    return pchains_one_shot("prf_period_chains_seq", c, seq,
                            pchains_request{begin, end, pos0, pos1, kmin, kmax, n_matches, min_seed, max_gap, min_len, dst, capacity, n_chains, 0},
                            stats);
}

}  // extern "C"
