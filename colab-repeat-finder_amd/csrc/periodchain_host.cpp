// periodchain_host.cpp -- the host path of the list of diverged tandem repeats of a range (prf_period_chains, its _ex and one-shot
// forms; kernels: periodchain.hip).  Modelled on dotchain_host.cpp, whose order of refusals it keeps, with the helpers
// of matrix_host.h.  One call = one window of start positions x one range of k:
//   1. the find kernel over the words of the window, cut into launches of at most launch_cells cells: rows, or entries of the
//      long list;
//   2. the long kernel for the first runs and chains the find kernel left, one wave each.
// The rows are copied and sorted here.  No selection is read, no row sink written, the last scan's rows stay.
#include <algorithm>
#include <vector>

#include "matrix_host.h"

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
    struct room {
        u64 n;              // positions of the clipped range
        u64 pos0, pos1;     // the clipped window
    };

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
        const int rc = matrix_clip(name, begin, end, seq_len, &o->n);
        if (rc) return rc;
        o->pos1 = pos1 < o->n ? pos1 : o->n;
        o->pos0 = pos0 < o->pos1 ? pos0 : o->pos1;
        const u64 starts = o->pos1 - o->pos0, nk = (u64)kmax - kmin + 1;
        if (starts && nk > PRF_DOT_MAX_CELLS / starts)
            return fail(PRF_EUNSUPPORTED, "%s: a window of %llu positions x %llu lines is above the limit of 2^42 cells per call (PRF_DOT_MAX_CELLS)",
                        name, (unsigned long long)starts, (unsigned long long)nk);
        return PRF_OK;
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
    const u64 starts = o.pos1 - o.pos0;
    if (starts && (u64)r.kmin < o.n) {                         // a line k >= n is empty
        prf_periodchain_args a{};
        a.pl = v.planes;
        a.g_begin = v.base + r.begin;
        a.n = o.n;
        a.n_words = (o.n + 63) / 64;
        a.pos0 = o.pos0;
        a.pos1 = o.pos1;
        a.kmin = r.kmin;
        a.kmax = (u64)r.kmax < o.n ? r.kmax : (u32)(o.n - 1);
        a.n_matches = r.n_matches;
        a.max_gap = r.max_gap;
        a.min_seed = r.min_seed;
        a.min_len = r.min_len;
        a.capacity = r.capacity;
        const u64 nk = (u64)a.kmax - a.kmin + 1;
        // two heads of one line lie more than PRF_DOTCHAIN_FOLLOW cells apart if the first one is still going there
        const u64 most_long = nk * (starts / PRF_DOTCHAIN_FOLLOW + 2);
        a.long_cap = most_long < PRF_PCHAIN_LONG_ROWS ? most_long : PRF_PCHAIN_LONG_ROWS;
        dev_array<prf_pchain_dev> d_out;
        dev_array<prf_pchain_long> d_long;
        dev_array<u64> d_cnt;
        if ((rc = d_out.alloc(a.capacity)) || (rc = d_long.alloc(a.long_cap)) || (rc = d_cnt.alloc(PRF_PC_N))) return rc;
        a.dst = d_out.p;
        a.longs = d_long.p;
        a.counters = d_cnt.p;
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, PRF_PC_N * sizeof(u64), c->stream));
        // ---- 1. the words of the window, whole spans per launch
        u32 span_words, kslice, stride;
        prf_periodchain_shape(a.pl.E[0] != nullptr, &span_words, &kslice, &stride);
        const u64 cells = r.launch_cells ? r.launch_cells : PRF_DOT_LAUNCH_CELLS;
        u64 spans = cells / nk / 64 / span_words;
        if (spans < 1) spans = 1;
        if (spans > (1ull << 30)) spans = 1ull << 30;
        const u64 w_end = (o.pos1 + 63) / 64;
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        for (u64 w = o.pos0 / 64; w < w_end; w += spans * span_words) {
            a.word0 = w;
            a.word1 = w_end - w > spans * span_words ? w + spans * span_words : w_end;
            HIPCHK(prf_launch_periodchain_find(c->stream, a));
            ++launches;
        }
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        if (cnt[PRF_PC_LONG] > a.long_cap)
            return fail(PRF_EUNSUPPORTED, "%s: %llu runs and chains are still going %u cells (PRF_DOTCHAIN_FOLLOW) behind their start, the call keeps room for %llu: ask for a smaller window",
                        name, (unsigned long long)cnt[PRF_PC_LONG], PRF_DOTCHAIN_FOLLOW, (unsigned long long)a.long_cap);
        // ---- 2. what the find kernel left
        if (cnt[PRF_PC_LONG]) {
            HIPCHK(hipEventRecord(c->ev[0], c->stream));
            HIPCHK(prf_launch_periodchain_long(c->stream, a, cnt[PRF_PC_LONG]));
            ++launches;
            HIPCHK(hipEventRecord(c->ev[1], c->stream));
            HIPCHK(hipMemcpyAsync(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipEventElapsedTime(&ms_long, c->ev[0], c->ev[1]));
        }
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
