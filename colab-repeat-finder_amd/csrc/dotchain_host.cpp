// dotchain_host.cpp -- the host path of the list of chained diagonal runs of the dot plot of two ranges (prf_dotpair_chains, its
// _ex and one-shot forms; kernels: dotruns.hip for the seeds, dotchain.hip for the chains).  Modelled on
// dotruns_host.cpp, whose order of refusals it keeps, with the helpers of matrix_host.h.  One call = one window of start cells:
//   1. the seeds: the find and long kernels of dotruns.hip at min_len = min_seed into a buffer of this call, cut into launches as
//      dotruns_host.cpp cuts them; 2^20 rows at first, the exact number (up to PRF_DOTCHAIN_MAX_ROWS) if there were more.  The
//      seeds stay on the device.
//   2. the link kernel, one thread per seed: head test, follow, rows or entries of the long list.
//   3. the long kernel for the chains the link kernel left, one wave each.
// The rows are copied and sorted here.  No selection is read, no row sink written, the last scan's rows stay.
#include <algorithm>
#include <vector>

#include "dotseeds_host.h"

namespace {

struct chains_request {
    static constexpr u32 path = 8;
    u64 begin, end;     // A's range
    u32 b_contig;
    u64 b_begin, b_end;
    u32 strand;
    u64 row0, row1, col0, col1;
    u32 directions;
    u64 min_seed;
    u32 max_gap;
    u64 min_len;
    prf_dotchain *dst;
    u64 capacity;
    uint64_t *n_chains;
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS
    using room = seeds_room;

    int check(const char *name) const {
        if (begin > end) return fail(PRF_EINVAL, "%s: a_begin %llu is behind a_end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (b_begin > b_end)
            return fail(PRF_EINVAL, "%s: b_begin %llu is behind b_end %llu", name, (unsigned long long)b_begin, (unsigned long long)b_end);
        if (row0 > row1) return fail(PRF_EINVAL, "%s: row0 %llu is behind row1 %llu", name, (unsigned long long)row0, (unsigned long long)row1);
        if (col0 > col1) return fail(PRF_EINVAL, "%s: col0 %llu is behind col1 %llu", name, (unsigned long long)col0, (unsigned long long)col1);
        if (strand > 1) return fail(PRF_EINVAL, "%s: strand is %u. It must be 0 (plus) or 1 (minus).", name, strand);
        if (!directions || directions > 3)
            return fail(PRF_EINVAL, "%s: directions is %u. It must be 1 (main), 2 (anti) or 3 (both).", name, directions);
        if (!min_seed) return fail(PRF_EINVAL, "%s: min_seed is 0. It must be at least 1.", name);
        if (max_gap > PRF_DOTCHAIN_MAX_GAP)
            return fail(PRF_EUNSUPPORTED, "%s: a max_gap of %u cells is above %u (PRF_DOTCHAIN_MAX_GAP)", name, max_gap, PRF_DOTCHAIN_MAX_GAP);
        if (capacity > PRF_DOTCHAIN_MAX_ROWS)
            return fail(PRF_EUNSUPPORTED, "%s: a capacity of %llu rows is above %llu (PRF_DOTCHAIN_MAX_ROWS)", name,
                        (unsigned long long)capacity, (unsigned long long)PRF_DOTCHAIN_MAX_ROWS);
        if (!n_chains) return fail(PRF_EINVAL, "%s: NULL n_chains", name);
        if (!dst && capacity) return fail(PRF_EINVAL, "%s: NULL destination with a capacity of %llu rows", name, (unsigned long long)capacity);
        return PRF_OK;
    }

    int check_room(const char *name, u64 a_len, room *o) const {
        return seeds_check_room(name, begin, end, b_begin, b_end, row0, row1, col0, col1, a_len, o);
    }
};

int chains_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const chains_request &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v, vb;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = prf_genome_contig_view(g, r.b_contig, &vb))) return rc;
    chains_request::room o{};
    o.b_base = vb.base;
    o.b_len = vb.len;
    if ((rc = r.check_room(name, v.len, &o))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    HIPCHK(hipSetDevice(c->dev));
    float ms = 0, ms_seeds = 0;
    u32 launches = 0;
    u64 n_chains = 0, n_seeds = 0;
    const u64 rows = o.row1 - o.row0, cols = o.col1 - o.col0;
    if (rows && cols) {
        dev_array<prf_dotrun_dev> d_seeds, d_long;
        dev_array<u64> d_cnt;
        const prf_dotruns_args a = seeds_args(v, o, r.begin, r.b_begin, r.strand, r.directions, r.min_seed);
        if ((rc = d_long.alloc(a.long_cap)) || (rc = d_cnt.alloc(PRF_DR_N + PRF_DC_N))) return rc;
        // ---- 1. the seeds
        if ((rc = all_seeds(name, c, a, r.launch_cells, o, d_seeds, d_long, d_cnt.p, &n_seeds, &ms, &launches))) return rc;
        ms_seeds = ms;
        if (n_seeds) {
            // ---- 2. link: every seed is at most one row or one entry of the long list
            dev_array<prf_dotchain_dev> d_out;
            dev_array<prf_dotchain_long> d_clong;
            prf_dotchain_args k{};
            k.seed_rows = d_seeds.p;
            k.n_seeds = n_seeds;
            k.min_seed = r.min_seed;
            k.min_len = r.min_len;
            k.max_gap = r.max_gap;
            k.capacity = r.capacity;
            k.long_cap = n_seeds < PRF_DOTCHAIN_LONG_ROWS ? n_seeds : PRF_DOTCHAIN_LONG_ROWS;
            k.counters = d_cnt.p + PRF_DR_N;
            if ((rc = d_out.alloc(k.capacity)) || (rc = d_clong.alloc(k.long_cap))) return rc;
            k.dst = d_out.p;
            k.longs = d_clong.p;
            float part = 0;
            HIPCHK(hipMemsetAsync(k.counters, 0, PRF_DC_N * sizeof(u64), c->stream));
            HIPCHK(hipEventRecord(c->ev[0], c->stream));
            HIPCHK(prf_launch_dotchain_link(c->stream, a, k));
            ++launches;
            HIPCHK(hipEventRecord(c->ev[1], c->stream));
            u64 cnt[PRF_DC_N] = {0, 0};
            HIPCHK(hipMemcpyAsync(cnt, k.counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipEventElapsedTime(&part, c->ev[0], c->ev[1]));
            ms += part;
            if (cnt[PRF_DC_LONG] > k.long_cap)
                return fail(PRF_EUNSUPPORTED, "%s: %llu chains are still going %u cells (PRF_DOTCHAIN_FOLLOW) behind their first seed, the call keeps room for %llu: ask for smaller windows",
                            name, (unsigned long long)cnt[PRF_DC_LONG], PRF_DOTCHAIN_FOLLOW, (unsigned long long)k.long_cap);
            // ---- 3. the chains the link kernel left
            if (cnt[PRF_DC_LONG]) {
                HIPCHK(hipEventRecord(c->ev[0], c->stream));
                HIPCHK(prf_launch_dotchain_long(c->stream, a, k, cnt[PRF_DC_LONG]));
                ++launches;
                HIPCHK(hipEventRecord(c->ev[1], c->stream));
                HIPCHK(hipMemcpyAsync(cnt, k.counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                HIPCHK(hipEventElapsedTime(&part, c->ev[0], c->ev[1]));
                ms += part;
            }
            n_chains = cnt[PRF_DC_CHAINS];
            if (n_chains && n_chains <= r.capacity) {
                std::vector<prf_dotchain> got(n_chains);
                static_assert(sizeof(prf_dotchain) == sizeof(prf_dotchain_dev), "one layout");
                HIPCHK(hipMemcpy(got.data(), d_out.p, n_chains * sizeof(prf_dotchain), hipMemcpyDeviceToHost));
                std::sort(got.begin(), got.end(), [](const prf_dotchain &x, const prf_dotchain &y) {
                    return x.row != y.row ? x.row < y.row : x.col != y.col ? x.col < y.col : x.dir < y.dir;
                });
                memcpy(r.dst, got.data(), n_chains * sizeof(prf_dotchain));
            }
        }
    }
    *r.n_chains = n_chains;
    lane_stats(stats, chains_request::path, ms, o.na + o.nb, (o.na + o.nb + 3) / 4, launches);
    if (stats) {
        stats->n_hits = n_chains;
        stats->n_candidates = n_seeds;       // the seeds of the window, and the time of their kernels and of the chain kernels
        stats->phase1_ms = ms_seeds;
        stats->phase2_ms = ms - ms_seeds;
    }
    return PRF_OK;
}

int chains_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const chains_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = r.check(name);
        return rc ? rc : chains_run(name, c, g, contig, r, stats);
    });
}

// two sequences become contigs 0 (A) and 1 (B) of a genome that lives for the call, as runs_one_shot (dotruns_host.cpp) loads
// them.  Everything that can be refused from the arguments and the bytes is refused before the context is looked at.
int chains_one_shot(const char *name, prf_ctx *c, const prf_contig *seq_a, const prf_contig *seq_b, const chains_request &r,
                    prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        for (const prf_contig *seq : {seq_a, seq_b})
            if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        chains_request::room o{};
        o.b_len = seq_b->len;
        if ((rc = r.check_room(name, seq_a->len, &o))) return rc;
        if ((rc = matrix_check_letters(name, seq_a)) || (rc = matrix_check_letters(name, seq_b))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        const prf_contig both[2] = {*seq_a, *seq_b};
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, both, 2, 64, &g))) return rc;
        rc = chains_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_dotpair_chains_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                          uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                          uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint64_t min_len, prf_dotchain *dst,
                          uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats, uint64_t launch_cells) {
    return chains_on_genome("prf_dotpair_chains", c, g, a_contig,
                            chains_request{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, directions, min_seed,
                                           max_gap, min_len, dst, capacity, n_chains, launch_cells},
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
    return chains_one_shot("prf_dotpair_chains_seq", c, seq_a, seq_b,
                           chains_request{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, directions, min_seed, max_gap,
                                          min_len, dst, capacity, n_chains, 0},
                           stats);
}

}  // extern "C"
