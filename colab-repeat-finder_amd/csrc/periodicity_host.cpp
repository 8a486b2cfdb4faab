// periodicity_host.cpp -- the periodicity matrix's part of the host path (prf_period_bits / prf_period_counts and their one-shot
// forms; kernel: periodicity.hip).  The path itself is matrix_host.h; one call = one launch.
#include "matrix_host.h"

namespace {

struct per_request {
    static constexpr u32 path = 4;
    u64 begin, end;
    u32 kmin, kmax;
    u64 window;      // 0: the cells themselves (bits)
    void *dst;
    u64 capacity;    // entries (counts) or words (bits) dst holds
    uint64_t *n_out; // receives the windows (counts) or the words (bits) per motif size
    struct room {
        u64 n, per_k, nk;   // positions of the clipped range; windows or words per motif size; motif sizes
        u64 total() const { return per_k * nk; }
    };
    bool bits() const { return window == 0; }
    u32 load_kmax() const { return kmax; }
    void publish(const room &o) const { *n_out = o.per_k; }
    int check_view(const char *, const prf_genome *, const prf_contig_view &v, room *) const { return check_params(kmin, kmax, 1, 1, v.kmax_hint); }

    int check(const char *name) const {
        int rc = check_params(kmin, kmax, 1, 1, 0);
        if (rc) return rc;
        if (!bits()) {
            if (window < 64 || window % 64) return fail(PRF_EINVAL, "%s: window is %llu. It must be a multiple of 64, at least 64.", name, (unsigned long long)window);
            if (window > (1ull << 31)) return fail(PRF_EINVAL, "%s: window %llu is above 2^31 (a count is 32 bits wide)", name, (unsigned long long)window);
        }
        if (begin > end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        if (!n_out) return fail(PRF_EINVAL, "%s: NULL size pointer", name);
        return PRF_OK;
    }

    int check_room(const char *name, u64 seq_len, room *o) const {
        const int rc = matrix_clip(name, begin, end, seq_len, &o->n);
        if (rc) return rc;
        const u64 unit = bits() ? 64 : window;
        o->per_k = (o->n + unit - 1) / unit;
        o->nk = (u64)kmax - kmin + 1;
        return matrix_check_output(name, bits(), capacity, o->nk, " motif sizes", o->per_k,
                                   bits() ? " (PRF_PERIOD_BITS_MAX_WORDS): ask for counts, or for fewer motif sizes or positions" : "");
    }

    int launch(hipStream_t stream, const prf_contig_view &v, const room &o, void *d_out, u32 *launches) const {
        prf_periodicity_args a{};
        a.pl = v.planes;
        a.g_begin = v.base + begin;
        a.len = o.n;
        a.n_words = (o.n + 63) / 64;
        a.kmin = kmin;
        a.kmax = kmax;
        a.wpw = bits() ? 1u : (u32)(window / 64);
        a.n_windows = bits() ? a.n_words : o.per_k;
        a.bits = bits() ? (u64 *)d_out : nullptr;
        a.counts = bits() ? nullptr : (u32 *)d_out;
        HIPCHK(prf_launch_periodicity(stream, a, bits()));
        *launches = 1;
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_period_counts(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                      uint64_t window, uint32_t *dst, uint64_t capacity, uint64_t *n_windows, prf_scan_stats *stats) {
    if (!window) return fail(PRF_EINVAL, "prf_period_counts: window is 0. It must be a multiple of 64, at least 64.");
    return matrix_on_genome("prf_period_counts", c, g, contig, per_request{begin, end, kmin, kmax, window, dst, capacity, n_windows}, stats);
}

int prf_period_bits(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                    uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_k, prf_scan_stats *stats) {
    return matrix_on_genome("prf_period_bits", c, g, contig, per_request{begin, end, kmin, kmax, 0, dst, capacity_words, words_per_k}, stats);
}

int prf_period_counts_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                          uint64_t window, uint32_t *dst, uint64_t capacity, uint64_t *n_windows, prf_scan_stats *stats) {
    if (!window) return fail(PRF_EINVAL, "prf_period_counts_seq: window is 0. It must be a multiple of 64, at least 64.");
    return matrix_one_shot("prf_period_counts_seq", c, seq, per_request{begin, end, kmin, kmax, window, dst, capacity, n_windows}, stats);
}

int prf_period_bits_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax, uint64_t *dst,
                        uint64_t capacity_words, uint64_t *words_per_k, prf_scan_stats *stats) {
    return matrix_one_shot("prf_period_bits_seq", c, seq, per_request{begin, end, kmin, kmax, 0, dst, capacity_words, words_per_k}, stats);
}

}  // extern "C"
