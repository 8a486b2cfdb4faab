// periodicity.cpp -- the host path of the periodicity matrix (prf_period_bits / prf_period_counts and their one-shot forms;
// kernel: periodicity.hip).
//
// One call = one launch over one range of one contig of a resident genome: judge the arguments (before the context or the
// genome is looked at), take the contig's planes, clip `end`, size and zero the output on the device, launch between two
// events, copy the output to the caller.  Nothing of the scans' state is touched: no selection is read, no row sink written,
// the rows of the last scan stay where they are.
#include <cctype>
#include <cstring>

#include "prf_ctx.h"

namespace {

struct per_request {
    u64 begin, end;
    u32 kmin, kmax;
    u64 window;      // 0: the cells themselves (bits)
    void *dst;
    u64 capacity;    // entries (counts) or words (bits) dst holds
    uint64_t *n_out; // receives the windows (counts) or the words (bits) per motif size
    bool bits() const { return window == 0; }
    u64 nk() const { return (u64)kmax - kmin + 1; }
};

// what can be said without a genome; `name` is the entry point
int check_request(const char *name, const per_request &r) {
    int rc = check_params(r.kmin, r.kmax, 1, 1, 0);
    if (rc) return rc;
    if (!r.bits()) {
        const u64 window = r.window;
        if (window < 64 || window % 64) return fail(PRF_EINVAL, "%s: window is %llu. It must be a multiple of 64, at least 64.", name, (unsigned long long)window);
        if (window > (1ull << 31)) return fail(PRF_EINVAL, "%s: window %llu is above 2^31 (a count is 32 bits wide)", name, (unsigned long long)window);
    }
    if (r.begin > r.end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)r.begin, (unsigned long long)r.end);
    if (!r.dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
    if (!r.n_out) return fail(PRF_EINVAL, "%s: NULL size pointer", name);
    return PRF_OK;
}

// what needs the length of the sequence: *per_k = windows or words per motif size of the clipped range
int check_room(const char *name, const per_request &r, u64 seq_len, u64 *len, u64 *per_k) {
    const u64 end = r.end < seq_len ? r.end : seq_len;
    *len = r.begin < end ? end - r.begin : 0;
    if (*len >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "%s: range too large (2^40 positions)", name);
    const u64 unit = r.bits() ? 64 : r.window;
    *per_k = (*len + unit - 1) / unit;
    const u64 total = *per_k * r.nk();
    if (total > r.capacity)
        return fail(PRF_EINVAL, "%s: the destination holds %llu %s, the output has %llu (%llu motif sizes x %llu)", name,
                    (unsigned long long)r.capacity, r.bits() ? "words" : "counts", (unsigned long long)total, (unsigned long long)r.nk(),
                    (unsigned long long)*per_k);
    if (total > PRF_PERIOD_BITS_MAX_WORDS)
        return fail(PRF_EUNSUPPORTED, "%s: an output of %llu %s is above the limit of %llu per call%s", name, (unsigned long long)total,
                    r.bits() ? "words" : "counts", (unsigned long long)PRF_PERIOD_BITS_MAX_WORDS,
                    r.bits() ? " (PRF_PERIOD_BITS_MAX_WORDS): ask for counts, or for fewer motif sizes or positions" : "");
    return PRF_OK;
}

int run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const per_request &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    if ((rc = check_params(r.kmin, r.kmax, 1, 1, v.kmax_hint))) return rc;
    u64 len = 0, per_k = 0;
    if ((rc = check_room(name, r, v.len, &len, &per_k))) return rc;
    if (c->slot[0].seq || c->slot[1].seq) return fail(PRF_EINVAL, "%s: pipelined scans are in flight on this context", name);
    HIPCHK(hipSetDevice(c->dev));
    *r.n_out = per_k;
    const u64 total = per_k * r.nk();
    const size_t bytes = (size_t)total * (r.bits() ? sizeof(u64) : sizeof(u32));
    float ms = 0;
    if (total) {
        dev_array<unsigned char> d_out;
        if ((rc = d_out.alloc(bytes))) return rc;
        prf_periodicity_args a{};
        a.pl = v.planes;
        a.g_begin = v.base + r.begin;
        a.len = len;
        a.n_words = (len + 63) / 64;
        a.kmin = r.kmin;
        a.kmax = r.kmax;
        a.wpw = r.bits() ? 1u : (u32)(r.window / 64);
        a.n_windows = r.bits() ? a.n_words : per_k;
        a.bits = r.bits() ? (u64 *)d_out.p : nullptr;
        a.counts = r.bits() ? nullptr : (u32 *)d_out.p;
        if (!r.bits()) HIPCHK(hipMemsetAsync(d_out.p, 0, bytes, c->stream));
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        HIPCHK(prf_launch_periodicity(c->stream, a, r.bits()));
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(r.dst, d_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->phase1_ms = ms;
        stats->positions = len;
        stats->packed_bytes = (len + 3) / 4;
        stats->n_launches = total ? 1u : 0u;
        stats->path = 4;
    }
    return PRF_OK;
}

int on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const per_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = check_request(name, r);
        return rc ? rc : run(name, c, g, contig, r, stats);
    });
}

// load + call + free; everything that can be refused from the arguments and the bytes is refused before the context is looked at
int one_shot(const char *name, prf_ctx *c, const prf_contig *seq, const per_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = check_request(name, r);
        if (rc) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        u64 len = 0, per_k = 0;
        if ((rc = check_room(name, r, seq->len, &len, &per_k))) return rc;
        for (u64 i = 0; i < seq->len; i++)
            if (!isalpha(seq->ascii[i]) || seq->ascii[i] > 127)
                return fail(PRF_ESYMBOL, "%s: unsupported symbol at position %llu: only letters can be packed", name, (unsigned long long)i);
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, r.kmax, &g))) return rc;
        rc = run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_period_counts(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                      uint64_t window, uint32_t *dst, uint64_t capacity, uint64_t *n_windows, prf_scan_stats *stats) {
    if (!window) return fail(PRF_EINVAL, "prf_period_counts: window is 0. It must be a multiple of 64, at least 64.");
    return on_genome("prf_period_counts", c, g, contig, per_request{begin, end, kmin, kmax, window, dst, capacity, n_windows}, stats);
}

int prf_period_bits(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                    uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_k, prf_scan_stats *stats) {
    return on_genome("prf_period_bits", c, g, contig, per_request{begin, end, kmin, kmax, 0, dst, capacity_words, words_per_k}, stats);
}

int prf_period_counts_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                          uint64_t window, uint32_t *dst, uint64_t capacity, uint64_t *n_windows, prf_scan_stats *stats) {
    if (!window) return fail(PRF_EINVAL, "prf_period_counts_seq: window is 0. It must be a multiple of 64, at least 64.");
    return one_shot("prf_period_counts_seq", c, seq, per_request{begin, end, kmin, kmax, window, dst, capacity, n_windows}, stats);
}

int prf_period_bits_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax, uint64_t *dst,
                        uint64_t capacity_words, uint64_t *words_per_k, prf_scan_stats *stats) {
    return one_shot("prf_period_bits_seq", c, seq, per_request{begin, end, kmin, kmax, 0, dst, capacity_words, words_per_k}, stats);
}

}  // extern "C"
