// prf_ctx.h -- what the host translation units of libprf that talk to the device (context.cpp, genome.cpp, scan_host.cpp,
// literal_host.cpp, handoff.cpp, interrupted.cpp, periodicity_host.cpp, dotplot_host.cpp) share and nobody else sees: the context, error reporting, the C-boundary guard, parameter checks, a scoped
// device array, the refusal while pipelined scans are in flight, the stats of a lane that waits for its own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../../include/prf.h"
#include "prf_host.h"

// Sets the calling thread's error text (prf_last_error) and returns `code`.  Defined in context.cpp; fasta_io.cpp reports through it too.
int prf_set_error(int code, const char *fmt, ...);
static constexpr auto &fail = prf_set_error;

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? PRF_ENOMEM : PRF_EHIP, "%s failed: %s (%s:%d)", #expr,    \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                           \
    } while (0)

// The C boundary: no exception leaves the library
template <class F>
static int guarded(const char *name, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(PRF_ENOMEM, "%s: out of host memory", name);
    } catch (...) {
        return fail(PRF_EHIP, "%s: unexpected exception", name);
    }
}

// Same conditions, same wording as the reference's ValueErrors (perfect_repeat_finder.py:23-30), then the library's limits:
// the motif sizes a resident genome was packed for (kmax_hint), or the 60000 of the lanes that take sequences (kmax_hint 0).
static int check_params(u32 kmin, u32 kmax, u32 min_repeats, u32 min_span, u32 kmax_hint) {
    if (kmin < 1) return fail(PRF_EINVAL, "min_motif_size is set to %u. It must be at least 1.", kmin);
    if (kmax < kmin) return fail(PRF_EINVAL, "max_motif_size is set to %u. It must be at least min_motif_size.", kmax);
    if (min_repeats < 1) return fail(PRF_EINVAL, "min_repeats is set to %u. It must be at least 1.", min_repeats);
    if (min_span < 1) return fail(PRF_EINVAL, "min_span is set to %u. It must be at least 1.", min_span);
    if (min_repeats > 1000000u || min_span > (1u << 30)) return fail(PRF_EINVAL, "threshold out of range");
    if (kmax_hint && kmax > kmax_hint)
        return fail(PRF_EUNSUPPORTED, "max_motif_size %u exceeds the kmax_hint %u this genome was packed with", kmax, kmax_hint);
    if (kmax > 60000) return fail(PRF_EUNSUPPORTED, "max_motif_size %u > 60000", kmax);
    return PRF_OK;
}

// One contig of a resident genome as the matrix products see it (the genome's own struct, genome.h, stays private to the scan's host files)
struct prf_contig_view {
    prf_ctx *ctx;
    prf_planes planes;  // linear planes; at least kmax_hint / 64 + 8 readable words behind them
    u64 base, len;      // first global position, positions
    u32 kmax_hint;
};
__attribute__((visibility("hidden"))) int prf_genome_contig_view(const prf_genome *g, u32 contig, prf_contig_view *out);

// A device array that lives as long as its scope.  alloc(0) still allocates, so that p is always an address a copy of nothing
// or a kernel over nothing may be given; what the array held before is freed, not kept.
template <class T>
struct dev_array {
    T *p = nullptr;
    dev_array() = default;
    dev_array(const dev_array &) = delete;
    dev_array &operator=(const dev_array &) = delete;
    ~dev_array() { (void)hipFree(p); }
    int alloc(size_t n) {
        (void)hipFree(p);
        p = nullptr;
        HIPCHK(hipMalloc((void **)&p, n ? n * sizeof(T) : 16));
        return PRF_OK;
    }
};

// A pinned host counter block (h_counters, h_async): PRF_CNT_N counters, then the scan's serial number in the word at PRF_CNT_N
static const u64 PRF_CNT_BLOCK_WORDS = PRF_CNT_N + 8;  // words of a block
static const u64 PRF_CNT_SPARE = PRF_CNT_N + 2;        // first of its spare words: staging for small copies to and from the device

struct prf_ctx {
    int dev = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {};  // timing events of the paths that wait for their kernels; each path names the ones it uses
    // fused path: one event pair per scan, in a ring, so that the kernel times of the last PRF_TIMING_RING scans can
    // be read after a timing loop (prf_scan_timings) instead of waiting for the events inside every scan
    hipEvent_t ring[3 * PRF_TIMING_RING] = {};  // per scan: before the scan kernel, between the two kernels, after the gather
    u64 *d_counters = nullptr;   // generic path + packer
    u64 *h_counters = nullptr;   // pinned, device-mapped: the fused path's last kernel writes the counters here
    u64 *h_counters_dev = nullptr;  // device address of h_counters
    u64 *d_vcounters = nullptr;  // fused path: two counter blocks used alternately (the idle one is cleared on the device)
    u64 *d_side_cnt = nullptr;   // pipelined wire hand-off: long rows packed so far (zero between packs)
    void *lit_scratch = nullptr;  // the literal lane's sort scratch (scan_literal.hip::prf_lit_sort_unique): kept between calls
    size_t lit_scratch_bytes = 0;
    hipEvent_t ev_handoff = nullptr;  // prf_stream_wait_for
    u32 parity = 0;
    u64 scan_seq = 0;
    // generic path scratch
    u64 *d_cand = nullptr;
    u64 cand_cap = 0;
    prf_hit_dev *d_hits = nullptr;  // flat rows: generic path output, or the compacted rows of the fused path
    u64 hit_cap = 0;
    prf_hit_dev *sink = nullptr;    // caller-owned device array the rows go to instead (prf_set_row_sink)
    u64 sink_cap = 0;
    struct last_scan {              // where the rows of the last scan are
        const prf_hit_dev *rows = nullptr;
        u64 nhits = 0;
        u32 kmax = 0;               // its largest motif size (the 8-byte wire rows hold 9 bits)
    } last;
    // pipelined scans (prf_scan_genome_async / prf_scan_wait): two slots used alternately, each with its own host
    // counter block and row array; slot 0 shares them with the synchronous path
    struct async_slot {
        u64 seq = 0;            // scan in this slot (0: free)
        u64 *h = nullptr;       // mapped host counter block (+ serial number word)
        u64 *h_dev = nullptr;
        prf_hit_dev *rows = nullptr;
        u64 positions = 0;
        u32 tiles = 0;
        u32 kmax = 0;
    } slot[2];
    u64 async_n = 0;
    u64 *h_async = nullptr;         // slot 1's counter block
    prf_hit_dev *d_hits_async = nullptr;
    u64 hit_cap_async = 0;
    // fused (bit-sliced) path scratch: one row slab and one row count per launch slot (= scanned tile)
    u64 *d_slabs = nullptr;         // 8-byte rows (scan_vertical.h)
    u64 *d_long_ends = nullptr;     // per launch slot: true ends of the rows whose span is clipped in the 8-byte form
    u32 *d_slab_count = nullptr;
    u32 *d_block_sum = nullptr;     // rows per PRF_GATHER_SLOTS launch slots; zero between scans (the gather clears it)
    u64 slab_slots = 0;
    u32 slab_cap = 0;
    u64 *stamps_buf = nullptr;      // diagnostic (PRF_STAMPS) builds only
    u32 stamps_n = 0;
};

// What every lane that uses the stream synchronously refuses: a pipelined scan holds a slot until prf_scan_wait.  `name` is the entry point.
static int refuse_in_flight(const prf_ctx *c, const char *name) {
    if (c->slot[0].seq || c->slot[1].seq) return fail(PRF_EINVAL, "%s: pipelined scans are in flight on this context", name);
    return PRF_OK;
}

// The stats of a lane that waits for its own kernels (`stats` may be NULL): one phase, no candidates or rows unless the caller adds them
static void lane_stats(prf_scan_stats *stats, u32 path, float ms, u64 positions, u64 packed_bytes, u32 launches) {
    if (!stats) return;
    memset(stats, 0, sizeof *stats);
    stats->scan_ms = stats->phase1_ms = ms;
    stats->positions = positions;
    stats->packed_bytes = packed_bytes;
    stats->n_launches = launches;
    stats->path = path;
}
