// scan_host.cpp -- the perfect scan on the host: its passes (fused_pass, exotic_pass, generic_pass under run_passes) with the
// buffers they grow, and the pipelined scans.  The whole path of a fused scan, from the entry points down to launch_fused and
// wait_for_seq, is in this one file: its calls are the host's share of a scan.
//
// Host-side shape of one perfect scan (what replaces the body of the reference's detect_repeats(),
// perfect_repeat_finder.py:33-81):
//   fused path (kmax <= 480): two launches -- the scan kernel (persistent workgroups: scan + verify + the rows of every
//   tile sorted into its slab) and the row gather (slabs -> ONE array sorted by (contig, start, end), as the reference
//   sorts its dict, :81; its last workgroup posts the counters to mapped host memory, where the host polls the scan's
//   serial number).  Generic path (any k): memset counters -> candidate kernel -> verify kernel -> copy back two
//   counters -> host sort.  Either way: grow buffers and repeat on overflow, then copy the rows back.
// Everything runs on the context's own HIP stream; timings are HIP events on that stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "genome.h"

// A device array of at least `want` elements; a smaller one is replaced (its contents are not kept)
template <class T>
static int grow(T *&p, u64 &cap, u64 want) {
    if (want <= cap) return PRF_OK;
    (void)hipFree(p);
    p = nullptr;
    cap = 0;
    HIPCHK(hipMalloc((void **)&p, want * sizeof(T)));
    cap = want;
    return PRF_OK;
}

// what a buffer that held too few of n elements grows to
static u64 with_headroom(u64 n) { return n + n / 8 + 1024; }

extern "C" {

// words of d_block_sum for nslots launch slots: per 8 slots, then two words per PRF_GATHER_SUPER gather workgroups
static size_t block_sum_words(u64 nslots) { return (size_t)(nslots / 8 + 1) + 2 * (size_t)(nslots / (8 * PRF_GATHER_SUPER) + 2); }

// After a fused launch failed or never posted its counters the device-side counter blocks are in an unknown state
// (the kernel clears the NEXT scan's block only when its last workgroup gets there): drain the stream, clear both.
static void reset_vcounters(prf_ctx *c) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemsetAsync(c->d_vcounters, 0, 2 * PRF_CNT_N * sizeof(u64), c->stream);
    if (c->d_block_sum) (void)hipMemsetAsync(c->d_block_sum, 0, block_sum_words(c->slab_slots) * sizeof(u32), c->stream);
    (void)hipStreamSynchronize(c->stream);
}

// Poll the serial number the fused kernel's last workgroup writes behind the counter block (mapped host memory).
// Bounded by the wall clock (PRF_SCAN_TIMEOUT_S, default 120 s): a wedged kernel becomes PRF_EHIP, not a wedged host.
static int wait_for_seq(prf_ctx *c, u64 seq, const u64 *block = nullptr) {
    const u64 *seqp = (block ? block : c->h_counters) + PRF_CNT_N;
    static const double limit_s = [] {
        const char *e = getenv("PRF_SCAN_TIMEOUT_S");
        const double v = e ? atof(e) : 0.0;
        return v > 0.0 ? v : 120.0;
    }();
    std::chrono::steady_clock::time_point t0;
    bool timing = false;
    for (u64 spins = 1;; spins++) {
        if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == seq) return PRF_OK;
        __builtin_ia32_pause();
        if ((spins & 0xFFFFu) == 0) {  // every ~millisecond: is the stream still alive?
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) {
                if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == seq) return PRF_OK;
                reset_vcounters(c);
                return fail(PRF_EHIP, "fused scan kernel finished without posting its counters (scan %llu)", (unsigned long long)seq);
            }
            if (e != hipErrorNotReady) {
                reset_vcounters(c);
                return fail(PRF_EHIP, "fused scan kernel failed: %s", hipGetErrorString(e));
            }
            if (!timing) {
                t0 = std::chrono::steady_clock::now();
                timing = true;
            } else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) {
                // the device-side blocks are not touched: the kernel may still be running
                return fail(PRF_EHIP, "fused scan %llu did not post its counters within %.0f s (PRF_SCAN_TIMEOUT_S)",
                            (unsigned long long)seq, limit_s);
            }
        }
    }
}

// the timing events of fused scan `seq`: before the scan kernel, between the two kernels, after the gather
static hipEvent_t *ring_events(prf_ctx *c, u64 seq) { return &c->ring[3 * (seq % PRF_TIMING_RING)]; }

static int scan_timings_impl(prf_ctx *c, uint64_t first_seq, uint32_t n, float *total_ms, float *scan_ms, float *gather_ms) {
    if (!c || first_seq == 0 || first_seq + n - 1 > c->scan_seq || c->scan_seq - first_seq >= PRF_TIMING_RING)
        return fail(PRF_EINVAL, "prf_scan_timings: scans %llu..%llu are not among the last %d fused scans of this context",
                    (unsigned long long)first_seq, (unsigned long long)(first_seq + n - 1), PRF_TIMING_RING);
    HIPCHK(hipSetDevice(c->dev));
    for (uint32_t i = 0; i < n; i++) {
        const hipEvent_t *ev = ring_events(c, first_seq + i);
        HIPCHK(hipEventSynchronize(ev[2]));
        if (total_ms) HIPCHK(hipEventElapsedTime(&total_ms[i], ev[0], ev[2]));
        if (scan_ms) HIPCHK(hipEventElapsedTime(&scan_ms[i], ev[0], ev[1]));
        if (gather_ms) HIPCHK(hipEventElapsedTime(&gather_ms[i], ev[1], ev[2]));
    }
    return PRF_OK;
}

int prf_scan_timings(prf_ctx *c, uint64_t first_seq, uint32_t n, float *kernel_ms) {
    if (!c || (n && !kernel_ms)) return fail(PRF_EINVAL, "prf_scan_timings: bad arguments");
    return scan_timings_impl(c, first_seq, n, kernel_ms, nullptr, nullptr);
}

int prf_scan_timings_split(prf_ctx *c, uint64_t first_seq, uint32_t n, float *scan_ms, float *gather_ms) {
    if (!c || (n && (!scan_ms || !gather_ms))) return fail(PRF_EINVAL, "prf_scan_timings_split: bad arguments");
    return scan_timings_impl(c, first_seq, n, nullptr, scan_ms, gather_ms);
}

static int ensure_buffers(prf_ctx *c, u64 want_cand, u64 want_hits) {
    const int rc = grow(c->d_cand, c->cand_cap, want_cand);
    return rc ? rc : grow(c->d_hits, c->hit_cap, want_hits);
}

static int ensure_slabs(prf_ctx *c, u64 nslots, u32 cap) {
    if (nslots <= c->slab_slots && cap <= c->slab_cap) return PRF_OK;
    nslots = std::max<u64>(nslots, c->slab_slots);
    cap = std::max<u32>(cap, c->slab_cap);
    HIPCHK(hipStreamSynchronize(c->stream));  // no scan in flight may still use the old buffers
    for (void *p : {(void *)c->d_slabs, (void *)c->d_long_ends, (void *)c->d_slab_count, (void *)c->d_block_sum}) (void)hipFree(p);
    c->d_slabs = c->d_long_ends = nullptr;
    c->d_slab_count = c->d_block_sum = nullptr;
    c->slab_slots = c->slab_cap = 0;
    const size_t n_blocks = block_sum_words(nslots);
    HIPCHK(hipMalloc((void **)&c->d_slabs, nslots * (u64)cap * sizeof(u64)));
    HIPCHK(hipMalloc((void **)&c->d_long_ends, nslots * (u64)PRF_LONG_PER_TILE * sizeof(u64)));
    HIPCHK(hipMalloc((void **)&c->d_slab_count, nslots * sizeof(u32)));
    HIPCHK(hipMalloc((void **)&c->d_block_sum, n_blocks * sizeof(u32)));
    HIPCHK(hipMemset(c->d_block_sum, 0, n_blocks * sizeof(u32)));
    c->slab_slots = nslots;
    c->slab_cap = cap;
    return PRF_OK;
}

// The two launches of a fused scan: tiles -> sorted slabs, slabs -> one compact sorted array + counters to the host.
// HIP events bracket the pair.
static int launch_fused(prf_ctx *c, const prf_genome *g, const prf_vplan &plan, const scan_params &p, prf_hit_dev *rows, u64 rows_cap,
                        u32 count_row, u64 *host_counters_dev, u64 *seq_out) {
    const launch_view lv = active_launch(g);
    prf_vscan_args a;
    a.VH = g->vp.VH; a.VL = g->vp.VL;
    a.H = g->H; a.L = g->L; a.X = g->X;
    a.E = g->d_E;
    a.launch_list = lv.list; a.n_launch = lv.n; a.flat_base = lv.flat;
    a.slabs = c->d_slabs; a.long_ends = c->d_long_ends; a.slab_count = c->d_slab_count; a.block_sum = c->d_block_sum; a.slab_cap = c->slab_cap;
    // the gather takes 8 launch slots per workgroup on small launches (more workgroups in flight), 64 on large ones
    a.gather_shift = lv.n <= 8192u ? 3u : 5u;
#ifdef PRF_DIAG
    {   // PRF_GATHER_SHIFT: launch slots per gather workgroup = 1 << shift, 3 .. 6
        static const int gs_env = getenv("PRF_GATHER_SHIFT") ? atoi(getenv("PRF_GATHER_SHIFT")) : -1;
        if (gs_env >= 3 && gs_env <= 6) a.gather_shift = (u32)gs_env;
    }
    {   // PRF_SKIP: phases left out to time the others (wrong rows, timing only)
        static const u32 skip_env = getenv("PRF_SKIP") ? (u32)strtoul(getenv("PRF_SKIP"), nullptr, 0) : 0u;
        a.skip = skip_env;
    }
#endif
    a.super_off = (lv.n + (1u << a.gather_shift) - 1u) >> a.gather_shift;  // the gather's grid
    a.min_repeats = p.min_repeats; a.min_span = p.min_span;
    a.tile_info = g->d_tile_info;
    a.counters = c->d_vcounters + (size_t)c->parity * PRF_CNT_N;
    a.dbg = nullptr;
#ifdef PRF_STAMPS
    {
        static u64 *dbg_buf = nullptr;
        const size_t nu = (size_t)(1u << 18) * PRF_VMAX_WAVES * PRF_STAMP_SLOTS;  // up to 262144 tiles
        if (!dbg_buf) HIPCHK(hipMalloc((void **)&dbg_buf, nu * sizeof(u64)));
        if (lv.n <= (1u << 18)) {
            HIPCHK(hipMemsetAsync(dbg_buf, 0, (size_t)lv.n * PRF_VMAX_WAVES * PRF_STAMP_SLOTS * sizeof(u64), c->stream));
            a.dbg = dbg_buf;
            c->stamps_buf = dbg_buf;
            c->stamps_n = lv.n;
        }
    }
#endif
    a.plan = plan;
    prf_vgather_args ga;
    ga.slabs = c->d_slabs; ga.long_ends = c->d_long_ends; ga.launch_list = lv.list; ga.flat_base = lv.flat; ga.tile_info = g->d_tile_info;
    ga.slab_count = c->d_slab_count; ga.block_sum = c->d_block_sum; ga.slab_cap = c->slab_cap; ga.n_launch = lv.n;
    ga.super_off = a.super_off;
    ga.gather_shift = a.gather_shift;
    ga.rows = rows; ga.rows_cap = rows_cap; ga.count_row = count_row;
    ga.counters = a.counters;
    ga.host_counters = host_counters_dev;
    ga.seq = ++c->scan_seq;
    ga.next_counters = c->d_vcounters + (size_t)(c->parity ^ 1u) * PRF_CNT_N;
    c->parity ^= 1u;
    const hipEvent_t *ev = ring_events(c, ga.seq);
    HIPCHK(hipEventRecord(ev[0], c->stream));
    hipError_t le = prf_vertical_launch(c->stream, a);
    if (le == hipSuccess) le = hipEventRecord(ev[1], c->stream);
    if (le == hipSuccess) le = prf_vertical_gather(c->stream, ga);
    if (le != hipSuccess) {
        reset_vcounters(c);
        return fail(PRF_EHIP, "fused scan launch failed: %s", hipGetErrorString(le));
    }
    HIPCHK(hipEventRecord(ev[2], c->stream));
    *seq_out = ga.seq;
    return PRF_OK;
}

// where the rows of a scan go: the caller's row sink, or the context's own array
struct row_dest {
    prf_hit_dev *rows;
    u64 cap;
    bool is_sink;
};
static row_dest row_destination(const prf_ctx *c) {
    return c->sink ? row_dest{c->sink, c->sink_cap, true} : row_dest{c->d_hits, c->hit_cap, false};
}

// the buffer sizes a scan asks for; a pass that overflowed raises them and the scan runs again
struct buffer_sizes {
    u64 cand, hits;
    u32 slab_cap;
};

// what the passes of one scan attempt found
struct pass_result {
    u64 ncand = 0, nhits = 0;
    u32 launches = 0;
    bool sorted = true;  // the rows are sorted by (contig, start, end) on the device
    float ms01 = 0, ms12 = 0;
    bool again = false;  // a buffer was too small (buffer_sizes raised): scan again
};

static int sink_too_small(const prf_ctx *c, u64 nhits) {
    return fail(PRF_EINVAL, "the row sink holds %llu rows, the scan found %llu", (unsigned long long)c->sink_cap,
                (unsigned long long)nhits);
}

// one word (PRF_SH_CAND, PRF_SH_EARLY) summed over the shards of a fused scan's counter block
static u64 shard_sum(const u64 *h, int word) {
    u64 s = 0;
    for (int sh = 0; sh < PRF_CNT_NSHARD; sh++) s += h[PRF_CNT_SHARD0 + sh * PRF_CNT_SHARD_STRIDE + word];
    return s;
}

// what a fused scan (one scan kernel + one gather) posted in its host counter block
static pass_result read_fused(const u64 *h) {
    pass_result r;
    r.nhits = h[PRF_CNT_ROWS];
    r.sorted = h[PRF_CNT_UNSORTED] == 0;
    r.ncand = shard_sum(h, PRF_SH_CAND);
    r.launches = 2;
    return r;
}

static void fill_stats(prf_scan_stats *s, const pass_result &r, u32 path, u64 positions, u32 tiles, u64 seq) {
    memset(s, 0, sizeof *s);
    s->phase1_ms = r.ms01;
    s->phase2_ms = r.ms12;
    s->scan_ms = (double)r.ms01 + (double)r.ms12;
    s->positions = positions;
    s->packed_bytes = (positions + 3) / 4;
    s->n_candidates = r.ncand;
    s->n_hits = r.nhits;
    s->n_launches = r.launches;
    s->path = path;
    s->seq = seq;
    s->sorted_on_device = r.sorted ? 1u : 0u;
    s->tiles_launched = tiles;
}

#ifdef PRF_STAMPS
static int dump_stamps(prf_ctx *c, const prf_vplan &plan) {
    const char *path = getenv("PRF_STAMPS_OUT");
    if (!path) return PRF_OK;
    fprintf(stderr, "[prf] plan: %u waves, %u tasks\n", plan.n_waves, plan.n_tasks);
    for (u32 w = 0; w < plan.n_waves; w++)
        for (u32 ti = plan.wave_begin[w]; ti < plan.wave_begin[w + 1]; ti++)
            fprintf(stderr, "[prf]   wave %u slot %u: kind %u k0 %u valid %02x stride %u\n", w, ti - plan.wave_begin[w],
                    plan.tasks[ti].kind, plan.tasks[ti].k0, plan.tasks[ti].valid, plan.tasks[ti].stride);
    if (c->stamps_buf) {
        HIPCHK(hipStreamSynchronize(c->stream));
        const size_t nu = (size_t)c->stamps_n * PRF_VMAX_WAVES * PRF_STAMP_SLOTS;
        std::vector<u64> host(nu);
        HIPCHK(hipMemcpy(host.data(), c->stamps_buf, nu * sizeof(u64), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(path, "wb")) { fwrite(host.data(), 8, nu, f); fclose(f); }
    }
    return PRF_OK;
}
#endif

// ---- fused bit-sliced kernel (scan + verify + sorted rows per tile), then the row gather into dst ----
// Tiles with a symbol outside ACGTN in reach are not on the launch list: exotic_pass takes them.
static int fused_pass(prf_ctx *c, const prf_genome *g, const prf_vplan &plan, const scan_params &p, const row_dest &dst, bool timed,
                      buffer_sizes *want, pass_result *r) {
    u64 seq = 0;
    int rc = launch_fused(c, g, plan, p, dst.rows, dst.cap, dst.is_sink ? 1u : 0u, c->h_counters_dev, &seq);
    if (rc) return rc;
    // The scan is over for the host when the gather's last workgroup has posted the counter block and this scan's serial
    // number in mapped host memory: poll that word instead of waiting for the stream to drain (the kernel's end-of-grid
    // handshake, the event and the wake-up cost ~5 us).  Everything that consumes the rows is enqueued on the same stream,
    // hence ordered after the kernels.
    rc = wait_for_seq(c, seq);
    if (rc) return rc;
#ifdef PRF_STAMPS
    rc = dump_stamps(c, plan);
    if (rc) return rc;
#endif
    // a row sink is read by the caller on streams of its own: wait until every workgroup has copied its rows
    if (dst.is_sink) HIPCHK(hipStreamSynchronize(c->stream));
    const u64 *h = c->h_counters;
    *r = read_fused(h);
    if (timed) {
        const hipEvent_t *ev = ring_events(c, seq);
        HIPCHK(hipEventSynchronize(ev[2]));
        HIPCHK(hipEventElapsedTime(&r->ms01, ev[0], ev[2]));
    }
#ifdef PRF_DIAG
    if (getenv("PRF_DEBUG"))
        fprintf(stderr, "[prf] fused: hits %llu cand-records %llu (verified on the spot, a list being full: %llu) hit_ovf %llu unsorted %llu ms %.4f\n",
                (unsigned long long)r->nhits, (unsigned long long)r->ncand, (unsigned long long)shard_sum(h, PRF_SH_EARLY),
                (unsigned long long)h[PRF_CNT_HIT_OVF], (unsigned long long)h[PRF_CNT_UNSORTED], r->ms01);
#endif
    if (h[PRF_CNT_LONG_OVF])
        return fail(PRF_EHIP, "internal: a tile reported %llu rows longer than 65534 positions (at most %u can exist)",
                    (unsigned long long)h[PRF_CNT_LONG_OVF], PRF_LONG_PER_TILE);
    const u64 hit_ovf = h[PRF_CNT_HIT_OVF];
    if (hit_ovf > c->slab_cap) {  // a tile held more rows than its slab: grow the slabs
        want->slab_cap = (u32)std::min<u64>(hit_ovf + hit_ovf / 4 + 64, 1u << 22);
        r->again = true;
    } else if (r->nhits > dst.cap) {  // the compact row array was too small
        if (dst.is_sink) return sink_too_small(c, r->nhits);
        want->hits = with_headroom(r->nhits);
        r->again = true;
    }
    return PRF_OK;
}

// ---- generic kernels over tile ranges (candidates), then verify (rows to rows[0 .. room)) ----
// A run belongs to the word that holds its first position: disjoint ranges give disjoint row sets.
static int tiles_pass(prf_ctx *c, const prf_genome *g, const scan_params &p, const tile_ranges &tiles, prf_hit_dev *rows, u64 room,
                      pass_result *r) {
    const prf_planes pl = planes_of(g);
    HIPCHK(hipMemsetAsync(c->d_counters, 0, PRF_CNT_N * sizeof(u64), c->stream));
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    for (const auto &tr : tiles)
        HIPCHK(prf_launch_scan_generic(c->stream, pl, tr.first * PRF_TILE_WORDS, tr.second * PRF_TILE_WORDS, p.kmin, p.kmax,
                                       p.min_repeats, p.min_span, c->d_cand, c->cand_cap, c->d_counters));
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(prf_launch_verify(c->stream, pl, c->d_cand, c->cand_cap, p.min_repeats, p.min_span, g->d_base, (u32)g->base.size(), rows,
                             room, c->d_counters));
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    u64 *stage = c->h_counters + PRF_CNT_SPARE;
    HIPCHK(hipMemcpyAsync(stage, c->d_counters, 2 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    r->ncand = stage[PRF_CNT_CAND];
    r->nhits = stage[PRF_CNT_HITS];
    HIPCHK(hipEventElapsedTime(&r->ms01, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&r->ms12, c->ev[1], c->ev[2]));
    return PRF_OK;
}

// The tiles with a symbol outside ACGTN in reach (class 3), within the active selection if there is one
static tile_ranges exotic_ranges(const prf_genome *g) {
    if (!g->sel_on) return g->exotic_tiles;
    tile_ranges out;
    for (const auto &e : g->exotic_tiles)
        for (const auto &r : g->sel_tiles) {
            const u64 lo = std::max(e.first, r.first), hi = std::min(e.second, r.second);
            if (lo < hi) out.emplace_back(lo, hi);
        }
    return out;
}

// ---- fused path, second pass: the tiles with symbols outside ACGTN, on the generic kernels with the symbols' own planes
// (R == R matches, reference utils/perfect_repeat_tracker.py:53).  A row belongs to the tile of its first position there too,
// so the two row sets are disjoint.  The rows are appended behind the fused pass's; the array is then sorted on the host.
static int exotic_pass(prf_ctx *c, const prf_genome *g, const scan_params &p, const tile_ranges &exotic, const row_dest &dst,
                       buffer_sizes *want, pass_result *r) {
    const u64 room = dst.cap > r->nhits ? dst.cap - r->nhits : 0;
    pass_result e;
    const int rc = tiles_pass(c, g, p, exotic, dst.rows + r->nhits, room, &e);
    if (rc) return rc;
    r->launches += 1 + (u32)exotic.size();
    const u64 total = r->nhits + e.nhits;
    if (e.ncand > c->cand_cap) {
        want->cand = with_headroom(e.ncand);
        r->again = true;
    } else if (e.nhits > room) {
        if (dst.is_sink) return sink_too_small(c, total);
        want->hits = with_headroom(total);
        r->again = true;
    } else {
        r->ncand += e.ncand;
        r->nhits = total;
        if (e.nhits) r->sorted = false;
        if (dst.is_sink) return prf_write_count_record(c, dst.rows, dst.cap, total);
    }
    return PRF_OK;
}

// ---- generic path: candidates, then rows, over the active selection or the whole genome (its sentinel tile aside) ----
static int generic_pass(prf_ctx *c, const prf_genome *g, const scan_params &p, buffer_sizes *want, pass_result *r) {
    const tile_ranges whole{{0, g->G / PRF_TILE - 1}};
    const int rc = tiles_pass(c, g, p, g->sel_on ? g->sel_tiles : whole, c->d_hits, c->hit_cap, r);
    if (rc) return rc;
    r->launches = 2;
    r->sorted = false;
    if (r->ncand > c->cand_cap) { want->cand = with_headroom(r->ncand); r->again = true; }
    if (r->nhits > c->hit_cap) { want->hits = with_headroom(r->nhits); r->again = true; }
    if (r->again || !c->sink) return PRF_OK;
    // the generic kernels write the context's array: the rows are handed to the sink afterwards
    if (r->nhits > c->sink_cap) return sink_too_small(c, r->nhits);
    if (r->nhits) HIPCHK(hipMemcpyAsync(c->sink, c->d_hits, r->nhits * sizeof(prf_hit_dev), hipMemcpyDeviceToDevice, c->stream));
    return prf_write_count_record(c, c->sink, c->sink_cap, r->nhits);
}

// The passes of a scan (plan: the fused plan, or nullptr for the generic path), repeated with larger buffers while one overflows
static int run_passes(prf_ctx *c, const prf_genome *g, const scan_params &p, const prf_vplan *plan, const tile_ranges &exotic,
                      bool timed, pass_result *r) {
    const launch_view lv = active_launch(g);
    const bool fused = plan && lv.n > 0;
    // rows per tile the slabs hold (8 bytes each): the densest 65536-position tile of the reference's golden chr22 BED has 748
    // rows at motif sizes 1-6
    buffer_sizes want{std::max<u64>(c->cand_cap, lv.positions / 8 + 65536), std::max<u64>(c->hit_cap, lv.positions / 32 + 65536),
                      std::max<u32>(c->slab_cap, 1024u)};
    for (int attempt = 0; attempt <= 8; attempt++) {
        int rc = fused ? ensure_slabs(c, lv.n, want.slab_cap) : PRF_OK;
        if (!rc) rc = ensure_buffers(c, fused && exotic.empty() ? c->cand_cap : want.cand, want.hits);  // (d_cand: generic kernels only)
        *r = pass_result{};
        if (!rc && !plan) rc = generic_pass(c, g, p, &want, r);
        if (!rc && fused) {
            rc = fused_pass(c, g, *plan, p, row_destination(c), timed, &want, r);
            r->launches = 2u * (attempt + 1);  // (a scan that had to grow its buffers and run again shows here)
        }
        if (!rc && plan && !r->again && !exotic.empty()) rc = exotic_pass(c, g, p, exotic, row_destination(c), &want, r);
        if (rc || !r->again) return rc;
    }
    return fail(PRF_EHIP, "prf_scan_genome: buffers still overflowing after 8 attempts");
}

// The rows of the last scan to the host.  The fused path hands them over sorted by (contig, start, end) (reference
// perfect_repeat_finder.py:81); the generic path, and a fused scan in which some tile held more rows than its LDS sort list,
// are sorted here.
static int fetch_rows(prf_ctx *c, u64 nhits, bool sorted, prf_hits *out) {
    prf_hit *rows = (prf_hit *)malloc(nhits * sizeof(prf_hit));
    if (!rows) return fail(PRF_ENOMEM, "prf_scan_genome: cannot allocate %llu rows", (unsigned long long)nhits);
    static_assert(sizeof(prf_hit) == sizeof(prf_hit_dev), "row layouts must agree");
    // on the library's stream: the scan returned when the counters were posted, the last workgroups may still be
    // copying their rows, and the stream is a non-blocking one (the null stream does not wait for it)
    hipError_t e = hipMemcpyAsync(rows, c->last.rows, nhits * sizeof(prf_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        free(rows);
        return fail(PRF_EHIP, "row copy failed: %s", hipGetErrorString(e));
    }
    if (!sorted)
        std::sort(rows, rows + nhits, [](const prf_hit &a, const prf_hit &b) {
            if (a.contig != b.contig) return a.contig < b.contig;
            if (a.start != b.start) return a.start < b.start;
            if (a.end != b.end) return a.end < b.end;
            return a.k < b.k;
        });
    out->rows = rows;
    out->n = nhits;
    return PRF_OK;
}

static int scan_impl(prf_ctx *c, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                     uint32_t min_span, uint32_t flags, prf_hits *out, prf_scan_stats *stats) {
    if (!c || !g) return fail(PRF_EINVAL, "prf_scan_genome: NULL context or genome");
    if (g->ctx != c) return fail(PRF_EINVAL, "prf_scan_genome: genome belongs to another context");
    if (out) { out->rows = nullptr; out->n = 0; }
    int rc = check_params(kmin, kmax, min_repeats, min_span, min_repeats < 2 ? 0u : g->kmax_hint);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->dev));
    const scan_params p{kmin, kmax, min_repeats, min_span};
    // outside the closed form of the packed kernels: the literal lane on the bytes rebuilt from the planes
    if (min_repeats < 2) return prf_literal_genome(c, g, p, out, stats);

    prf_vplan plan;
    const bool vs = !(flags & PRF_SCAN_FORCE_GENERIC) && prf_vertical_plan(kmin, kmax, min_repeats, min_span, &plan);
    const launch_view lv = active_launch(g);
    const tile_ranges exotic = vs ? exotic_ranges(g) : tile_ranges{};
    pass_result r;
    if (vs && lv.n == 0 && exotic.empty())  // nothing but N (or no contig at all): no tile to launch, no rows
        rc = c->sink ? prf_write_count_record(c, c->sink, c->sink_cap, 0) : PRF_OK;
    else
        rc = run_passes(c, g, p, vs ? &plan : nullptr, exotic, stats && !(flags & PRF_SCAN_DEFER_TIMING), &r);
    if (rc) return rc;
    c->last = {row_destination(c).rows, r.nhits, kmax};
    if (stats) fill_stats(stats, r, vs ? 1u : 0u, lv.positions, vs ? lv.n : 0u, vs && r.launches ? c->scan_seq : 0);
    if ((flags & PRF_SCAN_NO_FETCH) || !out || r.nhits == 0) return PRF_OK;
    return fetch_rows(c, r.nhits, r.sorted, out);
}

int prf_scan_genome(prf_ctx *c, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                    uint32_t min_span, uint32_t flags, prf_hits *out, prf_scan_stats *stats) {
    return guarded("prf_scan_genome", [&] { return scan_impl(c, g, kmin, kmax, min_repeats, min_span, flags, out, stats); });
}

int prf_scan(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
             uint32_t min_span, uint32_t flags, prf_hits *out, prf_scan_stats *stats) {
    if (min_repeats == 1)  // outside the closed form of the packed kernels: the literal lane, contig by contig
        return guarded("prf_scan", [&] {
            return prf_literal_impl(c, contigs, n_contigs, nullptr, scan_params{kmin, kmax, min_repeats, min_span}, out, stats);
        });
    prf_genome *g = nullptr;
    int rc = prf_genome_load(c, contigs, n_contigs, kmax, &g);
    if (rc) return rc;
    rc = prf_scan_genome(c, g, kmin, kmax, min_repeats, min_span, flags, out, stats);
    prf_genome_free(g);
    return rc;
}

// ---- pipelined scans: enqueue now, collect later (at most two in flight) ----
// The launch latency and the host's share of a scan (~9 of ~37 us on the chr22 scan) then overlap the previous
// scan's kernel: kernels of one stream run back to back.  Fused path only, no row sink, buffers already sized by an
// ordinary scan of the same genome and parameters; anything else is refused and the caller scans synchronously.
static int scan_async_impl(prf_ctx *c, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span,
                           uint64_t *seq_out, const u64 **counters_out = nullptr, const prf_hit_dev **rows_out = nullptr) {
    if (!c || !g || !seq_out) return fail(PRF_EINVAL, "prf_scan_genome_async: bad arguments");
    if (g->ctx != c) return fail(PRF_EINVAL, "prf_scan_genome_async: genome belongs to another context");
    if (c->sink) return fail(PRF_EUNSUPPORTED, "prf_scan_genome_async: not with a row sink");
    if (min_repeats < 2 || check_params(kmin, kmax, min_repeats, min_span, g->kmax_hint))
        return fail(PRF_EUNSUPPORTED, "prf_scan_genome_async: parameters the synchronous call would refuse or serve otherwise");
    prf_vplan plan;
    if (!prf_vertical_plan(kmin, kmax, min_repeats, min_span, &plan))
        return fail(PRF_EUNSUPPORTED, "prf_scan_genome_async: no fused plan for these parameters");
    const launch_view lv = active_launch(g);
    if (lv.n == 0) return fail(PRF_EUNSUPPORTED, "prf_scan_genome_async: nothing to launch");
    if (!g->exotic_tiles.empty())
        return fail(PRF_EUNSUPPORTED, "prf_scan_genome_async: the genome holds symbols outside ACGTN (a second pass follows the fused scan); scan synchronously");
    if (lv.n > c->slab_slots || c->slab_cap == 0 || c->hit_cap == 0)
        return fail(PRF_EUNSUPPORTED, "prf_scan_genome_async: scan this genome synchronously once first (buffers are sized there)");
    HIPCHK(hipSetDevice(c->dev));
    prf_ctx::async_slot &sl = c->slot[c->async_n & 1u];
    if (sl.seq) return fail(PRF_EINVAL, "prf_scan_genome_async: two scans are in flight already; prf_scan_wait() first");
    if ((c->async_n & 1u) == 0) {
        sl.h = c->h_counters; sl.h_dev = c->h_counters_dev; sl.rows = c->d_hits;
    } else {
        if (!c->h_async) {
            HIPCHK(hipHostMalloc((void **)&c->h_async, PRF_CNT_BLOCK_WORDS * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
            memset(c->h_async, 0, PRF_CNT_BLOCK_WORDS * sizeof(u64));
        }
        const int rc = grow(c->d_hits_async, c->hit_cap_async, c->hit_cap);
        if (rc) return rc;
        sl.h = c->h_async; sl.rows = c->d_hits_async;
        if (!sl.h_dev) HIPCHK(hipHostGetDevicePointer((void **)&sl.h_dev, c->h_async, 0));
    }
    // (the slabs are shared by the two scans in flight: kernels of one stream run in order, and a scan's gather has read
    // the slabs before the next scan's tiles write them)
    if (counters_out) *counters_out = c->d_vcounters + (size_t)c->parity * PRF_CNT_N;  // (the block this scan counts in)
    if (rows_out) *rows_out = sl.rows;
    u64 seq = 0;
    const int rc = launch_fused(c, g, plan, scan_params{kmin, kmax, min_repeats, min_span}, sl.rows, c->hit_cap, 0u, sl.h_dev, &seq);
    if (rc) return rc;
    sl.seq = seq;
    sl.positions = lv.positions;
    sl.tiles = lv.n;
    sl.kmax = kmax;
    c->async_n++;
    *seq_out = seq;
    return PRF_OK;
}

static prf_ctx::async_slot *slot_of(prf_ctx *c, u64 seq) {
    return c->slot[0].seq == seq ? &c->slot[0] : (c->slot[1].seq == seq ? &c->slot[1] : nullptr);
}

// Wait for the scan in a pipelined slot and free the slot, whether the scan succeeded or not.  clear_side_cnt: also zero the
// pack kernels' row counter (a pack that ran leaves it zero; this is for the pack that failed to launch behind the scan).
static int retire_slot(prf_ctx *c, prf_ctx::async_slot &sl, bool clear_side_cnt) {
    const int rc = wait_for_seq(c, sl.seq, sl.h);
    sl.seq = 0;
    if (clear_side_cnt) (void)hipMemsetAsync(c->d_side_cnt, 0, sizeof(u64), c->stream);
    return rc;
}

int prf_scan_genome_async(prf_ctx *c, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span,
                          uint64_t *seq_out) {
    return guarded("prf_scan_genome_async", [&] { return scan_async_impl(c, g, kmin, kmax, min_repeats, min_span, seq_out); });
}

// A pipelined scan whose rows leave as 8-byte wire words without the host in between: the pack kernels are enqueued behind the
// scan's gather on the library's stream and read the row count from the scan's counter block (which the NEXT scan's gather
// clears: stream order keeps it alive until then).  If the pack cannot be launched, the scan is collected here: the call
// fails and leaves the context as it was before it.
int prf_scan_genome_async_packed(prf_ctx *c, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span,
                                 void *dst_device, uint64_t capacity_rows, uint64_t side_capacity, uint64_t *seq_out) {
    return guarded("prf_scan_genome_async_packed", [&]() -> int {
        if (!dst_device) return fail(PRF_EINVAL, "prf_scan_genome_async_packed: no destination");
        if (kmax > 511u) return fail(PRF_EUNSUPPORTED, "the 8-byte wire rows hold motif sizes up to 511 (max_motif_size %u)", kmax);
        const u64 *counters = nullptr;
        const prf_hit_dev *rows = nullptr;
        const int rc = scan_async_impl(c, g, kmin, kmax, min_repeats, min_span, seq_out, &counters, &rows);
        if (rc) return rc;
        const hipError_t e = prf_launch_pack_rows_dev(c->stream, rows, counters, c->hit_cap, c->slab_cap, capacity_rows, g->d_base,
                                                      (u64 *)dst_device, side_capacity, c->d_side_cnt);
        if (e == hipSuccess) return PRF_OK;
        (void)retire_slot(c, *slot_of(c, *seq_out), true);
        return fail(e == hipErrorOutOfMemory ? PRF_ENOMEM : PRF_EHIP, "prf_launch_pack_rows_dev failed: %s", hipGetErrorString(e));
    });
}

int prf_scan_wait(prf_ctx *c, uint64_t seq, prf_scan_stats *stats) {
    if (!c || !seq) return fail(PRF_EINVAL, "prf_scan_wait: bad arguments");
    prf_ctx::async_slot *sl = slot_of(c, seq);
    if (!sl) return fail(PRF_EINVAL, "prf_scan_wait: scan %llu is not in flight", (unsigned long long)seq);
    const int rc = retire_slot(c, *sl, false);
    if (rc) return rc;
    const pass_result r = read_fused(sl->h);
    // (the conditions under which prf_pack_finish_dev_kernel poisons the count word: the wire buffer and this call agree)
    if (sl->h[PRF_CNT_HIT_OVF] > c->slab_cap)
        return fail(PRF_EUNSUPPORTED, "prf_scan_wait: the slabs sized by the last synchronous scan overflowed (a tile holds %llu rows, a slab %u); scan synchronously",
                    (unsigned long long)sl->h[PRF_CNT_HIT_OVF], c->slab_cap);
    if (r.nhits > c->hit_cap)
        return fail(PRF_EUNSUPPORTED, "prf_scan_wait: the row array sized by the last synchronous scan overflowed (%llu rows, it holds %llu); scan synchronously",
                    (unsigned long long)r.nhits, (unsigned long long)c->hit_cap);
    if (sl->h[PRF_CNT_LONG_OVF])
        return fail(PRF_EUNSUPPORTED, "prf_scan_wait: a tile's list of long rows overflowed; scan synchronously");
    c->last = {sl->rows, r.nhits, sl->kmax};
    if (stats) fill_stats(stats, r, 1, sl->positions, sl->tiles, seq);
    return PRF_OK;
}

}  // extern "C"
