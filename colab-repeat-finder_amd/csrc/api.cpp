// api.cpp -- the C ABI of libprf (include/prf.h) but for the FASTA / BED entry points (fasta_io.cpp) and the interrupted
// repeats (interrupted.cpp): contexts and the error text, genome residency, the perfect scan with its passes (fused_pass,
// exotic_pass, generic_pass under run_passes), the literal lane (min_repeats == 1: literal_device and its callers), pipelined
// scans, row hand-off to the device.  What it shares with interrupted.cpp is in prf_ctx.h.
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
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "prf_ctx.h"
#include "scan_vertical.h"

static thread_local std::string g_err;

static const u64 PRF_FRONT_PAD = 8;  // readable words in front of every linear plane (X = all ones there)

int prf_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

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

struct prf_genome {
    prf_ctx *ctx = nullptr;
    std::vector<u64> base, len;
    u64 positions = 0;   // sum of contig lengths
    u64 G = 0;           // positions in the global coordinate space incl. gaps and the sentinel tile
    u64 nwords = 0;      // G / 64
    u64 padw = 0;        // readable words past nwords in every linear plane
    u32 kmax_hint = 0;
    u64 *H = nullptr, *L = nullptr, *X = nullptr;  // point PRF_FRONT_PAD words into their allocations
    // symbols outside ACGTN (ordinary symbols to the reference): five planes of their codes, present only if the input has
    // any; the tiles with such a symbol in reach (class 3) are scanned by the generic kernels
    u64 *E[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    u64 **d_E = nullptr;                            // the five pointers, on the device (fused kernel's general routine)
    std::vector<std::pair<u64, u64>> exotic_tiles;  // merged [first, last) ranges of class-3 tiles, ascending
    u64 *d_base = nullptr;
    uint4 *d_tile_info = nullptr;  // per tile: {contig, 0, contig base lo, hi}
    prf_vplanes vp;      // bit-sliced copy for scan_vertical
    // active selection (prf_genome_select): the scans of this genome cover only these tiles.  Off: the whole genome.
    bool sel_on = false;
    u32 *d_sel_list = nullptr;
    u32 sel_n = 0, sel_flat = ~0u;
    u64 sel_positions = 0;
    std::vector<std::pair<u64, u64>> sel_tiles;  // merged [first, last) tile ranges, ascending
};

// what a scan of the genome launches
struct launch_view {
    const u32 *list;
    u32 n, flat;
    u64 positions;
};
static launch_view active_launch(const prf_genome *g) {
    if (g->sel_on) return launch_view{g->d_sel_list, g->sel_n, g->sel_flat, g->sel_positions};
    return launch_view{g->vp.launch_list, g->vp.n_launch, g->vp.flat_base, g->positions};
}

int prf_genome_contig_view(const prf_genome *g, u32 contig, prf_contig_view *out) {
    if (!g || !out) return fail(PRF_EINVAL, "NULL genome");
    if (contig >= g->base.size()) return fail(PRF_EINVAL, "contig %u out of range (the genome holds %zu)", contig, g->base.size());
    out->ctx = g->ctx;
    out->planes = prf_planes{g->H, g->L, g->X, {g->E[0], g->E[1], g->E[2], g->E[3], g->E[4]}};
    out->base = g->base[contig];
    out->len = g->len[contig];
    out->kmax_hint = g->kmax_hint;
    return PRF_OK;
}

extern "C" {

int prf_abi_version(void) { return PRF_ABI_VERSION; }

const char *prf_last_error(void) { return g_err.c_str(); }

int prf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int prf_open(int device_id, prf_ctx **out) {
    if (!out) return fail(PRF_EINVAL, "prf_open: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(PRF_ENODEV, "prf_open: no HIP device visible (%s); libprf has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(PRF_EINVAL, "prf_open: device %d out of range [0,%d)", device_id, n);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PRF_ENODEV, "prf_open: device %d is %s; libprf is built for gfx950 (MI355X) only", device_id,
                    prop.gcnArchName);
    HIPCHK(hipSetDevice(device_id));
    prf_ctx *c = new (std::nothrow) prf_ctx();
    if (!c) return fail(PRF_ENOMEM, "prf_open: out of host memory");
    c->dev = device_id;
    struct guard_t {  // a failure below must not leak the half-built context
        prf_ctx *c;
        ~guard_t() { if (c) prf_close(c); }
    } guard{c};
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto &ev : c->ev) HIPCHK(hipEventCreate(&ev));
    for (auto &ev : c->ring) HIPCHK(hipEventCreate(&ev));
    HIPCHK(hipMalloc((void **)&c->d_counters, PRF_CNT_N * sizeof(u64)));
    HIPCHK(hipHostMalloc((void **)&c->h_counters, (PRF_CNT_N + 8) * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
    // recycled pinned blocks are not zeroed, and the scan serial numbers restart at 1 for every context: a stale
    // serial number left by a closed context must never look like a finished scan
    memset(c->h_counters, 0, (PRF_CNT_N + 8) * sizeof(u64));
    HIPCHK(hipHostGetDevicePointer((void **)&c->h_counters_dev, c->h_counters, 0));
    HIPCHK(hipMalloc((void **)&c->d_vcounters, 2 * PRF_CNT_N * sizeof(u64)));
    HIPCHK(hipMemset(c->d_vcounters, 0, 2 * PRF_CNT_N * sizeof(u64)));
    HIPCHK(hipMalloc((void **)&c->d_side_cnt, sizeof(u64)));
    HIPCHK(hipMemset(c->d_side_cnt, 0, sizeof(u64)));
    HIPCHK(hipEventCreateWithFlags(&c->ev_handoff, hipEventDisableTiming));
    guard.c = nullptr;
    *out = c;
    return PRF_OK;
}

void prf_close(prf_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->dev);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)hipHostFree(c->h_counters);
    (void)hipHostFree(c->h_async);
    for (void *p : {(void *)c->d_counters, (void *)c->d_hits_async, (void *)c->d_vcounters, (void *)c->d_side_cnt, c->lit_scratch,
                    (void *)c->d_cand, (void *)c->d_hits, (void *)c->d_slabs, (void *)c->d_long_ends, (void *)c->d_slab_count,
                    (void *)c->d_block_sum})
        (void)hipFree(p);
    if (c->ev_handoff) (void)hipEventDestroy(c->ev_handoff);
    for (auto &ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : c->ring)
        if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void prf_genome_free(prf_genome *g) {
    if (!g) return;
    if (g->ctx) (void)hipSetDevice(g->ctx->dev);
    for (u64 *plane : {g->H, g->L, g->X, g->E[0], g->E[1], g->E[2], g->E[3], g->E[4]})
        if (plane) (void)hipFree(plane - PRF_FRONT_PAD);
    for (void *p : {(void *)g->d_E, (void *)g->d_base, (void *)g->d_tile_info, (void *)g->vp.VH, (void *)g->vp.VL,
                    (void *)g->vp.tile_class, (void *)g->vp.launch_list, (void *)g->d_sel_list})
        (void)hipFree(p);
    delete g;
}

uint64_t prf_genome_positions(const prf_genome *g) { return g ? g->positions : 0; }

// One linear plane of the genome: PRF_FRONT_PAD readable words in front of it, padw behind it, both filled with `pad`
static int alloc_plane(prf_ctx *c, const prf_genome *g, u64 **plane, int pad) {
    u64 *p = nullptr;
    HIPCHK(hipMalloc((void **)&p, (PRF_FRONT_PAD + g->nwords + g->padw) * 8));
    *plane = p + PRF_FRONT_PAD;
    HIPCHK(hipMemsetAsync(p, pad, PRF_FRONT_PAD * 8, c->stream));
    HIPCHK(hipMemsetAsync(*plane + g->nwords, pad, g->padw * 8, c->stream));
    return PRF_OK;
}

// The contig of every tile (contigs start on tile boundaries; the gap tiles behind a contig count as its own)
static int upload_tile_info(prf_genome *g) {
    const u64 ntiles = g->G / PRF_TILE;
    std::vector<uint4> info(ntiles, make_uint4(0, 0, 0, 0));
    for (size_t ci = 0; ci < g->base.size(); ci++) {
        const u64 t0 = g->base[ci] / PRF_TILE, t1 = ci + 1 < g->base.size() ? g->base[ci + 1] / PRF_TILE : ntiles;
        for (u64 t = t0; t < t1; t++) info[t] = make_uint4((u32)ci, 0u, (u32)g->base[ci], (u32)(g->base[ci] >> 32));
    }
    HIPCHK(hipMalloc((void **)&g->d_tile_info, sizeof(uint4) * ntiles));
    HIPCHK(hipMemcpy(g->d_tile_info, info.data(), sizeof(uint4) * ntiles, hipMemcpyHostToDevice));
    return PRF_OK;
}

// Letters other than A, C, G, T, N: the planes of their codes, and the tile ranges the generic kernels take
static int load_exotic(prf_ctx *c, prf_genome *g, const uint8_t *asc) {
    for (u64 *&plane : g->E) {
        const int rc = alloc_plane(c, g, &plane, 0);
        if (rc) return rc;
    }
    HIPCHK(prf_launch_pack_exotic(c->stream, asc, g->nwords, g->E));
    HIPCHK(hipMalloc((void **)&g->d_E, 5 * sizeof(u64 *)));
    HIPCHK(hipMemcpyAsync(g->d_E, g->E, 5 * sizeof(u64 *), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const std::vector<unsigned char> &cls = g->vp.h_class;
    for (u64 t = 0; t + 1 < cls.size(); t++) {
        if (cls[t] != 3) continue;
        if (!g->exotic_tiles.empty() && g->exotic_tiles.back().second == t) g->exotic_tiles.back().second = t + 1;
        else g->exotic_tiles.emplace_back(t, t + 1);
    }
    return PRF_OK;
}

// contigs[i].ascii == nullptr with seeds != nullptr: contig i is generated on the device from seeds[i]
// recipe (with seeds): 1 = uniform background, 2 = stand-in recipe 2 (N blocks + planted repeats)
static int genome_load_impl(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmax_hint, prf_genome **out,
                            const uint64_t *seeds = nullptr, int recipe = 1) {
    if (!c || !out || n_contigs < 0 || (n_contigs > 0 && !contigs))
        return fail(PRF_EINVAL, "prf_genome_load: bad arguments");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->dev));
    if (kmax_hint < 1) kmax_hint = 1;
    if (kmax_hint > 60000) return fail(PRF_EUNSUPPORTED, "prf_genome_load: kmax_hint %u > 60000", kmax_hint);
    prf_genome *g = new (std::nothrow) prf_genome();
    if (!g) return fail(PRF_ENOMEM, "prf_genome_load: out of host memory");
    struct guard_t {
        prf_genome *g;
        ~guard_t() { if (g) prf_genome_free(g); }
    } guard{g};
    g->ctx = c;
    g->kmax_hint = kmax_hint;
    const u64 gap = (u64)kmax_hint + 64;
    u64 cur = 0;
    for (int i = 0; i < n_contigs; i++) {
        if (contigs[i].len && !contigs[i].ascii && !seeds) return fail(PRF_EINVAL, "prf_genome_load: contig %d has NULL data", i);
        g->base.push_back(cur);
        g->len.push_back(contigs[i].len);
        g->positions += contigs[i].len;
        cur = (cur + contigs[i].len + gap + PRF_TILE - 1) / PRF_TILE * PRF_TILE;
    }
    if (cur == 0) cur = PRF_TILE;
    g->G = cur + PRF_TILE;  // one all-gap sentinel tile: every walk to the right ends inside the arrays
    if (g->G >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "prf_genome_load: input too large (2^40 positions)");  // row keys: 40-bit offsets
    g->nwords = g->G / 64;
    g->padw = kmax_hint / 64 + 8;

    uint8_t *asc = nullptr;
    HIPCHK(hipMalloc((void **)&asc, g->G));
    struct asc_guard_t {
        uint8_t *p;
        ~asc_guard_t() { (void)hipFree(p); }
    } asc_guard{asc};
    HIPCHK(prf_launch_fill_u64(c->stream, (u64 *)asc, g->G / 8, 0x4E4E4E4E4E4E4E4Eull));  // 'N' everywhere
    for (int i = 0; i < n_contigs; i++) {
        if (!contigs[i].len) continue;
        if (seeds && recipe == 2)
            HIPCHK(prf_launch_standin2(c->stream, asc + g->base[i], contigs[i].len, seeds[i]));
        else if (seeds)  // the generator writes whole 16-byte groups; the tail beyond len is 'N' again, like the gap
            HIPCHK(prf_launch_synth(c->stream, asc + g->base[i], contigs[i].len, seeds[i]));
        else
            HIPCHK(hipMemcpyAsync(asc + g->base[i], contigs[i].ascii, contigs[i].len, hipMemcpyHostToDevice, c->stream));
    }
    int rc = alloc_plane(c, g, &g->H, 0);
    if (!rc) rc = alloc_plane(c, g, &g->L, 0);
    if (!rc) rc = alloc_plane(c, g, &g->X, 0xFF);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_counters, 0xFF, PRF_CNT_N * sizeof(u64), c->stream));
    HIPCHK(hipMemsetAsync(c->d_counters + PRF_CNT_EXOTIC, 0, sizeof(u64), c->stream));
    HIPCHK(prf_launch_pack_linear(c->stream, asc, g->nwords, g->H, g->L, g->X, c->d_counters + PRF_CNT_BADPOS,
                                  c->d_counters + PRF_CNT_EXOTIC));
    HIPCHK(hipMalloc((void **)&g->d_base, sizeof(u64) * (size_t)(n_contigs > 0 ? n_contigs : 1)));
    if (n_contigs > 0)
        HIPCHK(hipMemcpyAsync(g->d_base, g->base.data(), sizeof(u64) * (size_t)n_contigs, hipMemcpyHostToDevice, c->stream));
    if ((rc = upload_tile_info(g))) return rc;
    // bit-sliced copy for the vertical kernel (built from the ASCII while it is still resident)
    rc = prf_vertical_pack(c->stream, asc, g->G, &g->vp);
    if (rc != hipSuccess)
        return fail(rc == (int)hipErrorOutOfMemory ? PRF_ENOMEM : PRF_EHIP, "vertical pack failed: %s", hipGetErrorString((hipError_t)rc));
    HIPCHK(hipMemcpyAsync(c->h_counters, c->d_counters, PRF_CNT_N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const u64 bad = c->h_counters[PRF_CNT_BADPOS];
    if (bad != ~0ull) {
        size_t ci = std::upper_bound(g->base.begin(), g->base.end(), bad) - g->base.begin() - 1;
        return fail(PRF_ESYMBOL,
                    "unsupported symbol at contig %zu position %llu: only letters can be packed (A, C, G, T, N and -- as ordinary "
                    "symbols, like the reference -- any other letter, in either case); libprf refuses other bytes instead of guessing",
                    ci, (unsigned long long)(bad - g->base[ci]));
    }
    if (c->h_counters[PRF_CNT_EXOTIC] && (rc = load_exotic(c, g, asc))) return rc;
    guard.g = nullptr;
    *out = g;
    return PRF_OK;
}

int prf_genome_load(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmax_hint, prf_genome **out) {
    return guarded("prf_genome_load", [&] { return genome_load_impl(c, contigs, n_contigs, kmax_hint, out); });
}

// contigs generated on the device from seeds (recipe 1: uniform background, 2: stand-in recipe 2)
static int genome_generate(const char *name, prf_ctx *c, const uint64_t *lens, const uint64_t *seeds, int n_contigs,
                           uint32_t kmax_hint, prf_genome **out, int recipe) {
    if (n_contigs < 0 || (n_contigs > 0 && (!lens || !seeds))) return fail(PRF_EINVAL, "%s: bad arguments", name);
    return guarded(name, [&] {
        std::vector<prf_contig> cs((size_t)(n_contigs > 0 ? n_contigs : 1));
        for (int i = 0; i < n_contigs; i++) cs[i] = prf_contig{nullptr, lens[i]};
        return genome_load_impl(c, cs.data(), n_contigs, kmax_hint, out, seeds, recipe);
    });
}

int prf_genome_synth(prf_ctx *c, const uint64_t *lens, const uint64_t *seeds, int n_contigs, uint32_t kmax_hint, prf_genome **out) {
    return genome_generate("prf_genome_synth", c, lens, seeds, n_contigs, kmax_hint, out, 1);
}

int prf_genome_standin(prf_ctx *c, const uint64_t *lens, const uint64_t *seeds, int n_contigs, uint32_t kmax_hint, prf_genome **out) {
    return genome_generate("prf_genome_standin", c, lens, seeds, n_contigs, kmax_hint, out, 2);
}

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
static int launch_fused(prf_ctx *c, const prf_genome *g, const prf_vplan &plan, u32 min_repeats, u32 min_span, prf_hit_dev *rows,
                        u64 rows_cap, u32 count_row, u64 *host_counters_dev, u64 *seq_out) {
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
    a.min_repeats = min_repeats; a.min_span = min_span;
    a.tile_info = g->d_tile_info;
    a.counters = c->d_vcounters + (size_t)c->parity * PRF_CNT_N;
    a.dbg = nullptr;
#ifdef PRF_STAMPS
    {
        static u64 *dbg_buf = nullptr;
        const size_t nu = (size_t)(1u << 18) * PRF_VMAX_WAVES * 16;  // up to 262144 tiles
        if (!dbg_buf) HIPCHK(hipMalloc((void **)&dbg_buf, nu * sizeof(u64)));
        if (lv.n <= (1u << 18)) {
            HIPCHK(hipMemsetAsync(dbg_buf, 0, (size_t)lv.n * PRF_VMAX_WAVES * 16 * sizeof(u64), c->stream));
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

static int literal_genome(prf_ctx *c, const prf_genome *g, u32 kmin, u32 kmax, u32 min_repeats, u32 min_span, prf_hits *out,
                          prf_scan_stats *stats);

struct scan_params {
    u32 kmin, kmax, min_repeats, min_span;
};

using tile_ranges = std::vector<std::pair<u64, u64>>;  // [first, last) tile ranges, ascending

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

// The count record {n, 0, 0} behind a caller-owned row array (dst[cap]), staged in the spare pinned words behind the counter
// block.  Returns when it is on the device.
static int write_count_record(prf_ctx *c, prf_hit_dev *dst, u64 cap, u64 n) {
    u64 *stage = c->h_counters + PRF_CNT_N + 2;
    stage[0] = n; stage[1] = 0; stage[2] = 0;
    HIPCHK(hipMemcpyAsync(dst + cap, stage, sizeof(prf_hit_dev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PRF_OK;
}

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
        const size_t nu = (size_t)c->stamps_n * PRF_VMAX_WAVES * 16;
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
    int rc = launch_fused(c, g, plan, p.min_repeats, p.min_span, dst.rows, dst.cap, dst.is_sink ? 1u : 0u, c->h_counters_dev, &seq);
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
        want->hits = r->nhits + r->nhits / 8 + 1024;
        r->again = true;
    }
    return PRF_OK;
}

// ---- generic kernels over tile ranges (candidates), then verify (rows to rows[0 .. room)) ----
// A run belongs to the word that holds its first position: disjoint ranges give disjoint row sets.
static int tiles_pass(prf_ctx *c, const prf_genome *g, const scan_params &p, const tile_ranges &tiles, prf_hit_dev *rows, u64 room,
                      pass_result *r) {
    const prf_planes pl{g->H, g->L, g->X, {g->E[0], g->E[1], g->E[2], g->E[3], g->E[4]}};
    HIPCHK(hipMemsetAsync(c->d_counters, 0, PRF_CNT_N * sizeof(u64), c->stream));
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    for (const auto &tr : tiles)
        HIPCHK(prf_launch_scan_generic(c->stream, pl, tr.first * PRF_TILE_WORDS, tr.second * PRF_TILE_WORDS, p.kmin, p.kmax,
                                       p.min_repeats, p.min_span, c->d_cand, c->cand_cap, c->d_counters));
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(prf_launch_verify(c->stream, pl, c->d_cand, c->cand_cap, p.min_repeats, p.min_span, g->d_base, (u32)g->base.size(), rows,
                             room, c->d_counters));
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    u64 *stage = c->h_counters + PRF_CNT_N + 2;  // spare pinned words behind the counter block
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
        want->cand = e.ncand + e.ncand / 8 + 1024;
        r->again = true;
    } else if (e.nhits > room) {
        if (dst.is_sink) return sink_too_small(c, total);
        want->hits = total + total / 8 + 1024;
        r->again = true;
    } else {
        r->ncand += e.ncand;
        r->nhits = total;
        if (e.nhits) r->sorted = false;
        if (dst.is_sink) return write_count_record(c, dst.rows, dst.cap, total);
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
    if (r->ncand > c->cand_cap) { want->cand = r->ncand + r->ncand / 8 + 1024; r->again = true; }
    if (r->nhits > c->hit_cap) { want->hits = r->nhits + r->nhits / 8 + 1024; r->again = true; }
    if (r->again || !c->sink) return PRF_OK;
    // the generic kernels write the context's array: the rows are handed to the sink afterwards
    if (r->nhits > c->sink_cap) return sink_too_small(c, r->nhits);
    if (r->nhits) HIPCHK(hipMemcpyAsync(c->sink, c->d_hits, r->nhits * sizeof(prf_hit_dev), hipMemcpyDeviceToDevice, c->stream));
    return write_count_record(c, c->sink, c->sink_cap, r->nhits);
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
    // outside the closed form of the packed kernels: the literal lane on the bytes rebuilt from the planes
    if (min_repeats < 2) return literal_genome(c, g, kmin, kmax, min_repeats, min_span, out, stats);

    prf_vplan plan;
    const bool vs = !(flags & PRF_SCAN_FORCE_GENERIC) && prf_vertical_plan(kmin, kmax, min_repeats, min_span, &plan);
    const launch_view lv = active_launch(g);
    const tile_ranges exotic = vs ? exotic_ranges(g) : tile_ranges{};
    pass_result r;
    if (vs && lv.n == 0 && exotic.empty())  // nothing but N (or no contig at all): no tile to launch, no rows
        rc = c->sink ? write_count_record(c, c->sink, c->sink_cap, 0) : PRF_OK;
    else
        rc = run_passes(c, g, scan_params{kmin, kmax, min_repeats, min_span}, vs ? &plan : nullptr, exotic,
                        stats && !(flags & PRF_SCAN_DEFER_TIMING), &r);
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

// ---- the literal lane (scan_literal.hip): regimes outside the closed form ----
// One sequence at a time, straight from its ASCII bytes (upper-cased on the device): one thread per (position, motif size)
// evaluates the reference's flush call as written; the rows are then sorted like reference :81 and reduced to the shortest
// motif per (start, end) -- what the reference's dictionary holds at the end (utils/perfect_repeat_tracker.py:93-101) -- on the
// device as well (prf_lit_sort_unique).
// d_seq: L bytes on the device (16-byte aligned: the 64-positions kernel reads whole 16-byte groups, 16 readable bytes behind them); upper: not upper-cased / validated yet
// front: the N trimmed off the front of the contig -- the rows and the position of an unsupported symbol are shifted by it
static int literal_device(prf_ctx *c, uint8_t *d_seq, u64 L, bool upper, u32 contig_index, u32 kmin, u32 kmax, u32 min_repeats,
                          u32 min_span, u64 stop, std::vector<prf_hit> &rows_out, float *ms, u32 *launches, u64 front) {
    if (stop > L) stop = L;
    dev_array<prf_hit_dev> rows;
    u64 cap = L / 16 + 4096;
    u64 *h = c->h_counters;
    for (int attempt = 0;; attempt++) {
        if (const int rc = rows.alloc(cap)) return rc;
        HIPCHK(hipMemsetAsync(c->d_counters, 0, PRF_CNT_N * sizeof(u64), c->stream));
        HIPCHK(hipMemsetAsync(c->d_counters + PRF_CNT_BADPOS, 0xFF, sizeof(u64), c->stream));
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        if (attempt == 0 && upper) HIPCHK(prf_launch_lit_upper(c->stream, d_seq, L, c->d_counters + PRF_CNT_BADPOS));
        HIPCHK(prf_launch_lit_events(c->stream, d_seq, L, kmin, kmax, min_repeats, min_span, stop, contig_index, rows.p, cap,
                                     c->d_counters));
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(h, c->d_counters, PRF_CNT_N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        *ms += t;
        *launches += attempt == 0 && upper ? 2 : 1;
        if (h[PRF_CNT_BADPOS] != ~0ull)
            return fail(PRF_ESYMBOL,
                        "unsupported symbol at contig %u position %llu: only letters are accepted (A, C, G, T, N and -- as ordinary "
                        "symbols, like the reference -- any other letter, in either case); libprf refuses other bytes instead of guessing",
                        contig_index, (unsigned long long)(h[PRF_CNT_BADPOS] + front));
        if (h[PRF_CNT_CAND])
            return fail(PRF_EINDEX, "string index out of range");  // the message of Python's IndexError (tracker :87)
        const u64 n = h[PRF_CNT_HITS];
        if (n <= cap) {
            // sorted by (start, end) and reduced to the shortest motif per (start, end) on the device (scan_literal.hip)
            if (n) {
                dev_array<prf_hit_dev> uniq;
                if (const int rc = uniq.alloc(n)) return rc;
                u64 *d_n = c->d_counters + PRF_CNT_HITS;  // read above; reused for the number of rows that stay
                HIPCHK(prf_lit_sort_unique(c->stream, rows.p, n, uniq.p, d_n, &c->lit_scratch, &c->lit_scratch_bytes));
                HIPCHK(hipMemcpyAsync(h, d_n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                const u64 kept = h[0];
                if (kept > n) return fail(PRF_EHIP, "prf_scan_literal: row compaction returned %llu of %llu rows", (unsigned long long)kept,
                                          (unsigned long long)n);
                const size_t at = rows_out.size();
                rows_out.resize(at + kept);
                if (kept) {
                    HIPCHK(hipMemcpyAsync(rows_out.data() + at, uniq.p, kept * sizeof(prf_hit), hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(hipStreamSynchronize(c->stream));
                }
                for (size_t r = at; r < rows_out.size(); r++) {
                    rows_out[r].start += front;
                    rows_out[r].end += front;
                }
                *launches += 5;
            }
            return PRF_OK;
        }
        if (attempt >= 2) return fail(PRF_EHIP, "prf_scan_literal: the row count changed between two runs");
        cap = n;
    }
}

static int literal_one(prf_ctx *c, const prf_contig &ct, u32 contig_index, u32 kmin, u32 kmax, u32 min_repeats, u32 min_span,
                       u64 stop, std::vector<prf_hit> &rows_out, float *ms, u32 *launches, u64 front) {
    const u64 L = ct.len;
    if (L && !ct.ascii) return fail(PRF_EINVAL, "prf_scan_literal: NULL sequence");
    if (L >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "prf_scan_literal: input too large (2^40 positions)");
    dev_array<uint8_t> seq;
    if (const int rc = seq.alloc(L + 16)) return rc;
    if (L) HIPCHK(hipMemcpyAsync(seq.p, ct.ascii, L, hipMemcpyHostToDevice, c->stream));
    return literal_device(c, seq.p, L, true, contig_index, kmin, kmax, min_repeats, min_span, stop, rows_out, ms, launches, front);
}

// what the literal lane refuses on a context: a row sink, pipelined scans in flight
static int literal_preamble(const prf_ctx *c, const char *api) {
    if (c->sink) return fail(PRF_EUNSUPPORTED, "min_repeats == 1: not with a row sink (the rows of the literal lane are handed over on the host)");
    return refuse_in_flight(c, api);
}

static int literal_finish(prf_ctx *c, std::vector<prf_hit> &rows, float ms, u32 launches, u64 positions, prf_hits *out,
                          prf_scan_stats *stats) {
    c->last.nhits = 0;  // the rows of this lane live on the host only
    c->last.rows = nullptr;
    lane_stats(stats, 2, ms, positions, positions, launches);  // packed_bytes: this lane reads the bytes themselves
    if (stats) stats->n_candidates = stats->n_hits = rows.size();
    if (!out || rows.empty()) return PRF_OK;
    prf_hit *r = (prf_hit *)malloc(rows.size() * sizeof(prf_hit));
    if (!r) return fail(PRF_ENOMEM, "prf_scan_literal: cannot allocate %zu rows", rows.size());
    memcpy(r, rows.data(), rows.size() * sizeof(prf_hit));
    out->rows = r;
    out->n = rows.size();
    return PRF_OK;
}

// min_repeats == 1 on a RESIDENT genome: the upper-cased bytes of every contig are rebuilt on the device from the linear
// planes (H, L, X and the code planes of the symbols outside ACGTN), trimmed of the N at both ends (reference
// perfect_repeat_finder.py:40-46) and handed to the literal lane -- nothing crosses PCIe but the rows.
static int literal_genome(prf_ctx *c, const prf_genome *g, u32 kmin, u32 kmax, u32 min_repeats, u32 min_span, prf_hits *out,
                          prf_scan_stats *stats) {
    if (g->sel_on)
        return fail(PRF_EUNSUPPORTED, "min_repeats == 1 scans whole contigs (its rows depend on where a sequence begins and ends): "
                                      "clear the selection of parts (prf_genome_select with n_parts == 0)");
    const int rc = literal_preamble(c, "prf_scan_genome");
    if (rc) return rc;
    std::vector<prf_hit> rows;
    float ms = 0;
    u32 launches = 0;
    for (size_t ci = 0; ci < g->len.size(); ci++) {
        const u64 len = g->len[ci];
        u64 lo = len, hi = len;  // nothing but N (or empty): the reference's window is seq[len:len]
        if (len) {
            u64 fl[2] = {~0ull, 0ull};
            HIPCHK(hipMemcpyAsync(c->d_counters, fl, sizeof fl, hipMemcpyHostToDevice, c->stream));
            HIPCHK(prf_launch_lit_trim(c->stream, g->X, g->E, g->base[ci] >> 6, len, c->d_counters));
            HIPCHK(hipMemcpyAsync(c->h_counters, c->d_counters, sizeof fl, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            launches++;
            if (c->h_counters[0] != ~0ull) { lo = c->h_counters[0]; hi = c->h_counters[1]; }
        }
        const u64 n = hi - lo;
        dev_array<uint8_t> seq;
        if (const int rc = seq.alloc(n + 16)) return rc;
        if (n) {
            HIPCHK(prf_launch_lit_unpack(c->stream, g->H, g->L, g->X, g->E, g->base[ci] + lo, n, seq.p));
            launches++;
        }
        const int rc = literal_device(c, seq.p, n, false, (u32)ci, kmin, kmax, min_repeats, min_span, n, rows, &ms, &launches, lo);
        if (rc) return rc;
    }
    return literal_finish(c, rows, ms, launches, g->positions, out, stats);
}

static int literal_impl(prf_ctx *c, const prf_contig *contigs, int n_contigs, const u64 *stops, u32 kmin, u32 kmax, u32 min_repeats,
                        u32 min_span, prf_hits *out, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "prf_scan_literal: NULL context");
    if (out) { out->rows = nullptr; out->n = 0; }
    if (n_contigs < 0 || (n_contigs && !contigs)) return fail(PRF_EINVAL, "prf_scan_literal: bad contig array");
    int rc = check_params(kmin, kmax, min_repeats, min_span, 0);
    if (!rc) rc = literal_preamble(c, "prf_scan_literal");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->dev));
    std::vector<prf_hit> rows;
    float ms = 0;
    u32 launches = 0;
    u64 positions = 0;
    for (int i = 0; i < n_contigs; i++) {
        prf_contig w = contigs[i];
        u64 lo = 0;
        if (!stops && w.len) {
            // prf_scan: the whole of reference detect_repeats() without an interval, whose :40-46 drop the N at both ends
            // first -- not a no-op in this regime, the rows depend on where the sequence begins and ends
            if (!w.ascii) return fail(PRF_EINVAL, "prf_scan: NULL sequence");
            u64 hi = w.len;
            while (lo < hi && (w.ascii[lo] | 0x20) == 'n') lo++;
            while (hi > lo && (w.ascii[hi - 1] | 0x20) == 'n') hi--;
            w.ascii += lo;
            w.len = hi - lo;
        }
        rc = literal_one(c, w, (u32)i, kmin, kmax, min_repeats, min_span, stops ? stops[i] : w.len, rows, &ms, &launches, lo);
        if (rc) return rc;
        positions += contigs[i].len;
    }
    return literal_finish(c, rows, ms, launches, positions, out, stats);
}

int prf_scan_literal(prf_ctx *c, const prf_contig *contig, uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span,
                     uint64_t stop, prf_hits *out, prf_scan_stats *stats) {
    if (!contig) return fail(PRF_EINVAL, "prf_scan_literal: NULL contig");
    const u64 stop_ = stop;
    return guarded("prf_scan_literal", [&] { return literal_impl(c, contig, 1, &stop_, kmin, kmax, min_repeats, min_span, out, stats); });
}

int prf_scan(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
             uint32_t min_span, uint32_t flags, prf_hits *out, prf_scan_stats *stats) {
    if (min_repeats == 1)  // outside the closed form of the packed kernels: the literal lane, contig by contig
        return guarded("prf_scan", [&] { return literal_impl(c, contigs, n_contigs, nullptr, kmin, kmax, min_repeats, min_span, out, stats); });
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
            HIPCHK(hipHostMalloc((void **)&c->h_async, (PRF_CNT_N + 8) * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
            memset(c->h_async, 0, (PRF_CNT_N + 8) * sizeof(u64));
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
    const int rc = launch_fused(c, g, plan, min_repeats, min_span, sl.rows, c->hit_cap, 0u, sl.h_dev, &seq);
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
        const hipError_t e = prf_launch_pack_rows_dev(c->stream, rows, counters + PRF_CNT_ROWS, capacity_rows, g->d_base,
                                                      (u64 *)dst_device, side_capacity, c->d_side_cnt);
        if (e == hipSuccess) return PRF_OK;
        (void)retire_slot(c, *slot_of(c, *seq_out), true);
        return fail(e == hipErrorOutOfMemory ? PRF_ENOMEM : PRF_EHIP, "prf_launch_pack_rows_dev failed: %s", hipGetErrorString(e));
    });
}

// Everything enqueued on the library's stream so far happens before whatever is enqueued on `other_stream` (a hipStream_t)
// from now on: the hand-off of a send buffer to a communication stream without a host wait.
int prf_stream_wait_for(prf_ctx *c, void *other_stream) {
    if (!c) return fail(PRF_EINVAL, "prf_stream_wait_for: NULL context");
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipEventRecord(c->ev_handoff, c->stream));
    HIPCHK(hipStreamWaitEvent((hipStream_t)other_stream, c->ev_handoff, 0));
    return PRF_OK;
}

int prf_scan_wait(prf_ctx *c, uint64_t seq, prf_scan_stats *stats) {
    if (!c || !seq) return fail(PRF_EINVAL, "prf_scan_wait: bad arguments");
    prf_ctx::async_slot *sl = slot_of(c, seq);
    if (!sl) return fail(PRF_EINVAL, "prf_scan_wait: scan %llu is not in flight", (unsigned long long)seq);
    const int rc = retire_slot(c, *sl, false);
    if (rc) return rc;
    const pass_result r = read_fused(sl->h);
    if (sl->h[PRF_CNT_HIT_OVF] > c->slab_cap || r.nhits > c->hit_cap || sl->h[PRF_CNT_LONG_OVF])
        return fail(PRF_EUNSUPPORTED, "prf_scan_wait: the buffers sized by the last synchronous scan overflowed; scan synchronously");
    c->last = {sl->rows, r.nhits, sl->kmax};
    if (stats) fill_stats(stats, r, 1, sl->positions, sl->tiles, seq);
    return PRF_OK;
}

int prf_set_row_sink(prf_ctx *c, void *dst_device, uint64_t capacity_rows) {
    if (!c) return fail(PRF_EINVAL, "prf_set_row_sink: NULL context");
    c->sink = (prf_hit_dev *)dst_device;
    c->sink_cap = dst_device ? capacity_rows : 0;
    return PRF_OK;
}

int prf_last_hits_to_device(prf_ctx *c, void *dst, uint64_t capacity_rows, int count_row, uint64_t *n_rows) {
    if (!c || !n_rows || ((capacity_rows || count_row) && !dst)) return fail(PRF_EINVAL, "prf_last_hits_to_device: bad arguments");
    HIPCHK(hipSetDevice(c->dev));
    *n_rows = c->last.nhits;
    const u64 n = std::min<u64>(c->last.nhits, capacity_rows);
    if (n && dst != (void *)c->last.rows)
        HIPCHK(hipMemcpyAsync(dst, c->last.rows, n * sizeof(prf_hit_dev), hipMemcpyDeviceToDevice, c->stream));
    if (count_row) return write_count_record(c, (prf_hit_dev *)dst, capacity_rows, n);
    if (n) HIPCHK(hipStreamSynchronize(c->stream));
    return PRF_OK;
}

uint64_t prf_tile_positions(void) { return PRF_TILE; }

int prf_genome_tile_classes(const prf_genome *g, uint32_t contig, uint8_t *dst, uint64_t capacity, uint64_t *n_tiles) {
    if (!g || !n_tiles || contig >= g->base.size() || (capacity && !dst)) return fail(PRF_EINVAL, "prf_genome_tile_classes: bad arguments");
    const u64 t0 = g->base[contig] / PRF_TILE, n = (g->len[contig] + PRF_TILE - 1) / PRF_TILE;
    *n_tiles = n;
    for (u64 i = 0; i < n && i < capacity; i++) dst[i] = g->vp.h_class[t0 + i];
    return PRF_OK;
}

static int genome_select_impl(prf_genome *g, const prf_part *parts, int n_parts) {
    if (!g || n_parts < 0 || (n_parts > 0 && !parts)) return fail(PRF_EINVAL, "prf_genome_select: bad arguments");
    prf_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipStreamSynchronize(c->stream));  // no scan of this genome may be reading the old selection
    if (n_parts == 0) {
        g->sel_on = false;
        return PRF_OK;
    }
    std::vector<std::pair<u64, u64>> tr;
    u64 positions = 0;
    for (int i = 0; i < n_parts; i++) {
        const prf_part &p = parts[i];
        if (p.contig >= g->base.size()) return fail(PRF_EINVAL, "prf_genome_select: part %d names contig %u of %zu", i, p.contig, g->base.size());
        const u64 len = g->len[p.contig];
        const u64 end = std::min<u64>(p.end, len);
        if (p.begin % PRF_TILE != 0 || (end % PRF_TILE != 0 && end != len) || p.begin > end)
            return fail(PRF_EINVAL, "prf_genome_select: part %d [%llu, %llu) of contig %u must begin on a multiple of %u and end on one or at "
                        "the contig's end", i, (unsigned long long)p.begin, (unsigned long long)p.end, p.contig, PRF_TILE);
        if (end == p.begin) continue;
        const u64 t0 = g->base[p.contig] / PRF_TILE;
        tr.emplace_back(t0 + p.begin / PRF_TILE, t0 + (end + PRF_TILE - 1) / PRF_TILE);
        positions += end - p.begin;
    }
    std::sort(tr.begin(), tr.end());
    std::vector<std::pair<u64, u64>> merged;
    for (const auto &r : tr) {
        if (!merged.empty() && r.first < merged.back().second)
            return fail(PRF_EINVAL, "prf_genome_select: parts overlap");
        if (!merged.empty() && r.first == merged.back().second) merged.back().second = r.second;
        else merged.push_back(r);
    }
    std::vector<u32> list;
    {
        const std::vector<u32> &all = g->vp.h_list;  // ascending by tile
        size_t i = 0;
        for (const auto &r : merged) {
            while (i < all.size() && (all[i] & ~PRF_LAUNCH_MIXED) < r.first) i++;
            while (i < all.size() && (all[i] & ~PRF_LAUNCH_MIXED) < r.second) list.push_back(all[i++]);
        }
    }
    if (!g->d_sel_list) HIPCHK(hipMalloc((void **)&g->d_sel_list, sizeof(u32) * std::max<size_t>(1, g->vp.h_list.size())));
    if (!list.empty()) HIPCHK(hipMemcpy(g->d_sel_list, list.data(), sizeof(u32) * list.size(), hipMemcpyHostToDevice));
    g->sel_n = (u32)list.size();
    g->sel_flat = prf_flat_base(list.data(), list.size());
    g->sel_positions = positions;
    g->sel_tiles = std::move(merged);
    g->sel_on = true;
    return PRF_OK;
}

int prf_genome_select(prf_genome *g, const prf_part *parts, int n_parts) {
    return guarded("prf_genome_select", [&] { return genome_select_impl(g, parts, n_parts); });
}

int prf_last_hits_packed_to_device(prf_ctx *c, const prf_genome *g, void *dst, uint64_t capacity_rows, uint64_t side_capacity,
                                   uint64_t *n_rows) {
    if (!c || !g || g->ctx != c || !n_rows || !dst) return fail(PRF_EINVAL, "prf_last_hits_packed_to_device: bad arguments");
    HIPCHK(hipSetDevice(c->dev));
    *n_rows = c->last.nhits;
    if (c->last.kmax > 511u)  // (such rows used to leave with a truncated motif size)
        return fail(PRF_EUNSUPPORTED, "the 8-byte wire rows hold motif sizes up to 511; the last scan went up to %u -- hand its rows over whole "
                    "(prf_last_hits_to_device)", c->last.kmax);
    if (c->last.nhits > capacity_rows)
        return fail(PRF_EINVAL, "the packed row buffer holds %llu rows, the scan found %llu", (unsigned long long)capacity_rows,
                    (unsigned long long)c->last.nhits);
    u64 *words = (u64 *)dst;
    // (a spare device word: the generic path's counters are idle here; spare pinned words behind the counter block,
    // written by the device)
    u64 *side_cnt = c->d_counters + PRF_CNT_CAND;
    HIPCHK(hipMemsetAsync(side_cnt, 0, sizeof(u64), c->stream));
    volatile u64 *stage = c->h_counters + PRF_CNT_N + 2;
    HIPCHK(prf_launch_pack_rows(c->stream, c->last.rows, c->last.nhits, g->d_base, words, capacity_rows, side_capacity, side_cnt,
                                c->h_counters_dev + PRF_CNT_N + 2));
    HIPCHK(hipStreamSynchronize(c->stream));
    const u64 n_side = stage[0];
    if (n_side > side_capacity)
        return fail(PRF_EINVAL, "the side list holds %llu rows, %llu rows are longer than 65534", (unsigned long long)side_capacity,
                    (unsigned long long)n_side);
    return PRF_OK;
}

int prf_genome_contig_bases(const prf_genome *g, uint64_t *bases, uint64_t capacity, uint64_t *n_contigs) {
    if (!g || !n_contigs || (capacity && !bases)) return fail(PRF_EINVAL, "prf_genome_contig_bases: bad arguments");
    *n_contigs = g->base.size();
    for (size_t i = 0; i < g->base.size() && i < capacity; i++) bases[i] = g->base[i];
    return PRF_OK;
}

int prf_genome_footprint(const prf_genome *g, uint64_t *device_bytes, uint64_t *positions) {
    if (!g || !device_bytes || !positions) return fail(PRF_EINVAL, "prf_genome_footprint: bad arguments");
    const u64 tot = PRF_FRONT_PAD + g->nwords + g->padw;      // words of one linear plane (alloc_plane)
    const u64 ntiles = g->G / PRF_TILE;
    u64 bytes = 3 * tot * 8;                                   // H, L, X
    if (g->d_E) bytes += 5 * tot * 8 + 5 * sizeof(u64 *);      // the code planes of the letters outside ACGTN
    bytes += 2 * ntiles * (PRF_TILE / 8);                      // VH, VL
    bytes += 2 * ntiles + sizeof(u32) * ntiles;                // tile classes (+ scratch), launch list
    bytes += sizeof(uint4) * ntiles + sizeof(u64) * std::max<size_t>(1, g->base.size());  // tile table, contig bases
    if (g->d_sel_list) bytes += sizeof(u32) * std::max<size_t>(1, g->vp.h_list.size());
    *device_bytes = bytes;
    *positions = g->G;
    return PRF_OK;
}

int prf_plan_describe(uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span, char *buf, uint64_t buf_len) {
    if (!buf || buf_len == 0) return fail(PRF_EINVAL, "prf_plan_describe: no buffer");
    const int n = prf_plan_json(kmin, kmax, min_repeats, min_span, buf, buf_len);
    if (n < 0) return fail(PRF_EINVAL, "prf_plan_describe: buffer too small");
    return n;
}

void prf_free_hits(prf_hits *h) {
    if (!h) return;
    free(h->rows);
    h->rows = nullptr;
    h->n = 0;
}

int prf_measure_hbm_read(prf_ctx *c, uint64_t bytes, int iters, double *gbps) {
    if (!c || !gbps || bytes < (1u << 20) || iters < 1) return fail(PRF_EINVAL, "prf_measure_hbm_read: bad arguments");
    HIPCHK(hipSetDevice(c->dev));
    bytes &= ~(uint64_t)15;
    void *buf = nullptr;
    u32 *sink = nullptr;
    HIPCHK(hipMalloc(&buf, bytes));
    hipError_t e = hipMalloc((void **)&sink, 64);
    if (e != hipSuccess) { (void)hipFree(buf); return fail(PRF_ENOMEM, "hipMalloc failed"); }
    (void)hipMemsetAsync(buf, 0x5A, bytes, c->stream);
    float best = 1e30f;
    for (int i = 0; i < iters + 1; i++) {  // first pass is a warm-up
        (void)hipEventRecord(c->ev[0], c->stream);
        (void)prf_launch_hbm_read(c->stream, buf, bytes, sink);
        (void)hipEventRecord(c->ev[1], c->stream);
        (void)hipStreamSynchronize(c->stream);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
        if (i > 0 && ms < best) best = ms;
    }
    (void)hipFree(buf);
    (void)hipFree(sink);
    *gbps = (double)bytes / (best * 1e-3) / 1e9;
    return PRF_OK;
}

}  // extern "C"
