// context.cpp -- the part of the C ABI (include/prf.h) that belongs to no lane: the error text, contexts and what they own, the
// hand-off of the library's stream to a stream of the caller's, and the small queries (tile size, plan, HBM read rate).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "prf_ctx.h"
#include "prf_plan.h"

static thread_local std::string g_err;

int prf_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
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
    HIPCHK(hipHostMalloc((void **)&c->h_counters, PRF_CNT_BLOCK_WORDS * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
    // recycled pinned blocks are not zeroed, and the scan serial numbers restart at 1 for every context: a stale
    // serial number left by a closed context must never look like a finished scan
    memset(c->h_counters, 0, PRF_CNT_BLOCK_WORDS * sizeof(u64));
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

// Everything enqueued on the library's stream so far happens before whatever is enqueued on `other_stream` (a hipStream_t)
// from now on: the hand-off of a send buffer to a communication stream without a host wait.
int prf_stream_wait_for(prf_ctx *c, void *other_stream) {
    if (!c) return fail(PRF_EINVAL, "prf_stream_wait_for: NULL context");
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipEventRecord(c->ev_handoff, c->stream));
    HIPCHK(hipStreamWaitEvent((hipStream_t)other_stream, c->ev_handoff, 0));
    return PRF_OK;
}

void prf_free_hits(prf_hits *h) {
    if (!h) return;
    free(h->rows);
    h->rows = nullptr;
    h->n = 0;
}

uint64_t prf_tile_positions(void) { return PRF_TILE; }

int prf_plan_describe(uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span, char *buf, uint64_t buf_len) {
    if (!buf || buf_len == 0) return fail(PRF_EINVAL, "prf_plan_describe: no buffer");
    const int n = prf_plan_json(kmin, kmax, min_repeats, min_span, buf, buf_len);
    if (n < 0) return fail(PRF_EINVAL, "prf_plan_describe: buffer too small");
    return n;
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
