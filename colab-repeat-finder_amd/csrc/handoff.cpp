// handoff.cpp -- the rows of a scan handed to device memory the caller owns: a row sink the scans write into, the last scan's
// rows copied whole, or packed to 8-byte wire words.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "genome.h"

// The count record {n, 0, 0} behind a caller-owned row array (dst[cap]), staged in the spare pinned words behind the counter
// block.  Returns when it is on the device.
int prf_write_count_record(prf_ctx *c, prf_hit_dev *dst, u64 cap, u64 n) {
    u64 *stage = c->h_counters + PRF_CNT_SPARE;
    stage[0] = n; stage[1] = 0; stage[2] = 0;
    HIPCHK(hipMemcpyAsync(dst + cap, stage, sizeof(prf_hit_dev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PRF_OK;
}

extern "C" {

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
    if (count_row) return prf_write_count_record(c, (prf_hit_dev *)dst, capacity_rows, n);
    if (n) HIPCHK(hipStreamSynchronize(c->stream));
    return PRF_OK;
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
    volatile u64 *stage = c->h_counters + PRF_CNT_SPARE;
    HIPCHK(prf_launch_pack_rows(c->stream, c->last.rows, c->last.nhits, g->d_base, words, capacity_rows, side_capacity, side_cnt,
                                c->h_counters_dev + PRF_CNT_SPARE));
    HIPCHK(hipStreamSynchronize(c->stream));
    const u64 n_side = stage[0];
    if (n_side > side_capacity)
        return fail(PRF_EINVAL, "the side list holds %llu rows, %llu rows are longer than 65534", (unsigned long long)side_capacity,
                    (unsigned long long)n_side);
    return PRF_OK;
}

}  // extern "C"
