// phased.hip -- the column counts of consensus rows whose positions come as SEGMENTS WITH A PHASE (DESIGN 19;
// include/prf_phased.h): position q of a segment (start, end, row, phase) lies in column (phase + q - start) mod k of its row.
// The host cuts the segments into work items of at most slice_positions positions and sorts the items by the regime of their
// row's k; the per-lane text of an item is ph_count_item of phased_word.h.
//
// prf_phased_count_kernel, one wave per item, is prf_consensus_count_kernel of consensus.hip with the item's first column taken
// from its segment: the same source of plane words (cs_wave_source: every word that holds a position of the item loaded once, as
// a whole word, and no other), the same three regimes by the row's k (registers up to 64, the wave's LDS region up to 1024,
// global adds above).  Several segments of a row, and several items of a segment, meet only in the global counts, through the
// same adds.  The letters and the sums are prf_consensus_finish_kernel's.
// No address into the planes is formed here but in cs_wave_source::take.
#include "../../include/prf.h"
#include "phased_launch.h"
#include "consensus_wave.h"

#define PH_THREADS 256
#define PH_WAVES (PH_THREADS / 64)

static_assert(sizeof(prf_segment) == 24 && sizeof(ph_segment) == sizeof(prf_segment) && sizeof(ph_item) == 24, "the segments and the items");
static_assert(PRF_CS_REG_K == 64u && PRF_CS_LDS_K > 64u, "the lanes of a step of k > 64 hit different columns");

namespace {

template <int REGIME>
__global__ __launch_bounds__(PH_THREADS) void prf_phased_count_kernel(const prf_phased_args a, const u64 item0, const u64 n_items) {
    extern __shared__ __attribute__((aligned(16))) u32 ph_lds[];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 at = (u64)blockIdx.x * PH_WAVES + wave;
    if (at >= n_items) return;                                                 // the whole wave
    const ph_item it = a.items[item0 + at];
    if (it.segment >= a.n_segments) return;
    const ph_segment sg = a.segments[it.segment];
    if (sg.row >= a.n_rows) return;
    const cs_row r = a.rows[sg.row];
    if (!r.k || sg.phase >= r.k || it.first < sg.start || it.first >= it.end || it.end > sg.end) return;
    cs_wave_source src{a.pl, (a.g_begin + it.end - 1ull) >> 6, lane};
    u32 *const out = a.counts + 4ull * r.offset;
    if (REGIME == PRF_CS_REG) {
        u32 c[4] = {0, 0, 0, 0};
        ph_count_item(src, a.g_begin, r.k, sg, it, lane, [&](u32, u32 b) {
#pragma unroll
            for (u32 i = 0; i < 4; i++) c[i] += b == i ? 1u : 0u;
        });
        // the lanes of one column are x, x + k, x + 2 k, ... below the step
        const u32 copies = 64u / r.k;
        const u32 own[4] = {c[0], c[1], c[2], c[3]};
#pragma unroll 1
        for (u32 j = 1; j < copies; j++) {
#pragma unroll
            for (u32 i = 0; i < 4; i++) c[i] += (u32)__shfl((int)own[i], (int)((lane + j * r.k) & 63u));
        }
        if (lane < r.k) {
            const u32 col = ph_lane_column(sg, r.k, it, lane);
#pragma unroll
            for (u32 i = 0; i < 4; i++)
                if (c[i]) atomicAdd(out + 4u * col + i, c[i]);
        }
    } else if (REGIME == PRF_CS_LDS) {
        u32 *const my = ph_lds + wave * 4u * PRF_CS_LDS_K;
        // the columns the item touches: min(k, its positions) of them from the column of its first position
        const u64 len = it.end - it.first;
        const u32 n_cols = len < (u64)r.k ? (u32)len : r.k;
        const u32 col0 = ph_first_column(sg, r.k, it);
        for (u32 i = lane; i < 4u * n_cols; i += 64u) {
            u32 col = col0 + (i >> 2);
            if (col >= r.k) col -= r.k;
            __hip_atomic_store(my + 4u * col + (i & 3u), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        cs_lds_fence();
        // the lanes of a step hit different columns, the steps of a wave follow one another: an add without a result will do
        ph_count_item(src, a.g_begin, r.k, sg, it, lane, [&](u32 col, u32 b) {
            (void)__hip_atomic_fetch_add(my + 4u * col + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        });
        cs_lds_fence();
        for (u32 i = lane; i < 4u * n_cols; i += 64u) {
            u32 col = col0 + (i >> 2);
            if (col >= r.k) col -= r.k;
            const u32 v = __hip_atomic_load(my + 4u * col + (i & 3u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (v) atomicAdd(out + 4ull * col + (i & 3u), v);
        }
    } else {
        ph_count_item(src, a.g_begin, r.k, sg, it, lane, [&](u32 col, u32 b) { atomicAdd(out + 4ull * col + b, 1u); });
    }
}

}  // namespace

hipError_t prf_launch_phased_count(hipStream_t st, const prf_phased_args &a, u32 regime, u64 item0, u64 n_items) {
    if (!n_items) return hipSuccess;
    const u64 blocks = (n_items + PH_WAVES - 1) / PH_WAVES;
    if (blocks > 0x7fffffffull || regime >= PRF_CS_REGIMES || !a.rows || !a.segments || !a.items || !a.counts) return hipErrorInvalidValue;
    const dim3 grid((u32)blocks);
    if (regime == PRF_CS_REG) hipLaunchKernelGGL((prf_phased_count_kernel<PRF_CS_REG>), grid, dim3(PH_THREADS), 0, st, a, item0, n_items);
    else if (regime == PRF_CS_LDS)
        hipLaunchKernelGGL((prf_phased_count_kernel<PRF_CS_LDS>), grid, dim3(PH_THREADS), PH_WAVES * 4u * PRF_CS_LDS_K * sizeof(u32), st, a, item0, n_items);
    else hipLaunchKernelGGL((prf_phased_count_kernel<PRF_CS_GLOBAL>), grid, dim3(PH_THREADS), 0, st, a, item0, n_items);
    return hipGetLastError();
}
