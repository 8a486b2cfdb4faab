// consensus.hip -- the consensus motif of each of a list of tandem repeats (start, end, k) of ONE range, column by column
// (include/prf_consensus.h).  The host cuts the rows into work items of at most slice_positions positions and sorts
// the items by regime; the per-lane text of an item is cs_count_item of consensus_word.h.
//
// prf_consensus_count_kernel, one wave per item.  The 64 lanes load 64 words of each of H, L, X at a time, lane j word base + j
// (cs_wave_source), and hand them round with a shuffle: every word of the planes that holds a position of the item is loaded
// once, as a whole word, and no other word is.  Adjacent lanes take adjacent positions.  Three regimes, by the row's k:
//   k <= 64 (PRF_CS_REG_K)     a step covers floor(64 / k) k positions, so a lane's column never changes: four counters in
//                              registers, folded over the lanes of equal column by shuffles, then one add per (column, base)
//                              that is not 0
//   k <= 1024 (PRF_CS_LDS_K)   the counters of the columns the item touches live in the wave's own LDS region; the 64 lanes of
//                              a step hit 64 different columns, so the adds (LDS adds without a result) never meet; at the
//                              end the wave sweeps the columns it touched: one add per (column, base) that is not 0
//   larger k                   the adds of a step go straight to the global counts: 64 different columns per step
// prf_consensus_finish_kernel, one wave per row: the letter of every column, and agree and acgt by a wave reduction.
// No address into the planes is formed here but in cs_wave_source::take (consensus_wave.h, shared with phased.hip).
#include "../../include/prf.h"
#include "consensus_launch.h"
#include "consensus_wave.h"

#define CS_THREADS 256
#define CS_WAVES (CS_THREADS / 64)

static_assert(sizeof(prf_consensus_dev) == sizeof(prf_consensus) && sizeof(prf_consensus) == 32, "prf_consensus is 32 bytes");
static_assert(sizeof(prf_repeat) == 24 && sizeof(cs_row) == 32 && sizeof(cs_item) == 24, "the rows and the items");
static_assert(PRF_CS_REG_K == 64u && PRF_CS_LDS_K > 64u, "the lanes of a step of k > 64 hit different columns");

namespace {

template <int REGIME>
__global__ __launch_bounds__(CS_THREADS) void prf_consensus_count_kernel(const prf_consensus_args a, const u64 item0, const u64 n_items) {
    extern __shared__ __attribute__((aligned(16))) u32 cs_lds[];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 at = (u64)blockIdx.x * CS_WAVES + wave;
    if (at >= n_items) return;                                                 // the whole wave
    const cs_item it = a.items[item0 + at];
    if (it.row >= a.n_rows) return;
    const cs_row r = a.rows[it.row];
    cs_wave_source src{a.pl, (a.g_begin + it.end - 1ull) >> 6, lane};
    u32 *const out = a.counts + 4ull * r.offset;
    if (REGIME == PRF_CS_REG) {
        u32 c[4] = {0, 0, 0, 0};
        cs_count_item(src, a.g_begin, r, it, lane, [&](u32, u32 b) {
#pragma unroll
            for (u32 i = 0; i < 4; i++) c[i] += b == i ? 1u : 0u;
        });
        // the lanes of column x are x, x + k, x + 2 k, ... below the step
        const u32 copies = 64u / r.k;
        const u32 own[4] = {c[0], c[1], c[2], c[3]};
#pragma unroll 1
        for (u32 j = 1; j < copies; j++) {
#pragma unroll
            for (u32 i = 0; i < 4; i++) c[i] += (u32)__shfl((int)own[i], (int)((lane + j * r.k) & 63u));
        }
        if (lane < r.k) {
            const u32 col = cs_lane_column(r, it, lane);
#pragma unroll
            for (u32 i = 0; i < 4; i++)
                if (c[i]) atomicAdd(out + 4u * col + i, c[i]);
        }
    } else if (REGIME == PRF_CS_LDS) {
        u32 *const my = cs_lds + wave * 4u * PRF_CS_LDS_K;
        // the columns the item touches: min(k, its positions) of them from the column of its first position
        const u64 len = it.end - it.first;
        const u32 n_cols = len < (u64)r.k ? (u32)len : r.k;
        const u32 col0 = (u32)((it.first - r.start) % r.k);
        for (u32 i = lane; i < 4u * n_cols; i += 64u) {
            u32 col = col0 + (i >> 2);
            if (col >= r.k) col -= r.k;
            __hip_atomic_store(my + 4u * col + (i & 3u), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        cs_lds_fence();
        // the lanes of a step hit different columns, the steps of a wave follow one another: an add without a result will do
        cs_count_item(src, a.g_begin, r, it, lane, [&](u32 col, u32 b) {
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
        cs_count_item(src, a.g_begin, r, it, lane, [&](u32 col, u32 b) { atomicAdd(out + 4ull * col + b, 1u); });
    }
}

__global__ __launch_bounds__(CS_THREADS) void prf_consensus_finish_kernel(const prf_consensus_args a) {
    const u32 lane = threadIdx.x & 63u;
    const u64 row = (u64)blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;                                               // the whole wave
    const cs_row r = a.rows[row];
    const uint4 *const counts = reinterpret_cast<const uint4 *>(a.counts) + r.offset;   // 16 bytes per column
    char *const motif = a.motifs + r.offset;
    u64 agree = 0, acgt = 0;
    for (u32 p = lane; p < r.k; p += 64u) {
        const uint4 v = counts[p];
        const u32 count[4] = {v.x, v.y, v.z, v.w};
        u32 best;
        motif[p] = cs_consensus(count, &best);
        agree += best;
        acgt += (u64)v.x + v.y + v.z + v.w;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) agree += __shfl_xor(agree, d), acgt += __shfl_xor(acgt, d);
    if (lane == 0) a.dst[row] = prf_consensus_dev{r.offset, agree, acgt, r.k, 0u};
}

}  // namespace

hipError_t prf_launch_consensus_count(hipStream_t st, const prf_consensus_args &a, u32 regime, u64 item0, u64 n_items) {
    if (!n_items) return hipSuccess;
    const u64 blocks = (n_items + CS_WAVES - 1) / CS_WAVES;
    if (blocks > 0x7fffffffull || regime >= PRF_CS_REGIMES || !a.rows || !a.items || !a.counts) return hipErrorInvalidValue;
    const dim3 grid((u32)blocks);
    if (regime == PRF_CS_REG) hipLaunchKernelGGL((prf_consensus_count_kernel<PRF_CS_REG>), grid, dim3(CS_THREADS), 0, st, a, item0, n_items);
    else if (regime == PRF_CS_LDS)
        hipLaunchKernelGGL((prf_consensus_count_kernel<PRF_CS_LDS>), grid, dim3(CS_THREADS), CS_WAVES * 4u * PRF_CS_LDS_K * sizeof(u32), st, a, item0, n_items);
    else hipLaunchKernelGGL((prf_consensus_count_kernel<PRF_CS_GLOBAL>), grid, dim3(CS_THREADS), 0, st, a, item0, n_items);
    return hipGetLastError();
}

hipError_t prf_launch_consensus_finish(hipStream_t st, const prf_consensus_args &a) {
    if (!a.n_rows) return hipSuccess;
    const u64 blocks = (a.n_rows + CS_WAVES - 1) / CS_WAVES;
    if (blocks > 0x7fffffffull || !a.rows || !a.counts || !a.motifs || !a.dst) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prf_consensus_finish_kernel, dim3((u32)blocks), dim3(CS_THREADS), 0, st, a);
    return hipGetLastError();
}
