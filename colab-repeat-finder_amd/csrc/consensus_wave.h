// consensus_wave.h -- what a wave of the count kernels of consensus.hip and phased.hip brings to the per-lane text
// of consensus_word.h and phased_word.h: the source of plane words and the fence of the wave's LDS region.  Device only; the two
// .hip files include it and nobody else.  No address into the planes is formed in the kernels but in cs_wave_source::take.
#pragma once
#include "consensus_word.h"

namespace {

// cs_count_item's source: the words of the planes, 64 at a time.  `last` is the last word that holds a position of the item;
// every lane of the wave calls take with the same w.
struct cs_wave_source {
    const prf_planes &pl;
    const u64 last;
    const u32 lane;
    u64 base = 0;
    bool loaded = false;
    u64 mine[3] = {0, 0, 0};
    __device__ __forceinline__ void take(u64 w, u64 *out) {
        if (!loaded || w - base >= 64ull) {
            base = w;
            loaded = true;
            const u64 my = w + lane;
            const bool in = my <= last;
            mine[0] = in ? pl.H[my] : 0ull;
            mine[1] = in ? pl.L[my] : 0ull;
            mine[2] = in ? pl.X[my] : 0ull;
        }
#pragma unroll
        for (int p = 0; p < 3; p++) out[p] = __shfl(mine[p], (int)(w - base));
    }
};

// between the phases of a wave's LDS region: what the lanes wrote is what the lanes read
__device__ __forceinline__ void cs_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
