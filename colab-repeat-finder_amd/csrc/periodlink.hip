// periodlink.hip -- the junctions between the chains of periodchain.hip across neighbouring period lines of ONE range: "chain X
// ends here on line k_X, chain Y starts there on line k_Y" (include/prf_periodlink.h, whose words these comments use).
// The HEADS are the rows the kernels of periodchain.hip wrote at min_len = 0 for the window, left on the device.  A cell of line
// k is (i, c) = (t, t + k); the lines that take part are 1 .. n - 1, whatever the window's range of k is.
//
// prf_periodlink_join_kernel, the shape of prf_dotlink_join_kernel: one WAVE per head Y; lane l stands for the shift s = l - 32
// (l < 32) or l - 31: -32 .. -1, 1 .. 32.  Lanes with |s| > max_shift idle, and so do the lanes whose line is below 1 or above
// n - 1.
//   step A   lane s looks on the line k_Y - s for the chain's end in the stretch where (X, Y) is a candidate (pl_step_a:
//            dl_tail_in_stretch); the wave's minimum over the packed keys is pred(Y) = X.  No candidate: no link.
//   step B   X is wave-uniform.  Lane s' looks on the line k_X + s' for the chain's start in the stretch where (X, Y') is a
//            candidate, cut by key(X, Y) (pl_step_b: dl_head_in_stretch).  The wave's minimum is succ(X), or something larger
//            than key(X, Y).
//   emit     lane 0, iff the minimum is key(X, Y) and the head found on Y's line is Y: one atomic per emitting wave.
// Everything between the two minima is periodlink_step.h's, which runs on the host too.  A lane reads its line through pc_word
// (periodchain_word.h) over the planes in global memory, behind the one-word cache of the step.  No address into the planes is
// formed here but through pc_word's accessor.
#include "../../include/prf.h"
#include "prf_host.h"
#include "periodchain_word.h"
#include "periodlink_step.h"

#define PL_THREADS 256
#define PL_WAVES (PL_THREADS / 64)

static_assert(sizeof(prf_plink_dev) == sizeof(prf_plink) && sizeof(prf_plink) == 32, "prf_plink is 32 bytes");

namespace {

template <bool EXOTIC>
struct pl_global {            // pc_word's accessor: the planes in global memory
    const prf_planes &pl;
    __device__ __forceinline__ u64 h(u64 w) const { return pl.H[w]; }
    __device__ __forceinline__ u64 l(u64 w) const { return pl.L[w]; }
    __device__ __forceinline__ u64 x(u64 w) const { return pl.X[w]; }
    __device__ __forceinline__ u64 e(int i, u64 w) const { return pl.E[i][w]; }
    __device__ __forceinline__ bool exotic() const { return EXOTIC; }
};

__device__ __forceinline__ u32 pl_wave_min(u32 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)v, d);
        v = o < v ? o : v;
    }
    return v;
}

template <bool EXOTIC>
__global__ __launch_bounds__(PL_THREADS) void prf_periodlink_join_kernel(const prf_periodlink_args a) {
    const u32 lane = threadIdx.x & 63u;
    const u64 entry = (u64)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);
    if (entry >= a.n_heads) return;                                            // the whole wave
    const prf_pchain_dev y = a.heads[entry];
    const pl_global<EXOTIC> planes{a.pl};
    const pc_range range = pc_range_of(a.g_begin, a.n, a.n_matches);
    const pl_params p{a.n, a.min_seed, a.max_gap, a.max_shift};
    const auto line = [&](u64 k, u64 wk) { return pc_word(planes, range, k, wk); };

    // ---- step A: pred(Y)
    u64 x_end = 0;                                                             // t_e of this lane's candidate
    const u32 key = pl_step_a(p, y.start, (u64)y.k, lane, line, &x_end);
    const u32 best = pl_wave_min(key);
    if (best == PL_NO_KEY) return;                                             // no candidate: the whole wave
    const u32 y_lane = pl_key_lane(best);                                      // the lane of s_Y = k_Y - k_X
    const u64 t_e = (u64)__shfl(x_end, (int)y_lane);
    const u64 k_x = (u64)((pl_i64)y.k - (pl_i64)pl_key_shift(best));

    // ---- step B: succ(X)
    bool is_y = false;
    const u32 key_b = pl_step_b(p, t_e, k_x, lane, best, y.start, line, &is_y);
    const u32 next = pl_wave_min(key_b);
    const bool same = __shfl((int)is_y, (int)y_lane) != 0;
    if (next != best || !same) return;                                         // X prefers another chain
    if (lane == 0) {
        const u64 at = atomicAdd(a.counter, 1ull);
        if (at < a.capacity)
            a.dst[at] = prf_plink_dev{y.start, t_e, y.k, pl_key_shift(best), pl_key_most(best) - pl_key_abs_shift(best), pl_key_overlap(best)};
    }
}

}  // namespace

hipError_t prf_launch_periodlink_join(hipStream_t st, const prf_periodlink_args &a) {
    if (!a.n_heads) return hipSuccess;
    if (a.n_heads > PRF_PCHAIN_MAX_ROWS || !a.n || !a.min_seed || a.n_matches > 1u || a.max_gap > PRF_DOTCHAIN_MAX_GAP || !a.max_shift ||
        a.max_shift > PRF_DOTLINK_MAX_SHIFT || !a.heads || !a.counter || (a.capacity && !a.dst))
        return hipErrorInvalidValue;
    const dim3 grid((u32)((a.n_heads + PL_WAVES - 1) / PL_WAVES));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_periodlink_join_kernel<true>), grid, dim3(PL_THREADS), 0, st, a);
    else hipLaunchKernelGGL((prf_periodlink_join_kernel<false>), grid, dim3(PL_THREADS), 0, st, a);
    return hipGetLastError();
}
