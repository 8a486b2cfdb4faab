// alignlocal.hip -- the local alignment of windows around tandem repeats to their motifs (include/prf_alignlocal.h):
// the Smith-Waterman form of align.hip's wraparound dynamic programming under (match, mismatch, indel) weights, one wave per row,
// sequential over the row's positions, the lanes over the motif's columns.  The recurrence, the packing of a cell into one u64,
// the saturating subtraction and everything a lane does on its own are alignlocal_word.h's; here is what crosses lanes.
//
// prf_alignlocal_kernel<C>: C = 1, 2, 4, 8, 16 consecutive columns per lane, in registers (k <= 64 C).  Per position:
//   - the base, the same in all lanes: cs_window over cs_wave_source (no address into the planes is formed here but in
//     cs_wave_source::take), read lane by lane;
//   - the diagonal term of a lane's first column comes from the last slot of the lane before it, for column 0 from the cell of
//     column k - 1, which is the value broadcast at the position before;
//   - the first pass is a prefix maximum: serial within the lane, then over the lanes' totals (log2 of the lanes that hold a
//     column steps of __shfl_up), then taken into the lane's slots;
//   - P[k - 1] is the maximum of all totals, read from the last lane that holds a column, with the bias of column k - 1 off;
//   - the running best stays in the lane; one butterfly of 6 steps behind the last position joins the lanes'.
// The weights are kernel arguments; the multiples of `indel` that a lane's slots need are those of its first column (once per
// row) plus a constant per slot, the same in all lanes.  No LDS, no atomics.
#include "../../include/prf.h"
#include "alignlocal_launch.h"
#include "consensus_wave.h"

#define ALL_THREADS 256
#define ALL_WAVES (ALL_THREADS / 64)

static_assert(sizeof(prf_local_alignment) == 24 && sizeof(all_result) == sizeof(prf_local_alignment) && sizeof(al_row) == 32, "the rows");
static_assert(PRF_ALL_MAX_WEIGHT == PRF_ALIGNLOCAL_MAX_WEIGHT && PRF_AL_MAX_K <= ALL_A_MASK + 1u && PRF_AL_MAX_LEN <= ALL_P_MASK + 1ull,
              "the weights' limit, and the labels of a cell hold a column and a position");
static_assert((u64)PRF_ALL_MAX_WEIGHT * (PRF_AL_MAX_LEN + PRF_AL_MAX_K) < (1ull << 25), "the score field holds a score and a bias");

namespace {

template <int C>
__global__ __launch_bounds__(ALL_THREADS) void prf_alignlocal_kernel(const prf_alignlocal_args a, const u64 row0, const u64 n_rows) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 at = (u64)blockIdx.x * ALL_WAVES + wave;
    if (at >= n_rows) return;                                                  // the whole wave
    const al_row r = a.rows[row0 + at];
    if (!r.k || r.k > 64u * C || r.start >= r.end || r.end - r.start > PRF_AL_MAX_LEN || r.index >= a.n_results) return;
    const u32 k = r.k, col0 = lane * C;
    const u32 real = al_real_slots(k, C, lane), lanes = al_real_lanes(k, C);
    const all_weights w = all_weights_of(a.match, a.mismatch, a.indel);
    const u64 bias0 = (u64)col0 * w.indel;
    const u64 codes = al_lane_codes<C>(a.motifs + r.offset, k, lane);
    u64 D[C], U[C];
#pragma unroll
    for (int c = 0; c < C; c++) D[c] = 0ull;
    u64 last = 0ull;                                                           // the cell of column k - 1
    all_best best{0ull, 0ull};
    cs_wave_source src{a.pl, (a.g_begin + r.end - 1ull) >> 6, lane};
    cs_window<cs_wave_source> win;
    win.open(src, a.g_begin + r.start, a.g_begin + r.end - 1ull);
#pragma unroll 1
    for (u64 cur = r.start; cur < r.end; cur += 64ull) {
        const u64 q = a.g_begin + cur;
        win.seek(src, q);
        const u32 mine = win.base(q, lane);                                    // the base of position cur + lane
        const u32 n = r.end - cur < 64ull ? (u32)(r.end - cur) : 64u;
        const u32 i0 = (u32)(cur - r.start);
#pragma unroll 1
        for (u32 t = 0; t < n; t++) {
            const u32 b = (u32)__builtin_amdgcn_readlane((int)mine, (int)t);
            const u64 up = __shfl_up(D[C - 1], 1);
            u64 inc = all_lane_scan<C>(D, lane ? up : last, b, codes, real, bias0, all_fresh(i0 + t, col0), w, U);
            for (u32 d = 1; d < lanes; d <<= 1) {
                const u64 o = __shfl_up(inc, d);
                if (lane >= d) inc = all_max(inc, o);
            }
            const u64 before = __shfl_up(inc, 1);
            last = all_last(__shfl(inc, (int)(lanes - 1u)), k, w);
            all_lane_wrap<C>(U, lane ? before : 0ull, last, real, bias0, w, D);
            all_lane_best<C>(D, all_where(i0 + t, col0), &best);
        }
    }
#pragma unroll
    for (u32 d = 32; d; d >>= 1) all_pick(&best, __shfl_xor(best.key, (int)d), __shfl_xor(best.cell, (int)d));
    if (lane == 0) a.dst[r.index] = all_finish(best);
}

template <int C>
void all_launch(hipStream_t st, const prf_alignlocal_args &a, u32 blocks, u64 row0, u64 n_rows) {
    hipLaunchKernelGGL((prf_alignlocal_kernel<C>), dim3(blocks), dim3(ALL_THREADS), 0, st, a, row0, n_rows);
}

}  // namespace

hipError_t prf_launch_alignlocal(hipStream_t st, const prf_alignlocal_args &a, u32 regime, u64 row0, u64 n_rows) {
    if (!n_rows) return hipSuccess;
    const u64 blocks = (n_rows + ALL_WAVES - 1) / ALL_WAVES;
    if (blocks > 0x7fffffffull || regime >= PRF_AL_REGIMES || !a.rows || !a.motifs || !a.dst) return hipErrorInvalidValue;
    if (!a.match || !a.mismatch || !a.indel || a.match > PRF_ALL_MAX_WEIGHT || a.mismatch > PRF_ALL_MAX_WEIGHT || a.indel > PRF_ALL_MAX_WEIGHT)
        return hipErrorInvalidValue;
    switch (regime) {
    case 0: all_launch<1>(st, a, (u32)blocks, row0, n_rows); break;
    case 1: all_launch<2>(st, a, (u32)blocks, row0, n_rows); break;
    case 2: all_launch<4>(st, a, (u32)blocks, row0, n_rows); break;
    case 3: all_launch<8>(st, a, (u32)blocks, row0, n_rows); break;
    default: all_launch<16>(st, a, (u32)blocks, row0, n_rows); break;
    }
    return hipGetLastError();
}
