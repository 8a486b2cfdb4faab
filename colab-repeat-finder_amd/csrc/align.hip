// align.hip -- the alignment of tandem repeats to their motifs (include/prf_align.h): wraparound dynamic programming
// with unit costs, one wave per row, sequential over the row's positions, the lanes over the motif's columns.  The recurrence,
// the packing of a cell into one u64 and everything a lane does on its own are align_word.h's; here is what crosses lanes.
//
// prf_align_kernel<C>: C = 1, 2, 4, 8, 16 consecutive columns per lane, in registers (k <= 64 C).  Per position:
//   - the base, the same in all lanes: the lanes hold the bases of 64 positions (cs_window over cs_wave_source, one plane word per
//     64 positions; no address into the planes is formed here but in cs_wave_source::take), read lane by lane;
//   - the diagonal term of a lane's first column comes from the last slot of the lane before it, for column 0 from the cell of
//     column k - 1, which is the value broadcast at the position before (align_word.h);
//   - the first pass is a prefix minimum: serial within the lane, then over the lanes' totals (log2 of the lanes that hold a
//     column steps of __shfl_up), then taken into the lane's slots;
//   - P[k - 1], the minimum of all totals, is read from the last lane that holds a column.
// No LDS, no atomics; the only global traffic of the loop is cs_wave_source's 3 x 8 bytes per lane and 4096 positions.
#include "../../include/prf.h"
#include "align_launch.h"
#include "consensus_wave.h"

#define AL_THREADS 256
#define AL_WAVES (AL_THREADS / 64)

static_assert(sizeof(prf_alignment) == 24 && sizeof(al_result) == sizeof(prf_alignment) && sizeof(al_row) == 32, "the rows");
static_assert(PRF_AL_MAX_K == PRF_ALIGN_MAX_K && PRF_AL_MAX_LEN == PRF_ALIGN_MAX_LEN && PRF_AL_MAX_K == 64u << (PRF_AL_REGIMES - 1u),
              "the limits, and sixteen columns per lane at the largest k");

namespace {

template <int C>
__global__ __launch_bounds__(AL_THREADS) void prf_align_kernel(const prf_align_args a, const u64 row0, const u64 n_rows) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 at = (u64)blockIdx.x * AL_WAVES + wave;
    if (at >= n_rows) return;                                                  // the whole wave
    const al_row r = a.rows[row0 + at];
    if (!r.k || r.k > 64u * C || r.start >= r.end || r.end - r.start > PRF_AL_MAX_LEN || r.index >= a.n_results) return;
    const u32 k = r.k, col0 = lane * C;
    const u32 real = al_real_slots(k, C, lane), lanes = al_real_lanes(k, C);
    const u64 bias0 = real ? al_bias(k, col0) : 0ull;
    const u64 codes = al_lane_codes<C>(a.motifs + r.offset, k, lane);
    u64 D[C], U[C];
    al_lane_open<C>(D, real);
    u64 last = 0ull;                                                           // the cell of column k - 1
    cs_wave_source src{a.pl, (a.g_begin + r.end - 1ull) >> 6, lane};
    cs_window<cs_wave_source> win;
    win.open(src, a.g_begin + r.start, a.g_begin + r.end - 1ull);
#pragma unroll 1
    for (u64 cur = r.start; cur < r.end; cur += 64ull) {
        const u64 q = a.g_begin + cur;
        win.seek(src, q);
        const u32 mine = win.base(q, lane);                                    // the base of position cur + lane
        const u32 n = r.end - cur < 64ull ? (u32)(r.end - cur) : 64u;
#pragma unroll 1
        for (u32 t = 0; t < n; t++) {
            const u32 b = (u32)__builtin_amdgcn_readlane((int)mine, (int)t);
            const u64 up = __shfl_up(D[C - 1], 1);
            u64 inc = al_lane_scan<C>(D, lane ? up : last, b, codes, real, bias0, U);
            for (u32 d = 1; d < lanes; d <<= 1) {
                const u64 o = __shfl_up(inc, d);
                if (lane >= d) inc = al_min(inc, o);
            }
            const u64 before = __shfl_up(inc, 1);
            last = __shfl(inc, (int)(lanes - 1u));
            al_lane_wrap<C>(U, lane ? before : AL_SENTINEL, last, real, bias0, col0, D);
        }
    }
    u64 best;
    u32 best_col;
    al_lane_pick<C>(D, real, col0, &best, &best_col);
#pragma unroll
    for (u32 d = 32; d; d >>= 1) al_pick(&best, &best_col, __shfl_xor(best, (int)d), (u32)__shfl_xor((int)best_col, (int)d));
    if (lane == 0) a.dst[r.index] = al_finish(best, best_col, k);
}

template <int C>
void al_launch(hipStream_t st, const prf_align_args &a, u32 blocks, u64 row0, u64 n_rows) {
    hipLaunchKernelGGL((prf_align_kernel<C>), dim3(blocks), dim3(AL_THREADS), 0, st, a, row0, n_rows);
}

}  // namespace

hipError_t prf_launch_align(hipStream_t st, const prf_align_args &a, u32 regime, u64 row0, u64 n_rows) {
    if (!n_rows) return hipSuccess;
    const u64 blocks = (n_rows + AL_WAVES - 1) / AL_WAVES;
    if (blocks > 0x7fffffffull || regime >= PRF_AL_REGIMES || !a.rows || !a.motifs || !a.dst) return hipErrorInvalidValue;
    switch (regime) {
    case 0: al_launch<1>(st, a, (u32)blocks, row0, n_rows); break;
    case 1: al_launch<2>(st, a, (u32)blocks, row0, n_rows); break;
    case 2: al_launch<4>(st, a, (u32)blocks, row0, n_rows); break;
    case 3: al_launch<8>(st, a, (u32)blocks, row0, n_rows); break;
    default: al_launch<16>(st, a, (u32)blocks, row0, n_rows); break;
    }
    return hipGetLastError();
}
