// alignpath.hip -- the alignment of tandem repeats to their motifs WITH ITS PATH (include/prf_alignpath.h): the
// forward pass of align.hip plus two bits per cell, a walk back through those bits, and the counts of the aligned columns.  What
// a lane does on its own, the layout of the trace and the step of the walk are alignpath_word.h's; here is what crosses lanes.
//
// prf_alignpath_forward_kernel<C>: prf_align_kernel<C>'s loop, cell for cell (so dst is the same, bit for bit), and per position
// the lane's 2 C bits, packed over 32 / (2 C) positions into one u32 and stored [group][lane]: 256 consecutive bytes per wave
// and group, nothing waits for them.
// prf_alignpath_walk_kernel: one wave per row, any regime.  The walk is serial and its state (i, j) is the same in all lanes;
// it visits the positions in descending order, so the wave holds the words of AP_BLOCK groups in registers (the next block is
// loaded while this one is walked) and reads the word of lane j >> regime by readlane.  64 path entries are kept across the
// lanes and stored together; a deletion is one non-returning add of one lane.
// prf_alignpath_counts_kernel: one thread per entry of the whole path: the base of its position against the motif letter of its
// column gives the SUB bit and the counts 0 .. 3; an insertion counts at 5.
// No LDS.
#include "../../include/prf.h"
#include "alignpath_launch.h"
#include "consensus_wave.h"

#define AP_THREADS 256
#define AP_WAVES (AP_THREADS / 64)
#define AP_BLOCK 8          // groups of the trace a lane of the walk holds at a time

static_assert(sizeof(prf_alignment) == 24 && sizeof(al_result) == sizeof(prf_alignment) && sizeof(ap_row) == 48, "the rows");
static_assert(PRF_AP_MAX_POSITIONS == PRF_ALIGNPATH_MAX_POSITIONS && PRF_AP_INS == PRF_PATH_INS && PRF_AP_SUB == PRF_PATH_SUB &&
                  PRF_AP_COLUMN == PRF_PATH_COLUMN && PRF_AL_MAX_K <= PRF_AP_COLUMN + 1u,
              "the limits and the bits of an entry");

namespace {

template <int C>
struct ap_regime_of {
    static constexpr u32 value = C == 1 ? 0u : C == 2 ? 1u : C == 4 ? 2u : C == 8 ? 3u : 4u;
};

// what both kernels refuse to touch: a row that is not one of this product's, or whose trace or path is not inside the buffers
__device__ __forceinline__ bool ap_row_fits(const prf_alignpath_args &a, const ap_row &r) {
    if (!r.k || r.k > PRF_AL_MAX_K || r.start >= r.end || r.end - r.start > PRF_AL_MAX_LEN || r.index >= a.n_results) return false;
    const u64 n = r.end - r.start, words = ap_trace_words((u32)n, al_regime(r.k));
    return r.trace <= a.trace_words && words <= a.trace_words - r.trace && r.path <= a.n_path && n <= a.n_path - r.path;
}

template <int C>
__global__ __launch_bounds__(AP_THREADS) void prf_alignpath_forward_kernel(const prf_alignpath_args a, const u64 row0, const u64 n_rows) {
    constexpr u32 R = ap_regime_of<C>::value;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 at = (u64)blockIdx.x * AP_WAVES + wave;
    if (at >= n_rows) return;                                                  // the whole wave
    const ap_row r = a.rows[row0 + at];
    if (!ap_row_fits(a, r) || al_regime(r.k) != R) return;
    const u32 k = r.k, col0 = lane * C, n_r = (u32)(r.end - r.start);
    const u32 real = al_real_slots(k, C, lane), lanes = al_real_lanes(k, C);
    const u64 bias0 = real ? al_bias(k, col0) : 0ull;
    const u64 codes = al_lane_codes<C>(a.motifs + r.offset, k, lane);
    u32 *const trace = a.trace + r.trace;
    u64 D[C], U[C];
    al_lane_open<C>(D, real);
    u64 last = 0ull;                                                           // the cell of column k - 1
    u32 word = 0u;
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
            u32 bits, own;
            u64 inc = ap_lane_scan<C>(D, lane ? up : last, b, codes, real, bias0, U, &bits, &own);
            for (u32 d = 1; d < lanes; d <<= 1) {
                const u64 o = __shfl_up(inc, d);
                if (lane >= d) inc = al_min(inc, o);
            }
            const u64 before = __shfl_up(inc, 1);
            last = __shfl(inc, (int)(lanes - 1u));
            ap_lane_wrap<C>(U, lane ? before : AL_SENTINEL, last, real, bias0, col0, own, D, &bits);
            if (ap_pack(&word, bits, i0 + t, n_r, R)) {                        // the same in all lanes
                trace[ap_word_index(i0 + t, lane, R)] = word;
                word = 0u;
            }
        }
    }
    u64 best;
    u32 best_col;
    al_lane_pick<C>(D, real, col0, &best, &best_col);
#pragma unroll
    for (u32 d = 32; d; d >>= 1) al_pick(&best, &best_col, __shfl_xor(best, (int)d), (u32)__shfl_xor((int)best_col, (int)d));
    if (lane == 0) a.dst[r.index] = al_finish(best, best_col, k);
}

__device__ __forceinline__ void ap_load_block(u32 *w, const u32 *trace, u32 block, u32 n_groups, u32 lane) {
#pragma unroll
    for (int x = 0; x < AP_BLOCK; x++) {
        const u32 g = block * AP_BLOCK + (u32)x;
        w[x] = g < n_groups ? trace[(u64)g * 64ull + lane] : 0u;
    }
}

__global__ __launch_bounds__(AP_THREADS) void prf_alignpath_walk_kernel(const prf_alignpath_args a, const u64 row0, const u64 n_rows) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 at = (u64)blockIdx.x * AP_WAVES + wave;
    if (at >= n_rows) return;                                                  // the whole wave
    const ap_row r = a.rows[row0 + at];
    if (!ap_row_fits(a, r)) return;
    // the state of the walk is the same in all lanes: say so, and it lives in scalar registers
    const u32 k = (u32)__builtin_amdgcn_readfirstlane((int)r.k);
    const u32 n = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(r.end - r.start));
    const u32 R = al_regime(k), group_shift = ap_group_shift(R);
    u32 j = (u32)__builtin_amdgcn_readfirstlane((int)a.dst[r.index].end_column);
    if (j >= k) return;
    const u32 *const trace = a.trace + r.trace;
    unsigned short *const out = a.path + r.path;
    u32 *const counts = a.counts ? a.counts + 6ull * r.offset : nullptr;
    const u32 n_groups = ap_n_groups(n, R), n_blocks = (n_groups + AP_BLOCK - 1u) / AP_BLOCK;
    u32 w[AP_BLOCK], ahead[AP_BLOCK];
    ap_load_block(w, trace, n_blocks - 1u, n_groups, lane);
    u32 i = n - 1u, mine = 0u;
#pragma unroll 1
    for (u32 block = n_blocks; block-- > 0u;) {
        ap_load_block(ahead, trace, block ? block - 1u : n_blocks, n_groups, lane);    // behind the first block: nothing, zeros
#pragma unroll
        for (int x = AP_BLOCK - 1; x >= 0; x--) {
            const u32 g = block * AP_BLOCK + (u32)x;
            if (g >= n_groups) continue;
            const u32 lowest = g << group_shift;                               // i is in group g; walk down to its first position
#pragma unroll 1
            for (;;) {
                u32 entry = 0u, run = 0u;
#pragma unroll 1
                for (;;) {
                    const u32 col = j;
                    u32 code = ap_code((u32)__builtin_amdgcn_readlane((int)w[x], (int)(j >> R)), i, j, R);
                    if (run >= k) code &= 1u;                                  // a run of deletions is shorter than k: never taken
                    if (ap_walk_step(code, k, &j, &entry)) break;
                    ++run;
                    if (counts && lane == 0u) atomicAdd(counts + 6u * col + 4u, 1u);
                }
                if (lane == (i & 63u)) mine = entry;
                if (!(i & 63u) && i + lane < n) out[i + lane] = (unsigned short)mine;
                if (i == lowest) break;
                --i;
            }
            if (i) --i;
        }
#pragma unroll
        for (int x = 0; x < AP_BLOCK; x++) w[x] = ahead[x];
    }
}

__global__ __launch_bounds__(AP_THREADS) void prf_alignpath_counts_kernel(const prf_alignpath_count_args a) {
    const u64 stride = (u64)gridDim.x * AP_THREADS;
    for (u64 p = (u64)blockIdx.x * AP_THREADS + threadIdx.x; p < a.n_path; p += stride) {
        u64 lo = 0, hi = a.n_rows;                                             // first[lo] <= p < first[hi]
        while (hi - lo > 1ull) {
            const u64 mid = lo + (hi - lo) / 2ull;
            if (a.first[mid] <= p) lo = mid;
            else hi = mid;
        }
        const u64 q = a.g_begin + a.start[lo] + (p - a.first[lo]), w = q >> 6;
        const u32 b = cs_base(a.pl.H[w], a.pl.L[w], a.pl.X[w], (u32)(q & 63ull));
        const u32 entry = a.path[p];
        const u64 letter = a.offset[lo] + (entry & PRF_AP_COLUMN);
        if (entry & PRF_AP_INS) {
            if (a.counts) atomicAdd(a.counts + 6ull * letter + 5ull, 1u);
            continue;
        }
        if ((al_motif_code(a.motifs[letter]) & 7u) != b) a.path[p] = (unsigned short)(entry | PRF_AP_SUB);
        if (a.counts && b < 4u) atomicAdd(a.counts + 6ull * letter + b, 1u);
    }
}

template <int C>
void ap_launch(hipStream_t st, const prf_alignpath_args &a, u32 blocks, u64 row0, u64 n_rows) {
    hipLaunchKernelGGL((prf_alignpath_forward_kernel<C>), dim3(blocks), dim3(AP_THREADS), 0, st, a, row0, n_rows);
}

bool ap_args_ok(const prf_alignpath_args &a, u64 n_rows, u64 *blocks) {
    *blocks = (n_rows + AP_WAVES - 1) / AP_WAVES;
    return *blocks <= 0x7fffffffull && a.rows && a.motifs && a.dst && a.trace && a.path;
}

}  // namespace

hipError_t prf_launch_alignpath_forward(hipStream_t st, const prf_alignpath_args &a, u32 regime, u64 row0, u64 n_rows) {
    if (!n_rows) return hipSuccess;
    u64 blocks;
    if (!ap_args_ok(a, n_rows, &blocks) || regime >= PRF_AL_REGIMES) return hipErrorInvalidValue;
    switch (regime) {
    case 0: ap_launch<1>(st, a, (u32)blocks, row0, n_rows); break;
    case 1: ap_launch<2>(st, a, (u32)blocks, row0, n_rows); break;
    case 2: ap_launch<4>(st, a, (u32)blocks, row0, n_rows); break;
    case 3: ap_launch<8>(st, a, (u32)blocks, row0, n_rows); break;
    default: ap_launch<16>(st, a, (u32)blocks, row0, n_rows); break;
    }
    return hipGetLastError();
}

hipError_t prf_launch_alignpath_walk(hipStream_t st, const prf_alignpath_args &a, u64 row0, u64 n_rows) {
    if (!n_rows) return hipSuccess;
    u64 blocks;
    if (!ap_args_ok(a, n_rows, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prf_alignpath_walk_kernel, dim3((u32)blocks), dim3(AP_THREADS), 0, st, a, row0, n_rows);
    return hipGetLastError();
}

hipError_t prf_launch_alignpath_counts(hipStream_t st, const prf_alignpath_count_args &a) {
    if (!a.n_path) return hipSuccess;
    if (!a.n_rows || !a.first || !a.start || !a.offset || !a.motifs || !a.path) return hipErrorInvalidValue;
    const u64 blocks = (a.n_path + AP_THREADS - 1) / AP_THREADS;
    hipLaunchKernelGGL(prf_alignpath_counts_kernel, dim3((u32)(blocks < 16384ull ? blocks : 16384ull)), dim3(AP_THREADS), 0, st, a);
    return hipGetLastError();
}
