// dotchain.hip -- the exact runs of one diagonal or anti-diagonal of the dot plot of two ranges, chained across short stretches
// of mismatches (include/prf_dotchain.h).  The SEEDS are the rows that the kernels of dotruns.hip wrote at min_len =
// min_seed: every maximal run of at least min_seed raw cells that starts in the window, as (row, col, len, dir), unsorted, on the
// device.  Both kernels here work in LINE coordinates: a seed at (i, j) lies on the line that begins at (i - m, j - m), m = min(i,
// j) (main) or (i - m, j + m), m = min(i, nb - 1 - j) (anti), at cell t0 = m; dr_step from that origin yields cells 64 k .. 64 k +
// 63 of the line for any k, outside the line as mismatches, so a look backwards is a smaller k and the line's end needs no test.
//
// prf_dotchain_link_kernel, one thread per seed:
//   head test   the seed at t0 starts a chain iff no seed has its last cell in [t0 - 1 - max_gap, t0 - 2] (cell t0 - 1 is a
//               mismatch: the seed is maximal).  The words below t0 are walked downwards; a run whose end lies in that stretch is
//               followed back, past the stretch's far end too, until it has min_seed cells (not a head) or ends (look on).
//   follow      heads only: the state machine dc_follow walks forward from the seed's end.  A run that reaches min_seed cells
//               commits (the end moves, the cells of the short runs since the last end are added, seeds goes up); the chain ends
//               when no run starts within max_gap cells of the committed end.  A head that is still going PRF_DOTCHAIN_FOLLOW
//               cells behind its seed goes to the long list with its state.
//   emit        one atomic per wave and counter: the lanes with a row rank themselves by a ballot.
// prf_dotchain_long_kernel finishes each entry of the long list with one wave: the 64 lanes load 64 words of the line per step,
// the same state machine runs on wave-uniform values and reads its words with a shuffle.
// No address is formed here: every read of the planes is dr_step's, guarded by dr_bits.
#include "../../include/prf.h"
#include "prf_host.h"
#include "dotruns_step.h"
#include "dotchain_walk.h"

#define DC_THREADS 256

static_assert(sizeof(prf_dotchain_dev) == sizeof(prf_dotchain) && sizeof(prf_dotchain) == 40, "prf_dotchain is 40 bytes");
static_assert(PRF_DOTCHAIN_FOLLOW % 64 == 0 && PRF_DOTCHAIN_FOLLOW >= 64, "the follow limit is a multiple of 64");
static_assert(PRF_DOTCHAIN_MAX_GAP == 64 * 64, "a look for the next seed is at most 64 word steps");

namespace {

struct dc_line {
    u64 i0, j0;   // the line's first cell
    u32 dir;
};

// word k of the line's raw cells: bit b = cell 64 k + b is raw; cells behind the line's end are 0
template <bool EXOTIC>
__device__ __forceinline__ u64 dc_word(const prf_dotruns_args &a, const dr_words &w, const dc_line &l, u64 k) {
    return ~dr_step<EXOTIC>(a, w, l.i0, l.j0, l.dir, 64ull * k);
}

// the slots of a wave's rows with one atomic: `mine` lanes get consecutive slots from *counter, the others ~0
__device__ __forceinline__ u64 dc_reserve(u64 *counter, bool mine, u32 lane) {
    const u64 vote = __ballot(mine);
    if (!vote) return ~0ull;
    const u32 first = (u32)__builtin_ctzll(vote);
    u64 base = 0;
    if (lane == first) base = atomicAdd(counter, (u64)__builtin_popcountll(vote));
    base = __shfl(base, (int)first);
    return mine ? base + (u64)__builtin_popcountll(vote & ((1ull << lane) - 1ull)) : ~0ull;
}

template <bool EXOTIC>
__global__ __launch_bounds__(DC_THREADS) void prf_dotchain_link_kernel(const prf_dotruns_args a, const prf_dotchain_args c) {
    const u32 lane = threadIdx.x & 63u;
    const u64 idx = (u64)blockIdx.x * DC_THREADS + threadIdx.x;
    const dr_words words = dr_words_of(a);
    bool head = false, done = false;
    prf_dotrun_dev seed{};
    dc_line l{};
    dc_state s{};
    u64 t0 = 0;
    if (idx < c.n_seeds) {
        seed = c.seed_rows[idx];
        const bool anti = seed.dir == PRF_DOTRUN_ANTI;
        const u64 side = anti ? a.nb - 1ull - seed.col : seed.col;
        t0 = seed.row < side ? seed.row : side;
        l = dc_line{seed.row - t0, anti ? seed.col + t0 : seed.col - t0, seed.dir};
        u64 have = ~0ull, word = 0;                      // the word looked at last: several steps of a walk may fall into one
        const auto cached = [&](u64 k) {
            if (k != have) word = dc_word<EXOTIC>(a, words, l, k), have = k;
            return word;
        };
        head = dc_is_head(t0, c.min_seed, c.max_gap, cached);
        if (head) {
            s = dc_first_seed(t0, seed.len);
            done = dc_follow(s, c.min_seed, c.max_gap, t0 + seed.len + PRF_DOTCHAIN_FOLLOW, cached);
        }
    }
    // ---- emit: every lane of the wave is here
    const u64 len = s.end - t0 + 1ull;
    const u64 at = dc_reserve(c.counters + PRF_DC_CHAINS, head && done && len >= c.min_len, lane);
    if (at < c.capacity) c.dst[at] = prf_dotchain_dev{seed.row, seed.col, len, s.matches, seed.dir, s.seeds};
    const u64 lat = dc_reserve(c.counters + PRF_DC_LONG, head && !done, lane);
    if (lat < c.long_cap)
        c.longs[lat] = prf_dotchain_long{l.i0, l.j0, t0, s.end, s.matches, s.pending, s.p, s.run_start, l.dir, s.seeds, s.in_run ? 1u : 0u, 0u};
}

template <bool EXOTIC>
__global__ __launch_bounds__(DC_THREADS) void prf_dotchain_long_kernel(const prf_dotruns_args a, const prf_dotchain_args c, const u64 n_long) {
    const u32 lane = threadIdx.x & 63u;
    const u64 entry = (u64)blockIdx.x * (DC_THREADS / 64u) + (threadIdx.x >> 6);
    if (entry >= n_long) return;                                               // the whole wave
    const prf_dotchain_long e = c.longs[entry];
    const dr_words words = dr_words_of(a);
    const dc_line l{e.i0, e.j0, e.dir};
    dc_state s{e.end, e.matches, e.pending, e.p, e.run_start, e.seeds, e.in_run != 0u};
    // every value of the state is the same in all lanes: the branches of dc_follow are taken by the whole wave
    u64 base = 0, mine = 0;
    bool loaded = false;
    dc_follow(s, c.min_seed, c.max_gap, ~0ull, [&](u64 k) {
        if (!loaded || k - base >= 64ull) {                                    // k only grows
            base = k;
            mine = dc_word<EXOTIC>(a, words, l, base + lane);
            loaded = true;
        }
        return (u64)__shfl(mine, (int)(k - base));
    });
    const u64 len = s.end - e.t0 + 1ull;
    if (lane == 0 && len >= c.min_len) {
        const u64 at = atomicAdd(c.counters + PRF_DC_CHAINS, 1ull);
        if (at < c.capacity)
            c.dst[at] = prf_dotchain_dev{e.i0 + e.t0, e.dir == PRF_DOTRUN_ANTI ? e.j0 - e.t0 : e.j0 + e.t0, len, s.matches, e.dir, s.seeds};
    }
}

}  // namespace

hipError_t prf_launch_dotchain_link(hipStream_t st, const prf_dotruns_args &a, const prf_dotchain_args &c) {
    if (!c.n_seeds) return hipSuccess;
    if (!a.na || !a.nb || a.strand > 1u || !c.min_seed || c.max_gap > PRF_DOTCHAIN_MAX_GAP || c.n_seeds > PRF_DOTCHAIN_MAX_ROWS)
        return hipErrorInvalidValue;
    const dim3 grid((u32)((c.n_seeds + DC_THREADS - 1) / DC_THREADS));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_dotchain_link_kernel<true>), grid, dim3(DC_THREADS), 0, st, a, c);
    else hipLaunchKernelGGL((prf_dotchain_link_kernel<false>), grid, dim3(DC_THREADS), 0, st, a, c);
    return hipGetLastError();
}

hipError_t prf_launch_dotchain_long(hipStream_t st, const prf_dotruns_args &a, const prf_dotchain_args &c, u64 n_long) {
    if (!n_long) return hipSuccess;
    if (n_long > c.long_cap || !a.na || !a.nb || !c.min_seed) return hipErrorInvalidValue;
    const dim3 grid((u32)((n_long + DC_THREADS / 64 - 1) / (DC_THREADS / 64)));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_dotchain_long_kernel<true>), grid, dim3(DC_THREADS), 0, st, a, c, n_long);
    else hipLaunchKernelGGL((prf_dotchain_long_kernel<false>), grid, dim3(DC_THREADS), 0, st, a, c, n_long);
    return hipGetLastError();
}
