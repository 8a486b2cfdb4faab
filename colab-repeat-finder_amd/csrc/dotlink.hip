// dotlink.hip -- the junctions between the chains of dotchain.hip across neighbouring lines of the dot plot of two ranges: "chain
// X ends here, chain Y starts there, |s| lines away" (include/prf_dotlink.h, whose words these comments use).  The
// SEEDS are the rows the kernels of dotruns.hip wrote at min_len = min_seed, as for dotchain.hip.  Both kernels work in the
// coordinates (i, c) of a direction, c = j (main) or nb - 1 - j (anti): the line of offset delta = c - i begins at
// (max(0, -delta), max(0, delta)) and its cell t lies t rows further on; dr_step from that origin yields cells 64 k .. 64 k + 63
// of the line for any k, outside the line as mismatches.
//
// prf_dotlink_heads_kernel, one thread per seed: dc_is_head; the indices of the heads are compacted into a list with one atomic
// per wave.
// prf_dotlink_join_kernel, one WAVE per head Y; lane l stands for the shift s = l - 32 (l < 32) or l - 31: -32 .. -1, 1 .. 32.
// Lanes with |s| > max_shift idle.
//   step A   lane s looks on the line delta_Y - s for the chain's end in the stretch where (X, Y) is a candidate
//            (dl_tail_in_stretch); the wave's minimum over the packed keys is pred(Y) = X.  No candidate: no link.
//   step B   X is wave-uniform.  Lane s' looks on the line delta_X + s' for the chain's start in the stretch where (X, Y') is a
//            candidate (dl_head_in_stretch).  A stretch is cut where it can only hold keys larger than key(X, Y): gaps above
//            key(X, Y)'s first part minus |s'|.  The wave's minimum is succ(X), or something larger than key(X, Y).
//   emit     lane 0, iff the minimum is key(X, Y), which names Y's line; a line holds one candidate, so it is Y.
// A packed key is (m + |s|) << 12 | |s| << 6 | o << 1 | (s < 0): m <= 4096, |s| <= 32, o <= 16; |s| and the sign make the keys
// of a wave differ.  No address is formed here: every read of the planes is dr_step's, guarded by dr_bits.
#include "../../include/prf.h"
#include "prf_host.h"
#include "dotruns_step.h"
#include "dotchain_walk.h"
#include "dotlink_walk.h"

#define DL_THREADS 256

static_assert(sizeof(prf_dotlink_dev) == sizeof(prf_dotlink) && sizeof(prf_dotlink) == 48, "prf_dotlink is 48 bytes");
static_assert(PRF_DOTLINK_MAX_SHIFT == 32, "one lane of a wave per shift");
static_assert(PRF_DOTCHAIN_MAX_GAP + PRF_DOTLINK_MAX_SHIFT < (1u << 13) && PRF_DOTLINK_OVERLAP < 32, "the packed key");

namespace {

typedef long long i64;

struct dl_line {
    u64 i0, j0;   // the line's first cell
    u32 dir;
};

// word k of the line's raw cells: bit b = cell 64 k + b is raw; cells behind the line's end are 0
template <bool EXOTIC>
__device__ __forceinline__ u64 dl_word(const prf_dotruns_args &a, const dr_words &w, const dl_line &l, u64 k) {
    return ~dr_step<EXOTIC>(a, w, l.i0, l.j0, l.dir, 64ull * k);
}

// the line of offset delta in (i, c), if the rectangle has it; *cells: its cells
__device__ __forceinline__ bool dl_line_of(const prf_dotruns_args &a, i64 delta, bool anti, dl_line *l, u64 *cells) {
    if (delta <= -(i64)a.na || delta >= (i64)a.nb) return false;
    const u64 i0 = delta < 0 ? (u64)-delta : 0ull, c0 = delta > 0 ? (u64)delta : 0ull;
    *l = dl_line{i0, anti ? a.nb - 1ull - c0 : c0, anti ? (u32)PRF_DOTRUN_ANTI : (u32)PRF_DOTRUN_MAIN};
    *cells = a.na - i0 < a.nb - c0 ? a.na - i0 : a.nb - c0;
    return true;
}

__device__ __forceinline__ u32 dl_wave_min(u32 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ u32 dl_key(i64 g, u32 shift, bool neg) {
    const u32 m = g > 0 ? (u32)g : 0u, o = g < 0 ? (u32)-g : 0u;
    return (m + shift) << 12 | shift << 6 | o << 1 | (neg ? 1u : 0u);
}

template <bool EXOTIC>
__global__ __launch_bounds__(DL_THREADS) void prf_dotlink_heads_kernel(const prf_dotruns_args a, const prf_dotlink_args c) {
    const u32 lane = threadIdx.x & 63u;
    const u64 idx = (u64)blockIdx.x * DL_THREADS + threadIdx.x;
    const dr_words words = dr_words_of(a);
    bool head = false;
    if (idx < c.n_seeds) {
        const prf_dotrun_dev seed = c.seed_rows[idx];
        const bool anti = seed.dir == PRF_DOTRUN_ANTI;
        const u64 side = anti ? a.nb - 1ull - seed.col : seed.col;
        const u64 t0 = seed.row < side ? seed.row : side;
        const dl_line l{seed.row - t0, anti ? seed.col + t0 : seed.col - t0, seed.dir};
        u64 have = ~0ull, word = 0;                      // the word looked at last
        head = dc_is_head(t0, c.min_seed, c.max_gap, [&](u64 k) {
            if (k != have) word = dl_word<EXOTIC>(a, words, l, k), have = k;
            return word;
        });
    }
    // ---- every lane of the wave is here: the heads rank themselves by a ballot, one atomic per wave
    const u64 vote = __ballot(head);
    if (!vote) return;
    const u32 first = (u32)__builtin_ctzll(vote);
    u64 base = 0;
    if (lane == first) base = atomicAdd(c.counters + PRF_DL_HEADS, (u64)__builtin_popcountll(vote));
    base = __shfl(base, (int)first);
    if (head) {
        const u64 at = base + (u64)__builtin_popcountll(vote & ((1ull << lane) - 1ull));
        if (at < c.n_seeds) c.heads[at] = (u32)idx;
    }
}

template <bool EXOTIC>
__global__ __launch_bounds__(DL_THREADS) void prf_dotlink_join_kernel(const prf_dotruns_args a, const prf_dotlink_args c, const u64 n_heads) {
    const u32 lane = threadIdx.x & 63u;
    const u64 entry = (u64)blockIdx.x * (DL_THREADS / 64u) + (threadIdx.x >> 6);
    if (entry >= n_heads) return;                                              // the whole wave
    const u32 at_seed = c.heads[entry];
    if ((u64)at_seed >= c.n_seeds) return;
    const prf_dotrun_dev y = c.seed_rows[at_seed];
    const dr_words words = dr_words_of(a);
    const bool anti = y.dir == PRF_DOTRUN_ANTI;
    const i64 i_s = (i64)y.row, c_s = (i64)(anti ? a.nb - 1ull - y.col : y.col);
    const i64 delta_y = c_s - i_s;
    const bool neg = lane < 32u;
    const u32 shift = neg ? 32u - lane : lane - 31u;                           // |s|
    const i64 s = neg ? -(i64)shift : (i64)shift;
    const bool works = shift <= c.max_shift;
    const i64 ov = (i64)(c.min_seed - 1ull < PRF_DOTLINK_OVERLAP ? c.min_seed - 1ull : PRF_DOTLINK_OVERLAP);
    const i64 max_gap = (i64)c.max_gap;

    // ---- step A: the chain that ends on line delta_Y - s with g = base - i_e in [-ov, max_gap]
    u32 key = ~0u;
    i64 x_end = 0;                                                             // i_e of this lane's candidate
    {
        const i64 delta_x = delta_y - s;
        dl_line l{};
        u64 cells = 0;
        if (works && dl_line_of(a, delta_x, anti, &l, &cells)) {
            const i64 base = (neg ? c_s - 1ll - delta_x : i_s - 1ll) - (i64)l.i0;      // in cells of the line
            const i64 lo = base - max_gap, hi = base + ov;
            if (hi >= 0 && lo < (i64)cells) {
                u64 have = ~0ull, word = 0;
                const u64 e = dl_tail_in_stretch(lo > 0 ? (u64)lo : 0ull, (u64)hi, c.min_seed, c.max_gap, [&](u64 k) {
                    if (k != have) word = dl_word<EXOTIC>(a, words, l, k), have = k;
                    return word;
                });
                if (e != ~0ull) {
                    key = dl_key(base - (i64)e, shift, neg);
                    x_end = (i64)(l.i0 + e);
                }
            }
        }
    }
    const u32 best = dl_wave_min(key);
    if (best == ~0u) return;                                                   // no candidate: the whole wave
    const u32 best_shift = (best >> 6) & 63u;
    const u32 y_lane = (best & 1u) ? 32u - best_shift : 31u + best_shift;      // the lane of s_Y = delta_Y - delta_X
    const i64 i_e = (i64)__shfl((u64)x_end, (int)y_lane);
    const i64 delta_x = delta_y - ((best & 1u) ? -(i64)best_shift : (i64)best_shift);
    const i64 c_e = i_e + delta_x;

    // ---- step B: the chain that starts on line delta_X + s' with g = i_s' - base in [-ov, max_gap]
    key = ~0u;
    bool is_y = false;
    const u32 most = best >> 12;                                               // m + |s| of key(X, Y)
    if (works && shift <= most) {
        const i64 delta = delta_x + s;
        dl_line l{};
        u64 cells = 0;
        if (dl_line_of(a, delta, anti, &l, &cells)) {
            const i64 base = (neg ? c_e + 1ll - delta : i_e + 1ll) - (i64)l.i0;
            const i64 room = (i64)(most - shift);
            const i64 lo = base - ov, hi = base + (room < max_gap ? room : max_gap);
            if (hi >= 0 && lo < (i64)cells) {
                u64 have = ~0ull, word = 0;
                const u64 t = dl_head_in_stretch(lo > 0 ? (u64)lo : 0ull, (u64)hi, c.min_seed, c.max_gap, [&](u64 k) {
                    if (k != have) word = dl_word<EXOTIC>(a, words, l, k), have = k;
                    return word;
                });
                if (t != ~0ull) {
                    key = dl_key((i64)t - base, shift, neg);
                    is_y = (i64)(l.i0 + t) == i_s;
                }
            }
        }
    }
    const u32 next = dl_wave_min(key);
    const bool same = __shfl((int)is_y, (int)y_lane) != 0;
    if (next != best || !same) return;                                         // X prefers another chain
    if (lane == 0) {
        const u64 at = atomicAdd(c.counters + PRF_DL_LINKS, 1ull);
        if (at < c.capacity) {
            const u32 o = (best >> 1) & 31u;
            c.dst[at] = prf_dotlink_dev{y.row, y.col, (u64)i_e, anti ? a.nb - 1ull - (u64)c_e : (u64)c_e, y.dir,
                                        (best & 1u) ? -(int)best_shift : (int)best_shift, most - best_shift, o};
        }
    }
}

}  // namespace

hipError_t prf_launch_dotlink_heads(hipStream_t st, const prf_dotruns_args &a, const prf_dotlink_args &c) {
    if (!c.n_seeds) return hipSuccess;
    if (!a.na || !a.nb || a.strand > 1u || !c.min_seed || c.max_gap > PRF_DOTCHAIN_MAX_GAP || c.n_seeds > PRF_DOTCHAIN_MAX_ROWS)
        return hipErrorInvalidValue;
    const dim3 grid((u32)((c.n_seeds + DL_THREADS - 1) / DL_THREADS));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_dotlink_heads_kernel<true>), grid, dim3(DL_THREADS), 0, st, a, c);
    else hipLaunchKernelGGL((prf_dotlink_heads_kernel<false>), grid, dim3(DL_THREADS), 0, st, a, c);
    return hipGetLastError();
}

hipError_t prf_launch_dotlink_join(hipStream_t st, const prf_dotruns_args &a, const prf_dotlink_args &c, u64 n_heads) {
    if (!n_heads) return hipSuccess;
    if (n_heads > c.n_seeds || c.n_seeds > PRF_DOTCHAIN_MAX_ROWS || !a.na || !a.nb || a.strand > 1u || !c.min_seed ||
        c.max_gap > PRF_DOTCHAIN_MAX_GAP || !c.max_shift || c.max_shift > PRF_DOTLINK_MAX_SHIFT)
        return hipErrorInvalidValue;
    const dim3 grid((u32)((n_heads + DL_THREADS / 64 - 1) / (DL_THREADS / 64)));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_dotlink_join_kernel<true>), grid, dim3(DL_THREADS), 0, st, a, c, n_heads);
    else hipLaunchKernelGGL((prf_dotlink_join_kernel<false>), grid, dim3(DL_THREADS), 0, st, a, c, n_heads);
    return hipGetLastError();
}
