// periodchain.hip -- the exact runs of the period lines k = kmin .. kmax of ONE range, chained across short stretches of
// mismatches (include/prf_periodchain.h).  Line k of the periodicity matrix is diagonal k of the range's dot plot with
// itself; the seeds, links and chains are those of DESIGN 14, the walks those of dotchain_walk.h.
//
// prf_periodchain_find_kernel, geometry of periodicity.hip: a workgroup owns a span of 64-position words of the range and a slice
// [klo, khi] of k (blockIdx.x, blockIdx.y).  It stages, ONCE, the words of every plane that its cells touch into LDS, with one
// word in front of each side for the cell in front of a word; words outside the range are staged as 0 and never loaded.  Each
// wave takes every fourth k of the slice; a lane owns a word: its "a" side stays in registers over the k loop.  Per (k, word):
//   1. the cell word m and the run starts in it: m & ~(m << 1 | last cell of the previous word), cut to the window of starts
//   2. the probe: the starts whose first min(min_seed, 16) cells are raw, by shifts and ANDs over the lane's word and its
//      neighbour's (a shuffle; where the neighbour's word is not in the wave the probe lets the start pass)
//   3. for every start that passes, one per lane and round of the wave: the first run is measured (pc_run_end), a run of at least
//      min_seed cells is tested for a head (dc_is_head) and a head is followed (dc_follow) for PRF_DOTCHAIN_FOLLOW cells.  These
//      walks read the line through pc_word, straight on the planes in global memory, beginning with the word the lane holds.
//   emit: every lane of the wave is there; one atomic per wave and list, the lanes rank themselves by a ballot.  A first run or a
//      chain that is still going goes to the long list with its state.  The seeds of the window are counted in a register and
//      added once per wave.
// prf_periodchain_long_kernel finishes each entry of the long list with one wave: the 64 lanes load 64 words of the line per
// step, the walks run on wave-uniform values and read their words with a shuffle.
// No address into the planes is formed here but in pc_stage's guarded loop and through pc_word's accessor.
#include "../../include/prf.h"
#include "prf_host.h"
#include "periodchain_word.h"

#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / 64)
#define PC_PROBE 16u

static_assert(sizeof(prf_pchain_dev) == sizeof(prf_pchain) && sizeof(prf_pchain) == 32, "prf_pchain is 32 bytes");
static_assert(PRF_DOTCHAIN_FOLLOW % 64 == 0 && PRF_DOTCHAIN_FOLLOW >= 64, "the follow limit is a multiple of 64");

namespace {

template <bool EXOTIC>
struct pc_global {            // pc_word's accessor: the planes in global memory
    const prf_planes &pl;
    __device__ __forceinline__ u64 h(u64 w) const { return pl.H[w]; }
    __device__ __forceinline__ u64 l(u64 w) const { return pl.L[w]; }
    __device__ __forceinline__ u64 x(u64 w) const { return pl.X[w]; }
    __device__ __forceinline__ u64 e(int i, u64 w) const { return pl.E[i][w]; }
    __device__ __forceinline__ bool exotic() const { return EXOTIC; }
};

// planes staged in LDS: n words of every plane from global word word0 (which may be -1) to dst + p * stride
template <int NP>
__device__ __forceinline__ void pc_stage(u64 *lds, const prf_periodchain_args &a, long long word0, u32 n, long long wfirst, long long wlast) {
    const u64 *const P[8] = {a.pl.H, a.pl.L, a.pl.X, a.pl.E[0], a.pl.E[1], a.pl.E[2], a.pl.E[3], a.pl.E[4]};
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const u64 *__restrict__ src = P[p];
        u64 *dst = lds + (size_t)p * a.lds_stride;
        for (u32 i = threadIdx.x; i < n; i += PC_THREADS) {
            const long long wi = word0 + (long long)i;
            dst[i] = (wi >= wfirst && wi <= wlast) ? src[wi] : 0ull;
        }
    }
}

// 64 bits of a staged plane from bit s of word idx, and the bit in front of them (idx >= 1)
__device__ __forceinline__ u64 pc_take(const u64 *plane, u32 idx, u32 s, u32 *prev, int bit) {
    const u64 lo = plane[idx], hi = plane[idx + 1];
    *prev |= (u32)((s ? lo >> (s - 1u) : plane[idx - 1] >> 63) & 1ull) << bit;
    return prf_fsr(lo, hi, s);
}

// the slots of a wave's rows with one atomic: `mine` lanes get consecutive slots from *counter, the others ~0
__device__ __forceinline__ u64 pc_reserve(u64 *counter, bool mine, u32 lane) {
    const u64 vote = __ballot(mine);
    if (!vote) return ~0ull;
    const u32 first = (u32)__builtin_ctzll(vote);
    u64 base = 0;
    if (lane == first) base = atomicAdd(counter, (u64)__builtin_popcountll(vote));
    base = __shfl(base, (int)first);
    return mine ? base + (u64)__builtin_popcountll(vote & ((1ull << lane) - 1ull)) : ~0ull;
}

template <bool EXOTIC>
__global__ __launch_bounds__(PC_THREADS) void prf_periodchain_find_kernel(const prf_periodchain_args a) {
    extern __shared__ __attribute__((aligned(16))) u64 pc_lds[];
    constexpr int NP = EXOTIC ? 8 : 3;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 span_w0 = a.word0 + (u64)blockIdx.x * a.span_words;        // first word of the span, in words of the range
    const u32 nsw = (u32)min((u64)a.span_words, a.word1 - span_w0);      // words of the span that exist (word1 <= n_words)
    const u32 klo = a.kmin + blockIdx.y * a.kslice;
    const u32 khi = min(a.kmax, klo + a.kslice - 1u);
    const u64 q0 = a.g_begin + span_w0 * 64;                             // global position of the span's first cell
    const u32 s = (u32)(q0 & 63);
    const long long word_a = (long long)(q0 >> 6), word_b = (long long)((q0 + klo) >> 6);
    const long long wfirst = (long long)(a.g_begin >> 6), wlast = (long long)((a.g_begin + a.n - 1) >> 6);
    // side A: words word_a - 1 .. word_a + nsw; side B: words word_b - 1 .. word_b + nsw + 1 + (khi - klo) / 64
    const u32 n_a = nsw + 2, n_b = nsw + 3 + ((khi - klo) >> 6);
    u32 b_off;                                                           // LDS word of global word word_b - 1
    if (word_b - word_a <= (long long)n_a) {                             // one region
        b_off = (u32)(word_b - word_a);
        pc_stage<NP>(pc_lds, a, word_a - 1, b_off + n_b, wfirst, wlast);
    } else {
        b_off = n_a;
        pc_stage<NP>(pc_lds, a, word_a - 1, n_a, wfirst, wlast);
        pc_stage<NP>(pc_lds + b_off, a, word_b - 1, n_b, wfirst, wlast);
    }
    __syncthreads();

    const pc_global<EXOTIC> planes{a.pl};
    const pc_range range = pc_range_of(a.g_begin, a.n, a.n_matches);
    const u32 probe = a.min_seed < PC_PROBE ? (u32)a.min_seed : PC_PROBE;
    u32 my_seeds = 0;
    const u32 n_chunks = (nsw + 63u) / 64u;
    for (u32 ch = 0; ch < n_chunks; ch++) {
        const u32 lw = ch * 64 + lane;                                   // the lane's word, in words of the span
        const bool live = lw < nsw;
        const u32 lwc = live ? lw : 0u;                                  // (dead lanes read word 0 and find nothing)
        const u64 gw = span_w0 + lw;                                     // ... in words of the range
        const u64 t_word = 64ull * gw;                                   // the word's first cell
        u64 Ah, Al, Ax, Ae[5] = {0, 0, 0, 0, 0};
        u32 Ap = 0;                                                      // the symbol in front of the word: bit p = plane p
        Ah = pc_take(pc_lds, 1 + lwc, s, &Ap, 0);
        Al = pc_take(pc_lds + a.lds_stride, 1 + lwc, s, &Ap, 1);
        Ax = pc_take(pc_lds + 2 * (size_t)a.lds_stride, 1 + lwc, s, &Ap, 2);
        if (EXOTIC) {
#pragma unroll
            for (int i = 0; i < 5; i++) Ae[i] = pc_take(pc_lds + (size_t)(3 + i) * a.lds_stride, 1 + lwc, s, &Ap, 3 + i);
        }
        // the starts this call reports: cells pos0 <= t < pos1 of this word
        u64 window = 0;
        if (live && t_word < a.pos1 && t_word + 64ull > a.pos0) {
            window = ~0ull;
            if (a.pos0 > t_word) window &= ~0ull << (a.pos0 - t_word);
            if (a.pos1 - t_word < 64ull) window &= (1ull << (a.pos1 - t_word)) - 1ull;
        }
        const long long room = (long long)a.n - 64ll * (long long)gw;   // positions of the range from the word's first
        const bool next_here = lane < 63u && lw + 1u < nsw;              // the next word of the line is the next lane's
        const bool next_none = gw + 1ull >= a.n_words;                   // ... or lies behind every line's end
#pragma unroll 1
        for (u32 k = klo + wave; k <= khi; k += PC_WAVES) {
            const u32 off = (u32)((q0 + klo) & 63) + (k - klo);          // bit offset of seq[i + k] in side B
            const u32 bw = b_off + 1u + lwc + (off >> 6), bs = off & 63u;
            u64 Be[5] = {0, 0, 0, 0, 0};
            u32 Bp = 0;
            const u64 Bh = pc_take(pc_lds, bw, bs, &Bp, 0);
            const u64 Bl = pc_take(pc_lds + a.lds_stride, bw, bs, &Bp, 1);
            const u64 Bx = pc_take(pc_lds + 2 * (size_t)a.lds_stride, bw, bs, &Bp, 2);
            if (EXOTIC) {
#pragma unroll
                for (int i = 0; i < 5; i++) Be[i] = pc_take(pc_lds + (size_t)(3 + i) * a.lds_stride, bw, bs, &Bp, 3 + i);
            }
            // ---- 1. the cells and the run starts
            const long long valid = room - (long long)k;                 // cells of line k from the word's first
            u64 m = pc_cells(Ah, Al, Ax, Ae, Bh, Bl, Bx, Be, EXOTIC, a.n_matches);
            m &= valid >= 64 ? ~0ull : valid <= 0 ? 0ull : (1ull << valid) - 1ull;
            if (!live) m = 0;
            u64 before = 0;                                              // the cell in front of the word
            if (gw && valid >= 0) {
                u64 pa[5], pb[5];
#pragma unroll
                for (int i = 0; i < 5; i++) pa[i] = (Ap >> (3 + i)) & 1u, pb[i] = (Bp >> (3 + i)) & 1u;
                before = pc_cells(Ap & 1u, (Ap >> 1) & 1u, (Ap >> 2) & 1u, pa, Bp & 1u, (Bp >> 1) & 1u, (Bp >> 2) & 1u, pb, EXOTIC, a.n_matches) & 1ull;
            }
            u64 cand = m & ~((m << 1) | before) & window;
            // ---- 2. the probe: cells b .. b + probe - 1 are raw, over this word and the next
            u64 lo = m, hi = __shfl_down(m, 1);
            if (!next_here) hi = next_none ? 0ull : ~0ull;
            u32 cover = 1;
#pragma unroll 1
            while (cover < probe) {
                const u32 step = min(cover, probe - cover);
                lo &= (lo >> step) | (hi << (64u - step));
                hi &= hi >> step;
                cover += step;
            }
            cand &= lo;
            // ---- 3. one start per lane and round
#pragma unroll 1
            while (__ballot(cand != 0ull)) {
                bool seed = false, head = false, done = false, going = false;
                dc_state st{};
                u64 t0 = 0, p = 0;
                if (cand) {
                    t0 = t_word + (u64)__builtin_ctzll(cand);
                    cand &= cand - 1ull;
                    u64 have = gw, word = m;                             // the word looked at last: the lane's own at first
                    const auto cached = [&](u64 wk) {
                        if (wk != have) word = pc_word(planes, range, (u64)k, wk), have = wk;
                        return word;
                    };
                    p = t0 + 1ull;
                    if (pc_run_end(p, t0 + PRF_DOTCHAIN_FOLLOW, cached)) {
                        const u64 len = p - t0;
                        seed = len >= a.min_seed;
                        if (seed) head = dc_is_head(t0, a.min_seed, a.max_gap, cached);
                        if (head) {
                            st = dc_first_seed(t0, len);
                            done = dc_follow(st, a.min_seed, a.max_gap, t0 + len + PRF_DOTCHAIN_FOLLOW, cached);
                        }
                    } else {
                        going = true;                                    // a first run of more than PRF_DOTCHAIN_FOLLOW cells
                    }
                }
                // ---- emit: every lane of the wave is here
                my_seeds += seed ? 1u : 0u;
                const u64 len = st.end - t0 + 1ull;
                const u64 at = pc_reserve(a.counters + PRF_PC_CHAINS, head && done && len >= a.min_len, lane);
                if (at < a.capacity) a.dst[at] = prf_pchain_dev{t0, len, st.matches, k, st.seeds};
                const u64 lat = pc_reserve(a.counters + PRF_PC_LONG, going || (head && !done), lane);
                if (lat < a.long_cap)
                    a.longs[lat] = going ? prf_pchain_long{t0, 0ull, 0ull, 0ull, p, 0ull, k, 0u, 0u, 0u}
                                         : prf_pchain_long{t0, st.end, st.matches, st.pending, st.p, st.run_start, k, st.seeds, st.in_run ? 1u : 0u, 1u};
            }
        }
    }
    // the seeds of the window: one atomic per wave
#pragma unroll
    for (int d = 32; d; d >>= 1) my_seeds += __shfl_xor(my_seeds, d);
    if (lane == 0 && my_seeds) atomicAdd(a.counters + PRF_PC_SEEDS, (u64)my_seeds);
}

template <bool EXOTIC>
__global__ __launch_bounds__(PC_THREADS) void prf_periodchain_long_kernel(const prf_periodchain_args a, const u64 n_long) {
    const u32 lane = threadIdx.x & 63u;
    const u64 entry = (u64)blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (entry >= n_long) return;                                               // the whole wave
    const prf_pchain_long e = a.longs[entry];
    const pc_global<EXOTIC> planes{a.pl};
    const pc_range range = pc_range_of(a.g_begin, a.n, a.n_matches);
    // every value of the walks is the same in all lanes: their branches are taken by the whole wave
    u64 base = 0, mine = 0;
    bool loaded = false, back = false;
    const auto word = [&](u64 wk) {
        if (!loaded || wk < base || wk - base >= 64ull) {                      // 64 words in the direction of the walk
            base = back ? (wk >= 63ull ? wk - 63ull : 0ull) : wk;
            mine = pc_word(planes, range, (u64)e.k, base + lane);
            loaded = true;
        }
        return (u64)__shfl(mine, (int)(wk - base));
    };
    dc_state st{e.end, e.matches, e.pending, e.p, e.run_start, e.seeds, e.in_run != 0u};
    if (e.phase == 0u) {                                                       // the first run is still being measured
        u64 p = e.p;
        pc_run_end(p, ~0ull, word);                                            // the line's end ends it
        const u64 len = p - e.t0;
        if (len < a.min_seed) return;
        if (lane == 0) atomicAdd(a.counters + PRF_PC_SEEDS, 1ull);
        back = true;
        const bool head = dc_is_head(e.t0, a.min_seed, a.max_gap, word);
        if (!head) return;
        back = false;
        st = dc_first_seed(e.t0, len);
    }
    dc_follow(st, a.min_seed, a.max_gap, ~0ull, word);
    const u64 len = st.end - e.t0 + 1ull;
    if (lane == 0 && len >= a.min_len) {
        const u64 at = atomicAdd(a.counters + PRF_PC_CHAINS, 1ull);
        if (at < a.capacity) a.dst[at] = prf_pchain_dev{e.t0, len, st.matches, e.k, st.seeds};
    }
}

}  // namespace

// The shape of one launch, that of prf_periodicity_shape with one more word in front of each side
void prf_periodchain_shape(bool exotic, u32 *span_words, u32 *kslice, u32 *lds_stride) {
    *span_words = exotic ? 256u : 512u;
    *kslice = exotic ? 1024u : 2048u;
    // side A: span + 2 words; side B: span + 3 + (kslice - 1) / 64 words; one more so that the stride is even (16-byte rows)
    *lds_stride = ((*span_words + 2u) + (*span_words + 3u + (*kslice - 1u) / 64u) + 1u) & ~1u;
}

hipError_t prf_launch_periodchain_find(hipStream_t st, prf_periodchain_args a) {
    if (a.word0 >= a.word1) return hipSuccess;
    if (!a.n || !a.kmin || a.kmin > a.kmax || (u64)a.kmax >= a.n || a.word1 > a.n_words || !a.min_seed || a.n_matches > 1u ||
        a.max_gap > PRF_DOTCHAIN_MAX_GAP)
        return hipErrorInvalidValue;
    const bool exotic = a.pl.E[0] != nullptr;
    prf_periodchain_shape(exotic, &a.span_words, &a.kslice, &a.lds_stride);
    const u64 n_spans = (a.word1 - a.word0 + a.span_words - 1) / a.span_words;
    const u32 n_slices = (a.kmax - a.kmin) / a.kslice + 1u;
    if (n_spans > 0x7fffffffull || n_slices > 65535u) return hipErrorInvalidValue;
    const dim3 grid((u32)n_spans, n_slices);
    const size_t lds = (size_t)(exotic ? 8 : 3) * a.lds_stride * sizeof(u64);
    if (exotic) hipLaunchKernelGGL((prf_periodchain_find_kernel<true>), grid, dim3(PC_THREADS), lds, st, a);
    else hipLaunchKernelGGL((prf_periodchain_find_kernel<false>), grid, dim3(PC_THREADS), lds, st, a);
    return hipGetLastError();
}

hipError_t prf_launch_periodchain_long(hipStream_t st, const prf_periodchain_args &a, u64 n_long) {
    if (!n_long) return hipSuccess;
    if (n_long > a.long_cap || !a.n || !a.min_seed) return hipErrorInvalidValue;
    const dim3 grid((u32)((n_long + PC_WAVES - 1) / PC_WAVES));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_periodchain_long_kernel<true>), grid, dim3(PC_THREADS), 0, st, a, n_long);
    else hipLaunchKernelGGL((prf_periodchain_long_kernel<false>), grid, dim3(PC_THREADS), 0, st, a, n_long);
    return hipGetLastError();
}
