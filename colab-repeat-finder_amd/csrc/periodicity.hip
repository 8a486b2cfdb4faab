// periodicity.hip -- the periodicity matrix of a range of a resident genome (reference utils/plot_utils.py:12-25):
// cell (k, i) = seq[i] == seq[i + k] for begin <= i < end - k, by plain comparison of symbols -- N == N is a match here, and the
// end of the RANGE clips a row (the guard gap behind a contig is N and would match N).
//
// One kernel template, two outputs:
//   PER_BITS    the cells themselves, nk x ceil(len / 64) words; bit j of word w of row k = cell (k, begin + 64 w + j)
//   PER_COUNTS  nk x ceil(len / W) sums of cells over windows of W = 64 * wpw positions
//
// A workgroup owns a span of span_words 64-position words of the range and one slice [klo, khi] of the motif sizes
// (blockIdx.x, blockIdx.y).  It stages, ONCE, the words of every plane that its cells touch into LDS: the "a" side seq[i]
// (span_words + 1 words from the word of the span's first position) and the "b" side seq[i + k] (span_words + 2 +
// (khi - klo) / 64 words from the word of first position + klo); where the two overlap or touch -- every slice that begins at a
// small k -- they are one region, read once.  Words behind the last position of the range are staged as 0 and never read from
// memory, so nothing behind `end` is compared or even loaded.  Then each wave takes every fourth k of the slice; a lane owns a
// word: its "a" bits stay in registers for the whole k loop, its "b" bits are two LDS words funnel-shifted by (s + k) & 63,
// which is uniform over the wave.
// Counts: popcount per lane, an inclusive wave scan over the wave's chunk of 64 words, and the lane that holds the last word
// of a window (or of the chunk, or of the range) writes the sum of the window's words in the chunk: a plain store if the whole
// window lies inside the chunk, an atomicAdd on the (zeroed) entry otherwise.  Integer sums: the result does not depend on
// the order.
#include "prf_host.h"

#define PER_THREADS 256
#define PER_WAVES (PER_THREADS / 64)

enum { PER_COUNTS = 0, PER_BITS = 1 };

namespace {

struct per_a_side {
    u64 h, l, x;
    u64 e[5];
};

// planes staged in LDS: plane p of side A at lds + p * stride, of side B at lds + p * stride + b_off
template <int NP>
__device__ __forceinline__ void per_stage(u64 *lds, const prf_periodicity_args &a, u64 word0, u32 n, u64 wlast) {
    const u64 *const P[8] = {a.pl.H, a.pl.L, a.pl.X, a.pl.E[0], a.pl.E[1], a.pl.E[2], a.pl.E[3], a.pl.E[4]};
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const u64 *__restrict__ src = P[p];
        u64 *dst = lds + (size_t)p * a.lds_stride;
        for (u32 i = threadIdx.x; i < n; i += PER_THREADS) {
            const u64 wi = word0 + i;
            dst[i] = wi <= wlast ? src[wi] : 0ull;
        }
    }
}

template <int MODE, bool EXOTIC>
__global__ __launch_bounds__(PER_THREADS) void prf_periodicity_kernel(const prf_periodicity_args a) {
    extern __shared__ __attribute__((aligned(16))) u64 per_lds[];
    constexpr int NP = EXOTIC ? 8 : 3;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 span_w0 = (u64)blockIdx.x * a.span_words;                  // first word of the span, in words of the range
    const u32 nsw = (u32)min((u64)a.span_words, a.n_words - span_w0);    // words of the span that exist
    const u32 klo = a.kmin + blockIdx.y * a.kslice;
    const u32 khi = min(a.kmax, klo + a.kslice - 1u);
    const u64 q0 = a.g_begin + span_w0 * 64;                             // global position of the span's first cell
    const u32 s = (u32)(q0 & 63);
    const u64 word_a = q0 >> 6, word_b = (q0 + klo) >> 6;
    const u64 wlast = (a.g_begin + a.len - 1) >> 6;                      // the word of the last position of the range
    const u32 n_a = nsw + 1, n_b = nsw + 2 + ((khi - klo) >> 6);
    u32 b_off;                                                           // LDS word of global word word_b
    if (word_b - word_a <= n_a) {                                        // one region
        b_off = (u32)(word_b - word_a);
        per_stage<NP>(per_lds, a, word_a, b_off + n_b, wlast);
    } else {
        b_off = n_a;
        per_stage<NP>(per_lds, a, word_a, n_a, wlast);
        per_stage<NP>(per_lds + b_off, a, word_b, n_b, wlast);
    }
    __syncthreads();

    const u64 *const lh = per_lds, *const ll = per_lds + a.lds_stride, *const lx = per_lds + 2 * (size_t)a.lds_stride;
    const u32 n_chunks = (nsw + 63u) / 64u;
    for (u32 ch = 0; ch < n_chunks; ch++) {
        const u32 lw = ch * 64 + lane;                                   // the lane's word, in words of the span
        const bool live = lw < nsw;
        const u32 lwc = live ? lw : 0u;                                  // (dead lanes read word 0 and write nothing)
        const u64 gw = span_w0 + lw;                                     // ... in words of the range
        per_a_side A;
        A.h = prf_fsr(lh[lwc], lh[lwc + 1], s);
        A.l = prf_fsr(ll[lwc], ll[lwc + 1], s);
        A.x = prf_fsr(lx[lwc], lx[lwc + 1], s);
        if (EXOTIC) {
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const u64 *le = per_lds + (size_t)(3 + i) * a.lds_stride;
                A.e[i] = prf_fsr(le[lwc], le[lwc + 1], s);
            }
        }
        // cells of this word that exist for k: positions r = 64 gw + j of the range with r + k < len
        const long long room = (long long)a.len - 64ll * (long long)gw;
        // counts: the last word of a window, of the wave's chunk, of the span or of the range closes a sum
        const u32 in_win = (u32)(gw % a.wpw);
        const bool closes = live && (in_win + 1 == a.wpw || lane == 63u || lw + 1 == nsw);
        const u32 first = lane > in_win ? lane - in_win : 0u;            // first lane of the window's words in this chunk
        for (u32 k = klo + wave; k <= khi; k += PER_WAVES) {
            const u32 off = (u32)((q0 + klo) & 63) + (k - klo);          // bit offset of seq[i + k] in side B
            const u32 bw = b_off + lwc + (off >> 6), bs = off & 63u;
            const u64 bh = prf_fsr(lh[bw], lh[bw + 1], bs);
            const u64 bl = prf_fsr(ll[bw], ll[bw + 1], bs);
            const u64 bx = prf_fsr(lx[bw], lx[bw + 1], bs);
            u64 same_n = ~0ull;                                          // both not ACGT: the same symbol?
            if (EXOTIC) {
                u64 diff = 0;
#pragma unroll
                for (int i = 0; i < 5; i++) {
                    const u64 *le = per_lds + (size_t)(3 + i) * a.lds_stride;
                    diff |= A.e[i] ^ prf_fsr(le[bw], le[bw + 1], bs);
                }
                same_n = ~diff;
            }
            u64 m = (~(A.x | bx) & ~((A.h ^ bh) | (A.l ^ bl))) | (A.x & bx & same_n);
            const long long valid = room - (long long)k;
            m &= valid >= 64 ? ~0ull : valid <= 0 ? 0ull : (1ull << valid) - 1ull;
            if (!live) m = 0;
            const u64 row = (u64)(k - a.kmin);
            if (MODE == PER_BITS) {
                if (live) a.bits[row * a.n_words + gw] = m;
            } else {
                u32 sum = (u32)__popcll(m);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const u32 up = __shfl_up(sum, d, 64);
                    if (lane >= (u32)d) sum += up;
                }
                const u32 before = __shfl(sum, first ? first - 1 : 0, 64);
                const u32 total = sum - (first ? before : 0u);
                if (closes) {
                    const u64 win = gw / a.wpw;
                    const u64 w_begin = win * a.wpw, w_end = min(w_begin + a.wpw, a.n_words);
                    u32 *dst = a.counts + row * a.n_windows + win;
                    // the window's words in this chunk begin at lane `first`; it is whole iff it began there and ends here
                    const bool whole = w_begin == gw - (lane - first) && gw + 1 == w_end;
                    if (whole) *dst = total;
                    else atomicAdd(dst, total);
                }
            }
        }
    }
}

template <int MODE>
hipError_t per_launch(hipStream_t st, const prf_periodicity_args &a, dim3 grid, size_t lds) {
    if (a.pl.E[0]) hipLaunchKernelGGL((prf_periodicity_kernel<MODE, true>), grid, dim3(PER_THREADS), lds, st, a);
    else hipLaunchKernelGGL((prf_periodicity_kernel<MODE, false>), grid, dim3(PER_THREADS), lds, st, a);
    return hipGetLastError();
}

}  // namespace

// The shape of one launch: span and k slice chosen so that both sides of all planes fit PRF_PER_LDS_BYTES
void prf_periodicity_shape(bool exotic, u32 *span_words, u32 *kslice, u32 *lds_stride) {
    *span_words = exotic ? 256u : 512u;
    *kslice = exotic ? 1024u : 2048u;
    // side A: span + 1 words; side B: span + 2 + (kslice - 1) / 64 words; one more so that the stride is even (16-byte rows)
    *lds_stride = ((*span_words + 1u) + (*span_words + 2u + (*kslice - 1u) / 64u) + 1u) & ~1u;
}

hipError_t prf_launch_periodicity(hipStream_t st, prf_periodicity_args a, bool want_bits) {
    if (!a.len) return hipSuccess;
    const bool exotic = a.pl.E[0] != nullptr;
    prf_periodicity_shape(exotic, &a.span_words, &a.kslice, &a.lds_stride);
    const u64 n_spans = (a.n_words + a.span_words - 1) / a.span_words;
    const u32 n_slices = (a.kmax - a.kmin) / a.kslice + 1u;
    if (n_spans > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((u32)n_spans, n_slices);
    const size_t lds = (size_t)(exotic ? 8 : 3) * a.lds_stride * sizeof(u64);
    return want_bits ? per_launch<PER_BITS>(st, a, grid, lds) : per_launch<PER_COUNTS>(st, a, grid, lds);
}
