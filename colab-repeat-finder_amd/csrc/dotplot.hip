// dotplot.hip -- the exact dot plot of a range of a resident genome (reference plot_dot_plot.py: generate_matrix,
// is_noise, filter_out_noise): raw(i, j) = s[i] == s[j] by plain comparison of symbols -- N == N is a match -- and
//   kept(i, j) = raw(i, j) and (a run of at least m = t - 1 raw cells along (+1, +1) or along (+1, -1) passes through (i, j)),
// runs taken in the unfiltered n x n matrix and clipped by its bounds alone; the range clips the matrix (the guard gap behind a
// contig is N and would match N), so rows and columns outside [0, n) are zero and nothing at or behind `end` is read.
//
// One kernel template, two outputs:
//   DOT_BITS    the kept cells of window rows x columns; bit j of word w of row r = kept(row0 + r, col0 + 64 w + j)
//   DOT_COUNTS  sums of kept cells over blocks of B x B cells of the window, B = 64 * wpb
//
// A workgroup owns a tile of DOT_TILE_ROWS rows x a span of span_words 64-column words of the window.  It stages, ONCE per plane,
// the column words of the span with one halo word on each side (words outside the range as 0, never read), and the symbol of
// each of its rows with `halo` = m - 1 rows above and below, as a packed word of plane bits.  Then it writes the RAW cells of
// (tile rows + 2 halo) x (span + 2) words into LDS: a thread owns a column word, whose planes it keeps in registers, and a
// row's raw word is a select on that row's symbol -- one compare per 64 cells.  The filter reads LDS only:
//   kept_main = OR_{a < m} AND_{u < m} raw(i + u - a, j + u - a),
// where row i + k is funnel-shifted by k bits (prf_fsr over two neighbouring words; |k| <= 62 stays within the halo word), and
// the anti-diagonal is the same with the opposite shift.  m = 2 (the default t = 3) is a template instance of its own, fully
// unrolled: three rows, five distinct shifted words.  Larger m is the same double loop, m^2 steps per direction.
// Counts: popcount per thread over its rows, summed per column word in LDS (integer atomics on LDS), then one thread per block
// column of the span adds the block's words: a plain store where the workgroup owns the whole block (B = 64: a tile's rows are
// one block row and a word is one block column), a vector atomicAdd on the zeroed entry otherwise.  Integer sums: the result
// does not depend on the order.  No floating point anywhere.
#include "prf_host.h"

#define DOT_THREADS 256
#define DOT_TILE_ROWS 64u

enum { DOT_COUNTS = 0, DOT_BITS = 1 };

namespace {

// bits [lo, hi) of a word, lo and hi clamped to 0 .. 64
__device__ __forceinline__ u64 dot_mask_range(long long lo, long long hi) {
    if (lo < 0) lo = 0;
    if (hi > 64) hi = 64;
    if (hi <= lo) return 0ull;
    const u64 upto_hi = hi == 64 ? ~0ull : (1ull << hi) - 1ull;
    return upto_hi & ~((1ull << lo) - 1ull);      // lo <= 63 here
}

// word c of raw row `row` moved by d bits: bit b of the result = bit 64 c + b + d of the row, -64 < d < 64, 1 <= c <= cw - 2
__device__ __forceinline__ u64 dot_shifted(const u64 *raw, u32 cw, u32 row, u32 c, int d) {
    const u64 *r = raw + (size_t)row * cw + c;
    return d >= 0 ? prf_fsr(r[0], r[1], (unsigned)d) : prf_fsr(r[-1], r[0], (unsigned)(64 + d));
}

template <int MODE, bool EXOTIC, int MFIX>
__global__ __launch_bounds__(DOT_THREADS) void prf_dotplot_kernel(const prf_dotplot_args a) {
    extern __shared__ __attribute__((aligned(16))) u64 dot_lds[];
    constexpr int NP = EXOTIC ? 8 : 3;
    const u32 m = MFIX ? (u32)MFIX : a.m;
    const u32 halo = m - 1u;
    const u32 cw = a.span_words + 2u;                  // 64 or 32: LDS words per raw row
    const u32 rb = DOT_TILE_ROWS + 2u * halo;          // raw rows in LDS
    const u32 pstride = cw + 2u;                       // LDS words per staged plane (cw + 1 used)
    u64 *const planes = dot_lds;
    u64 *const raw = dot_lds + (size_t)NP * pstride;
    u32 *const rowsym = (u32 *)(raw + (size_t)rb * cw);
    u32 *const acc = rowsym + ((rb + 1u) & ~1u);

    const u32 tid = threadIdx.x;
    const u32 c = tid & (cw - 1u), rsub = tid / cw, rstep = DOT_THREADS / cw;
    const u32 sp = blockIdx.x % a.n_spans, ti = blockIdx.x / a.n_spans;
    const u64 span_w0 = (u64)sp * a.span_words;        // first word of the span, in words of the window
    const u64 tr0 = a.lrow0 + (u64)ti * DOT_TILE_ROWS; // first row of the tile, relative to the range
    const u64 wfirst = a.g_begin >> 6, wlast = (a.g_begin + a.n - 1) >> 6;   // the words of the planes that hold the range

    // ---- stage the column words: LDS word i of a plane = plane word sw0 + i, or 0 outside the range's words
    const long long j0 = (long long)a.col0 + 64ll * ((long long)span_w0 - 1ll);   // column of bit 0 of LDS word 0 (may be < 0)
    const long long q0 = (long long)a.g_begin + j0;
    const long long sw0 = q0 >> 6;
    const u32 s = (u32)(q0 & 63);
    {
        const u64 *const P[8] = {a.pl.H, a.pl.L, a.pl.X, a.pl.E[0], a.pl.E[1], a.pl.E[2], a.pl.E[3], a.pl.E[4]};
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const u64 *__restrict__ src = P[p];
            for (u32 i = tid; i < cw + 1u; i += DOT_THREADS) {
                const long long wi = sw0 + (long long)i;
                planes[(size_t)p * pstride + i] = (wi >= (long long)wfirst && wi <= (long long)wlast) ? src[wi] : 0ull;
            }
        }
    }
    // ---- the symbols of the rows: bit 0 H, 1 L, 2 X, 3..7 E, 8 = the row exists
    for (u32 r = tid; r < rb; r += DOT_THREADS) {
        const long long i = (long long)tr0 - (long long)halo + (long long)r;
        u32 sym = 0;
        if (i >= 0 && i < (long long)a.n) {
            const u64 pos = a.g_begin + (u64)i;
            const u64 w = pos >> 6;
            const u32 b = (u32)(pos & 63);
            sym = 256u | (u32)((a.pl.H[w] >> b) & 1ull) | (u32)((a.pl.L[w] >> b) & 1ull) << 1 | (u32)((a.pl.X[w] >> b) & 1ull) << 2;
            if (EXOTIC) {
#pragma unroll
                for (int e = 0; e < 5; e++) sym |= (u32)((a.pl.E[e][w] >> b) & 1ull) << (3 + e);
            }
        }
        rowsym[r] = sym;
    }
    if (tid < cw) acc[tid] = 0u;
    __syncthreads();

    // ---- raw cells: a thread owns column word c
    {
        const long long jc = j0 + 64ll * (long long)c;                         // column of bit 0 of this word
        const u64 valid = dot_mask_range(-jc, (long long)a.n - jc);            // columns 0 <= j < n
        const u64 ch = prf_fsr(planes[c], planes[c + 1], s);
        const u64 cl = prf_fsr(planes[pstride + c], planes[pstride + c + 1], s);
        const u64 cx = prf_fsr(planes[2 * pstride + c], planes[2 * pstride + c + 1], s);
        u64 ce[5] = {0, 0, 0, 0, 0};
        if (EXOTIC) {
#pragma unroll
            for (int e = 0; e < 5; e++) ce[e] = prf_fsr(planes[(3 + e) * pstride + c], planes[(3 + e) * pstride + c + 1], s);
        }
        for (u32 r = rsub; r < rb; r += rstep) {
            const u32 sym = rowsym[r];
            const u64 hm = (sym & 1u) ? ~0ull : 0ull, lm = (sym & 2u) ? ~0ull : 0ull;
            u64 cell;
            if (sym & 4u) {                                                    // the row's symbol is not ACGT: N or another letter
                cell = cx;
                if (EXOTIC) {
                    u64 diff = 0;
#pragma unroll
                    for (int e = 0; e < 5; e++) diff |= ce[e] ^ ((sym & (8u << e)) ? ~0ull : 0ull);
                    cell &= ~diff;
                }
            } else {
                cell = ~cx & ~((ch ^ hm) | (cl ^ lm));
            }
            raw[(size_t)r * cw + c] = (sym & 256u) ? (cell & valid) : 0ull;
        }
    }
    __syncthreads();

    // ---- the filter and the output
    const u64 ncols = a.col1 - a.col0;
    const u64 gw = span_w0 + (u64)c - 1ull;                                    // the thread's word, in words of the window
    const bool live = c >= 1u && c <= a.span_words && gw < a.words_per_row;
    u32 sum = 0;
    if (live) {
        const u64 tail = ncols - 64ull * gw;                                   // > 0
        const u64 tmask = tail >= 64 ? ~0ull : (1ull << tail) - 1ull;
        for (u32 rr = rsub; rr < DOT_TILE_ROWS; rr += rstep) {
            const u64 i = tr0 + rr;
            if (i >= a.lrow1) break;
            const u32 centre = rr + halo;
            u64 kept = 0;
#pragma unroll 2
            for (u32 aa = 0; aa < m; aa++) {
                u64 wm = ~0ull, wa = ~0ull;
#pragma unroll 2
                for (u32 u = 0; u < m; u++) {
                    const int k = (int)u - (int)aa;
                    wm &= dot_shifted(raw, cw, (u32)((int)centre + k), c, k);
                    wa &= dot_shifted(raw, cw, (u32)((int)centre + k), c, -k);
                }
                kept |= wm | wa;
            }
            kept &= tmask;
            if (MODE == DOT_BITS) a.bits[(i - a.row0) * a.words_per_row + gw] = kept;
            else sum += (u32)__popcll(kept);
        }
    }
    if (MODE == DOT_COUNTS) {
        if (live && sum) atomicAdd(&acc[c], sum);                              // LDS
        __syncthreads();
        if (tid < cw && live) {
            const u64 brow = (tr0 - a.row0) / (64ull * a.wpb);                 // the tile's rows lie in one block row
            u32 *dst = a.counts + brow * a.n_block_cols;
            if (a.wpb == 1u) {
                dst[gw] = acc[c];                                              // the workgroup owns the whole block
            } else if (c == 1u || gw % a.wpb == 0) {                           // first word of a block in this span
                const u64 bcol = gw / a.wpb;
                u32 total = 0;
                for (u32 k = 0; c + k <= a.span_words && gw + k < a.words_per_row && (gw + k) / a.wpb == bcol; k++) total += acc[c + k];
                if (total) atomicAdd(dst + bcol, total);
            }
        }
    }
}

template <int MODE>
hipError_t dot_launch(hipStream_t st, const prf_dotplot_args &a, dim3 grid, size_t lds) {
    const bool exotic = a.pl.E[0] != nullptr;
    if (a.m == 2u) {
        if (exotic) hipLaunchKernelGGL((prf_dotplot_kernel<MODE, true, 2>), grid, dim3(DOT_THREADS), lds, st, a);
        else hipLaunchKernelGGL((prf_dotplot_kernel<MODE, false, 2>), grid, dim3(DOT_THREADS), lds, st, a);
    } else {
        if (exotic) hipLaunchKernelGGL((prf_dotplot_kernel<MODE, true, 0>), grid, dim3(DOT_THREADS), lds, st, a);
        else hipLaunchKernelGGL((prf_dotplot_kernel<MODE, false, 0>), grid, dim3(DOT_THREADS), lds, st, a);
    }
    return hipGetLastError();
}

}  // namespace

// The shape of a launch: the raw rows of a tile (64 + 2 halo) x (span + 2) words and the staged planes (3 or 8: the same shape
// serves both plane sets) fit 64 KiB of LDS
void prf_dotplot_shape_for(u32 min_diagonal_run, u32 *tile_rows, u32 *span_words, u32 *halo) {
    const u32 m = min_diagonal_run > 2u ? min_diagonal_run - 1u : 1u;
    *halo = m - 1u;
    *tile_rows = DOT_TILE_ROWS;
    *span_words = *halo <= 16u ? 62u : 30u;      // up to 96 raw rows of 64 words, or up to 188 of 32: 48 KiB
}

hipError_t prf_launch_dotplot(hipStream_t st, prf_dotplot_args a, bool want_bits) {
    if (!a.n || a.lrow1 <= a.lrow0 || a.col1 <= a.col0) return hipSuccess;
    const bool exotic = a.pl.E[0] != nullptr;
    prf_dotplot_shape_for(a.m + 1u, &a.tile_rows, &a.span_words, &a.halo);
    const u64 n_spans = (a.words_per_row + a.span_words - 1) / a.span_words;
    const u64 n_tiles = (a.lrow1 - a.lrow0 + DOT_TILE_ROWS - 1) / DOT_TILE_ROWS;
    if (n_spans > 0x7fffffffull || n_spans * n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
    a.n_spans = (u32)n_spans;
    const u32 cw = a.span_words + 2u, rb = DOT_TILE_ROWS + 2u * a.halo;
    const size_t lds = ((size_t)(exotic ? 8 : 3) * (cw + 2u) + (size_t)rb * cw) * sizeof(u64) + (((rb + 1u) & ~1u) + cw) * sizeof(u32);
    const dim3 grid((u32)(n_spans * n_tiles));
    return want_bits ? dot_launch<DOT_BITS>(st, a, grid, lds) : dot_launch<DOT_COUNTS>(st, a, grid, lds);
}
