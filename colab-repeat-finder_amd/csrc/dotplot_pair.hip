// dotplot_pair.hip -- the exact dot plot of TWO ranges of a resident genome, on either strand:
//   raw(i, j) = A[i] == B[j]  (strand 0)   or   A[i] == comp(B[j])  (strand 1),
// A = na positions from a_g_begin (the rows), B = nb positions from b_g_begin (the columns, in B's forward coordinates on both
// strands), by plain comparison of symbols as in dotplot.hip; comp swaps A/T, C/G, R/Y, K/M, B/V, D/H and leaves every other
// letter (N, S, W, ...) alone.  kept(i, j) is the closed form of DESIGN 11.1 on the na x nb rectangle: runs are clipped by the
// rectangle's bounds alone, so rows outside [0, na) and columns outside [0, nb) are zero and nothing at or behind either
// range's end is read.
//
// The kernel is prf_dotplot_kernel (dotplot.hip: tile, spans, LDS shape, filter, counts -- read the description there) with
// four differences, all before the raw cells are written:
//   the row symbols come from A's positions, a row exists for 0 <= i < na;
//   the column words are staged from B's positions, zero outside B's words;
//   the column validity mask is built against nb;
//   on the minus strand the staged ROW symbol is complemented (A[i] == comp(B[j]) <=> comp(A[i]) == B[j]): with the base code
//   A=0 C=1 T=2 G=3 that flips the high code bit H of an ACGT row; a row with X set and a letter code goes through
//   dot_comp_letter; an N row (X alone) stays.  The per-cell loop is the same.
// The self plot keeps its own translation unit and its own copies of the two helpers, so that its kernels are compiled from
// the text they were compiled from before.
// NOTE: dotplot.hip repeats this file's kernel and its two helpers (the two are kept apart so that a change to one cannot alter the
// instructions of the other's instances).
// A fix to the staging, the filter or the count section belongs in BOTH files; tests/test_dotpair_gpu.py compares the two
// kernels bit for bit on a few windows (pair(A, A, +) = the self plot) and nothing else keeps them in step.
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

// the complement of a letter outside ACGTN by its 5-bit code (A = 1 ... Z = 26; 0: N, which stays): R <-> Y, K <-> M, B <-> V,
// D <-> H; S, W and every other letter map to themselves
__device__ __forceinline__ u32 dot_comp_letter(u32 e) {
    switch (e) {
        case 18u: return 25u;   // R -> Y
        case 25u: return 18u;
        case 11u: return 13u;   // K -> M
        case 13u: return 11u;
        case 2u: return 22u;    // B -> V
        case 22u: return 2u;
        case 4u: return 8u;     // D -> H
        case 8u: return 4u;
        default: return e;
    }
}

template <int MODE, bool EXOTIC, int MFIX>
__global__ __launch_bounds__(DOT_THREADS) void prf_dotpair_kernel(const prf_dotpair_args a) {
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
    const u64 tr0 = a.lrow0 + (u64)ti * DOT_TILE_ROWS; // first row of the tile, relative to A
    const u64 wfirst = a.b_g_begin >> 6, wlast = (a.b_g_begin + a.nb - 1) >> 6;   // the words of the planes that hold B

    // ---- stage the column words: LDS word i of a plane = plane word sw0 + i, or 0 outside B's words
    const long long j0 = (long long)a.col0 + 64ll * ((long long)span_w0 - 1ll);   // column of bit 0 of LDS word 0 (may be < 0)
    const long long q0 = (long long)a.b_g_begin + j0;
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
    // ---- the symbols of the rows, from A: bit 0 H, 1 L, 2 X, 3..7 E, 8 = the row exists; complemented on the minus strand
    for (u32 r = tid; r < rb; r += DOT_THREADS) {
        const long long i = (long long)tr0 - (long long)halo + (long long)r;
        u32 sym = 0;
        if (i >= 0 && i < (long long)a.na) {
            const u64 pos = a.a_g_begin + (u64)i;
            const u64 w = pos >> 6;
            const u32 b = (u32)(pos & 63);
            sym = 256u | (u32)((a.pl.H[w] >> b) & 1ull) | (u32)((a.pl.L[w] >> b) & 1ull) << 1 | (u32)((a.pl.X[w] >> b) & 1ull) << 2;
            if (EXOTIC) {
#pragma unroll
                for (int e = 0; e < 5; e++) sym |= (u32)((a.pl.E[e][w] >> b) & 1ull) << (3 + e);
            }
            if (a.strand) {
                if (!(sym & 4u)) sym ^= 1u;                                    // A <-> T, C <-> G
                else if (EXOTIC) sym = (sym & ~(31u << 3)) | dot_comp_letter((sym >> 3) & 31u) << 3;
            }
        }
        rowsym[r] = sym;
    }
    if (tid < cw) acc[tid] = 0u;
    __syncthreads();

    // ---- raw cells: a thread owns column word c
    {
        const long long jc = j0 + 64ll * (long long)c;                         // column of bit 0 of this word
        const u64 valid = dot_mask_range(-jc, (long long)a.nb - jc);           // columns 0 <= j < nb
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
hipError_t pair_launch(hipStream_t st, const prf_dotpair_args &a, dim3 grid, size_t lds) {
    const bool exotic = a.pl.E[0] != nullptr;
    if (a.m == 2u) {
        if (exotic) hipLaunchKernelGGL((prf_dotpair_kernel<MODE, true, 2>), grid, dim3(DOT_THREADS), lds, st, a);
        else hipLaunchKernelGGL((prf_dotpair_kernel<MODE, false, 2>), grid, dim3(DOT_THREADS), lds, st, a);
    } else {
        if (exotic) hipLaunchKernelGGL((prf_dotpair_kernel<MODE, true, 0>), grid, dim3(DOT_THREADS), lds, st, a);
        else hipLaunchKernelGGL((prf_dotpair_kernel<MODE, false, 0>), grid, dim3(DOT_THREADS), lds, st, a);
    }
    return hipGetLastError();
}

}  // namespace

// The launch shape is the self plot's (prf_dotplot_shape_for, dotplot.hip): the same LDS serves both kernels.
hipError_t prf_launch_dotpair(hipStream_t st, prf_dotpair_args a, bool want_bits) {
    if (!a.na || !a.nb || a.lrow1 <= a.lrow0 || a.col1 <= a.col0) return hipSuccess;
    if (a.strand > 1u) return hipErrorInvalidValue;
    const bool exotic = a.pl.E[0] != nullptr;
    prf_dotplot_shape_for(a.m + 1u, &a.tile_rows, &a.span_words, &a.halo);
    const u64 n_spans = (a.words_per_row + a.span_words - 1) / a.span_words;
    const u64 n_tiles = (a.lrow1 - a.lrow0 + DOT_TILE_ROWS - 1) / DOT_TILE_ROWS;
    if (n_spans > 0x7fffffffull || n_spans * n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
    a.n_spans = (u32)n_spans;
    const u32 cw = a.span_words + 2u, rb = DOT_TILE_ROWS + 2u * a.halo;
    const size_t lds = ((size_t)(exotic ? 8 : 3) * (cw + 2u) + (size_t)rb * cw) * sizeof(u64) + (((rb + 1u) & ~1u) + cw) * sizeof(u32);
    const dim3 grid((u32)(n_spans * n_tiles));
    return want_bits ? pair_launch<DOT_BITS>(st, a, grid, lds) : pair_launch<DOT_COUNTS>(st, a, grid, lds);
}
