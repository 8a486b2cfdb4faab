// dotruns.hip -- the diagonal runs of the dot plot of two ranges as a list of coordinates: every maximal stretch of
// raw cells along (+1, +1) (main, dir 1) or (+1, -1) (anti, dir 2) of the na x nb rectangle of dotplot_pair.hip whose START cell
// (the one with the smallest row) lies in the window, of any length, once, as (row, col, len, dir).
//
// prf_dotruns_find_kernel tiles the window as prf_dotpair_kernel does (64 rows x a span of 62 column words, one workgroup each;
// the column planes staged with zeros outside B's words, the row symbols complemented on the minus strand, the column validity
// mask against nb, the raw rows in LDS) with a halo of ONE row above (the predecessor) and p - 1 rows below, p = min(min_len,
// PRF_DOTRUN_PROBE).  Per owned word
//     main starts = raw[r] & ~shifted(raw[r - 1], -1) & AND_{u = 1 .. p - 1} shifted(raw[r + u], +u)
// and the anti starts with the signs of the shifts swapped: O(p) looks per word.  A set bit is a run of at least p cells; the
// thread that owns the word FOLLOWS it on the planes in global memory, 64 cells per step (dr_step), up to PRF_DOTRUN_FOLLOW
// cells.  A run that ends within them and has min_len cells goes to the workgroup's list in LDS; a run that is still going goes
// to the long list in device memory, which prf_dotruns_long_kernel finishes with one wave per entry, 64 lanes x 64 cells a step.
// The LDS list is flushed with ONE global atomic per flush (thread 0 reserves the slots of all its entries); the total is
// counted past `capacity`, nothing is written past it.
// No address outside the words wfirst .. wlast of the planes that hold a range is ever formed (dr_bits): the anti look
// backwards at b_begin = 0 of contig 0 and the look ahead in the last word of the last contig read zeros instead.
// dr_step, dr_bits, dr_words, dr_is_letter and dot_comp_letter live in dotruns_step.h, which dotchain.hip includes too.
// NOTE: dot_mask_range, dot_shifted and dot_comp_letter and the staging are repeated from dotplot_pair.hip (each
// kernel keeps its own translation unit, so that a change here cannot alter the instructions of the other's instances).  A fix
// to the staging or the raw cells belongs in all three files.
#include "../../include/prf.h"
#include "prf_host.h"
#include "dotruns_step.h"

#define DR_THREADS 256
#define DR_TILE_ROWS 64u
#define DR_SPAN_WORDS 62u
#define DR_LIST 1024u          // entries of the workgroup's list; flushed while a round could overflow it

static_assert(sizeof(prf_dotrun_dev) == sizeof(prf_dotrun) && sizeof(prf_dotrun) == 32, "prf_dotrun is 32 bytes");
static_assert(PRF_DOTRUN_PROBE >= 2 && PRF_DOTRUN_PROBE <= 63, "the probe must fit the one-word column halo of the span");
static_assert(PRF_DOTRUN_FOLLOW % 64 == 0 && PRF_DOTRUN_FOLLOW >= 64, "the follow limit is a multiple of 64");

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

template <bool EXOTIC>
__global__ __launch_bounds__(DR_THREADS) void prf_dotruns_find_kernel(const prf_dotruns_args a) {
    extern __shared__ __attribute__((aligned(16))) u64 dr_lds[];
    constexpr int NP = EXOTIC ? 8 : 3;
    const u32 p = a.p;
    const u32 cw = a.span_words + 2u;                  // 64: LDS words per raw row
    const u32 rb = DR_TILE_ROWS + p;                   // raw rows in LDS: one above, the tile's, p - 1 below
    const u32 pstride = cw + 2u;                       // LDS words per staged plane (cw + 1 used)
    u64 *const planes = dr_lds;
    u64 *const raw = dr_lds + (size_t)NP * pstride;
    u64 *const list = raw + (size_t)rb * cw;           // DR_LIST entries: len << 32 | dir << 18 | column in the span << 6 | row in the tile
    u32 *const rowsym = (u32 *)(list + DR_LIST);
    u32 *const ctl = rowsym + ((rb + 1u) & ~1u);       // [0]: entries of the list; [2..3]: the slots a flush reserved (u64)

    const u32 tid = threadIdx.x;
    const u32 c = tid & (cw - 1u), rsub = tid / cw, rstep = DR_THREADS / cw;
    const u32 sp = blockIdx.x % a.n_spans, ti = blockIdx.x / a.n_spans;
    const u64 span_w0 = (u64)sp * a.span_words;        // first word of the span, in words of the window
    const u64 tr0 = a.lrow0 + (u64)ti * DR_TILE_ROWS;  // first row of the tile, relative to A
    const u64 wfirst = a.b_g_begin >> 6, wlast = (a.b_g_begin + a.nb - 1) >> 6;   // the words of the planes that hold B

    // ---- stage the column words: LDS word i of a plane = plane word sw0 + i, or 0 outside B's words
    const long long j0 = (long long)a.col0 + 64ll * ((long long)span_w0 - 1ll);   // column of bit 0 of LDS word 0 (may be < 0)
    const long long q0 = (long long)a.b_g_begin + j0;
    const long long sw0 = q0 >> 6;
    const u32 s = (u32)(q0 & 63);
    {
        const u64 *const P[8] = {a.pl.H, a.pl.L, a.pl.X, a.pl.E[0], a.pl.E[1], a.pl.E[2], a.pl.E[3], a.pl.E[4]};
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
            const u64 *__restrict__ src = P[pp];
            for (u32 i = tid; i < cw + 1u; i += DR_THREADS) {
                const long long wi = sw0 + (long long)i;
                planes[(size_t)pp * pstride + i] = (wi >= (long long)wfirst && wi <= (long long)wlast) ? src[wi] : 0ull;
            }
        }
    }
    // ---- the symbols of the rows, from A: bit 0 H, 1 L, 2 X, 3..7 E, 8 = the row exists; complemented on the minus strand
    for (u32 r = tid; r < rb; r += DR_THREADS) {
        const long long i = (long long)tr0 - 1ll + (long long)r;
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
    if (tid == 0) ctl[0] = 0u;
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

    // ---- starts, follow, list.  Every thread walks the same rounds and the same barriers; a thread without work idles through them.
    const dr_words words = dr_words_of(a);
    const u64 ncols = a.col1 - a.col0;
    const u64 gw = span_w0 + (u64)c - 1ull;                                    // the thread's word, in words of the window
    const bool live = c >= 1u && c <= a.span_words && gw < a.words_per_row;
    u64 tmask = 0;
    if (live) {
        const u64 tail = ncols - 64ull * gw;                                   // > 0
        tmask = tail >= 64 ? ~0ull : (1ull << tail) - 1ull;
    }
    // the slots of the list's n entries are reserved with one global atomic; rows behind `capacity` are counted, not written
    auto flush = [&](u32 n) {
        if (tid == 0) {
            *(u64 *)(ctl + 2) = atomicAdd(a.counters + PRF_DR_RUNS, (u64)n);
            ctl[0] = 0u;
        }
        __syncthreads();
        const u64 base = *(const u64 *)(ctl + 2);
        for (u32 e = tid; e < n; e += DR_THREADS) {
            const u64 v = list[e], at = base + e;
            if (at < a.capacity) {
                const u32 code = (u32)v;
                prf_dotrun_dev out;
                out.row = tr0 + (code & 63u);
                out.col = (u64)(j0 + (long long)((code >> 6) & 4095u));
                out.len = v >> 32;
                out.dir = code >> 18;
                out.reserved = 0u;
                a.dst[at] = out;
            }
        }
        __syncthreads();
    };
    for (u32 rr0 = 0; rr0 < DR_TILE_ROWS; rr0 += rstep) {
        const u32 rr = rr0 + rsub;
        const u64 i = tr0 + rr;
        u64 m_main = 0, m_anti = 0;
        if (live && i < a.lrow1) {
            const u32 r = rr + 1u;
            const u64 here = raw[(size_t)r * cw + c] & tmask;
            if (here) {
                if (a.directions & PRF_DOTRUN_MAIN) {
                    m_main = here & ~dot_shifted(raw, cw, r - 1u, c, -1);
                    for (u32 u = 1; u < p && m_main; u++) m_main &= dot_shifted(raw, cw, r + u, c, (int)u);
                }
                if (a.directions & PRF_DOTRUN_ANTI) {
                    m_anti = here & ~dot_shifted(raw, cw, r - 1u, c, 1);
                    for (u32 u = 1; u < p && m_anti; u++) m_anti &= dot_shifted(raw, cw, r + u, c, -(int)u);
                }
            }
        }
        for (;;) {
            const u32 listed = *(volatile u32 *)ctl;                           // stable: entries are added between the two barriers below
            if (!__syncthreads_or((m_main | m_anti) != 0ull)) break;
            if (listed + DR_THREADS > DR_LIST) flush(listed);                  // the same decision in every thread
            if (m_main | m_anti) {
                const u32 dir = m_main ? PRF_DOTRUN_MAIN : PRF_DOTRUN_ANTI;
                u64 &m = m_main ? m_main : m_anti;
                const u32 b = (u32)__builtin_ctzll(m);
                m &= m - 1ull;
                const u64 j = (u64)(j0 + 64ll * (long long)c + (long long)b);
                u64 len = 0;
                bool going = true;
#pragma unroll 1
                for (u64 done = 0; done < PRF_DOTRUN_FOLLOW; done += 64) {
                    const u64 mism = dr_step<EXOTIC>(a, words, i, j, dir, done);
                    if (mism) {
                        len = done + (u64)__builtin_ctzll(mism);
                        going = false;
                        break;
                    }
                }
                if (going) {                                                   // rare: at least PRF_DOTRUN_FOLLOW cells each
                    const u64 at = atomicAdd(a.counters + PRF_DR_LONG, 1ull);
                    if (at < a.long_cap) a.longs[at] = prf_dotrun_dev{i, j, (u64)PRF_DOTRUN_FOLLOW, dir, 0u};
                } else if (len >= a.min_len) {
                    const u32 at = atomicAdd(&ctl[0], 1u);                     // LDS; below DR_LIST by the flush above
                    list[at] = len << 32 | (u64)(dir << 18 | (c * 64u + b) << 6 | rr);
                }
            }
            __syncthreads();
        }
    }
    const u32 listed = ctl[0];                                                 // behind the last barrier of the rounds
    if (listed) flush(listed);
}

// One wave per entry of the long list: lane l compares cells len + 4096 t + 64 l .. + 63 in step t, a ballot finds the first lane
// with a mismatch or the rectangle's edge.
template <bool EXOTIC>
__global__ __launch_bounds__(DR_THREADS) void prf_dotruns_long_kernel(const prf_dotruns_args a, const u64 n_long) {
    const u32 lane = threadIdx.x & 63u;
    const u64 entry = (u64)blockIdx.x * (DR_THREADS / 64u) + (threadIdx.x >> 6);
    if (entry >= n_long) return;                                               // the whole wave
    const prf_dotrun_dev e = a.longs[entry];
    const dr_words words = dr_words_of(a);
    u64 done = e.len;
    for (;;) {
        const u64 mism = dr_step<EXOTIC>(a, words, e.row, e.col, e.dir, done + 64ull * lane);
        const u64 vote = __ballot(mism != 0ull);
        if (vote) {
            const u32 first = (u32)__builtin_ctzll(vote);
            const u64 len = done + 64ull * first + (u64)__builtin_ctzll(__shfl(mism, (int)first));   // that lane's word is not 0
            if (lane == 0 && len >= a.min_len) {
                const u64 at = atomicAdd(a.counters + PRF_DR_RUNS, 1ull);
                if (at < a.capacity) a.dst[at] = prf_dotrun_dev{e.row, e.col, len, e.dir, 0u};
            }
            return;
        }
        done += 4096ull;                                                       // ends: dr_step reports the edge as a mismatch
    }
}

}  // namespace

hipError_t prf_launch_dotruns_find(hipStream_t st, prf_dotruns_args a) {
    if (!a.na || !a.nb || a.lrow1 <= a.lrow0 || a.col1 <= a.col0) return hipSuccess;
    if (a.strand > 1u || !a.p || a.p > PRF_DOTRUN_PROBE || a.p > a.min_len || !(a.directions & 3u)) return hipErrorInvalidValue;
    const bool exotic = a.pl.E[0] != nullptr;
    a.span_words = DR_SPAN_WORDS;
    const u64 n_spans = (a.words_per_row + a.span_words - 1) / a.span_words;
    const u64 n_tiles = (a.lrow1 - a.lrow0 + DR_TILE_ROWS - 1) / DR_TILE_ROWS;
    if (n_spans > 0x7fffffffull || n_spans * n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
    a.n_spans = (u32)n_spans;
    const u32 cw = a.span_words + 2u, rb = DR_TILE_ROWS + a.p;
    const size_t lds = ((size_t)(exotic ? 8 : 3) * (cw + 2u) + (size_t)rb * cw + DR_LIST) * sizeof(u64) + (((rb + 1u) & ~1u) + 4u) * sizeof(u32);
    const dim3 grid((u32)(n_spans * n_tiles));
    if (exotic) hipLaunchKernelGGL((prf_dotruns_find_kernel<true>), grid, dim3(DR_THREADS), lds, st, a);
    else hipLaunchKernelGGL((prf_dotruns_find_kernel<false>), grid, dim3(DR_THREADS), lds, st, a);
    return hipGetLastError();
}

hipError_t prf_launch_dotruns_long(hipStream_t st, const prf_dotruns_args &a, u64 n_long) {
    if (!n_long) return hipSuccess;
    if (n_long > a.long_cap || !a.na || !a.nb) return hipErrorInvalidValue;
    const dim3 grid((u32)((n_long + DR_THREADS / 64 - 1) / (DR_THREADS / 64)));
    if (a.pl.E[0] != nullptr) hipLaunchKernelGGL((prf_dotruns_long_kernel<true>), grid, dim3(DR_THREADS), 0, st, a, n_long);
    else hipLaunchKernelGGL((prf_dotruns_long_kernel<false>), grid, dim3(DR_THREADS), 0, st, a, n_long);
    return hipGetLastError();
}
