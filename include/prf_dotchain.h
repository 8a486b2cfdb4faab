/*
 * prf_dotchain.h -- the entry points of libprf that list the diagonal repeats WITH MISMATCHES of the dot plot of two ranges: exact
 * runs of one diagonal or anti-diagonal, chained across short stretches of mismatches.  Part of the C ABI of include/prf.h,
 * which includes this file inside its extern "C" block (include prf.h, not this file).  They live in a header of their own so
 * that the lists of entry points of prf.h proper, prf_period.h, prf_dotplot.h, prf_dotpair.h and prf_dotruns.h stay what they
 * were; these are prf_native.DOTCHAIN_EXPORTS.
 */
#ifndef PRF_DOTCHAIN_H
#define PRF_DOTCHAIN_H
#ifndef PRF_H
#error "include prf.h, which includes prf_dotchain.h"
#endif

/* ---- chains of exact runs on one diagonal or anti-diagonal of the dot plot of two ranges ----
 * A, B, na, nb, strand, raw(i, j), the clipping of each end to its contig, the window and `directions` are exactly those of
 * prf_dotruns.h.
 * A LINE is one diagonal (dir 1) or one anti-diagonal (dir 2) of the whole na x nb rectangle; its cells are numbered t = 0, 1, ...
 * from the cell with the smallest row.  On a line, the SEEDS are the maximal runs of raw cells with len >= min_seed (the runs of
 * prf_dotpair_runs at min_len = min_seed).  Two seeds that follow each other on a line are LINKED if the number of cells
 * strictly between them is <= max_gap: with the first seed's last cell at e and the next seed's first cell at s the gap is
 * s - e - 1 >= 1.  Shorter runs inside the gap are not seeds and link nothing.  A CHAIN is a maximal sequence of consecutive
 * linked seeds.
 * row, col: the first seed's start cell, relative to a_begin and b_begin (on an anti line col is the largest column).
 * len: the cells from the first seed's first cell to the last seed's last cell.  matches: the raw cells among those len cells
 * (short runs inside the gaps count; nothing before the first seed or behind the last one does).  seeds: the seeds of the chain.
 * A call reports the chains whose START CELL lies in the window rows [row0, row1) (clipped to na) x columns [col0, col1) (clipped
 * to nb), whose direction is in `directions` and whose len >= min_len (0: no filter).  Seeds and links are judged in the whole
 * rectangle, never clipped by the window: a seed in the window whose predecessor lies outside it is not a start.  The lists of a
 * partition of the rectangle into windows therefore add up to the whole list, each chain once.  The rows come back sorted
 * ascending by (row, col, dir).
 * Hence: at max_gap = 0 the list is that of prf_dotpair_runs at min_len = max(min_seed, min_len), with matches = len and
 * seeds = 1; at any max_gap the seeds of all chains are exactly the runs of that call at min_len = min_seed;
 * matches >= seeds * min_seed; len - matches <= (seeds - 1) * max_gap.
 * *n_chains is always the number of chains found.  dst is written -- all *n_chains rows, sorted -- only if *n_chains <= capacity;
 * otherwise dst is left untouched and the call still returns PRF_OK: compare and call again.  dst == NULL with capacity == 0
 * counts only.
 * Refusals, judged before the context or the genome is looked at, in this order: PRF_EINVAL for a_begin > a_end, b_begin > b_end,
 * row0 > row1, col0 > col1, strand > 1, directions 0 or above 3, min_seed == 0; PRF_EUNSUPPORTED for max_gap above
 * PRF_DOTCHAIN_MAX_GAP and for a capacity above PRF_DOTCHAIN_MAX_ROWS; PRF_EINVAL for a NULL n_chains, or a NULL dst with a
 * capacity other than 0.  Once the lengths are known (the one-shot form: still before the context): PRF_EUNSUPPORTED for a window
 * above PRF_DOT_MAX_CELLS cells.  PRF_EINVAL for a contig the genome does not hold or a genome of another context.
 * PRF_EUNSUPPORTED, loudly and never a wrong list, if more than PRF_DOTCHAIN_MAX_ROWS seeds start in the window (ask for smaller
 * windows or a larger min_seed), or if the runs or chains that are still going after PRF_DOTRUN_FOLLOW / PRF_DOTCHAIN_FOLLOW cells
 * outnumber the lists the call keeps them in.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the other matrix products.
 * Stats: path = 8, scan_ms = HIP-event time of all launches (phase1_ms: the seed kernels', phase2_ms: the chain kernels'),
 * positions = na + nb, n_candidates = the seeds of the window, n_hits = *n_chains, n_launches.
 * The _ex form cuts the window's rows into launches of the seed kernel of at most launch_cells cells (0: the default), for the
 * tests.  The one-shot form takes two sequences of ASCII, which may be the same (prf_genome_load of both + the call +
 * prf_genome_free; PRF_ESYMBOL for a byte that is not a letter, found on the host before the context is looked at). */
typedef struct prf_dotchain {
    uint64_t row, col; /* the first seed's start cell, relative to a_begin / b_begin                         */
    uint64_t len;      /* cells from the first seed's first cell to the last seed's last cell                */
    uint64_t matches;  /* raw cells among them                                                               */
    uint32_t dir;      /* 1 main (i + s, j + s), 2 anti (i + s, j - s)                                       */
    uint32_t seeds;    /* exact runs of at least min_seed cells in the chain                                 */
} prf_dotchain;

#define PRF_DOTCHAIN_MAX_GAP 4096u          /* cells between two linked seeds: one look for the next seed is at most 64 word steps */
#define PRF_DOTCHAIN_MAX_ROWS (1ull << 24)  /* rows of dst per call, and seeds of a window                                        */
#define PRF_DOTCHAIN_LONG_ROWS (1ull << 20) /* chains still going after PRF_DOTCHAIN_FOLLOW cells a call can finish              */
#define PRF_DOTCHAIN_FOLLOW 2048u /* cells a chain is followed for behind its first seed by the thread that owns the seed; one wave finishes the rest */

int prf_dotpair_chains(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                       uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                       uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                       prf_dotchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats);
int prf_dotpair_chains_ex(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end,
                          uint32_t b_contig, uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1,
                          uint64_t col0, uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap,
                          uint64_t min_len, prf_dotchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats,
                          uint64_t launch_cells);
int prf_dotpair_chains_seq(prf_ctx *ctx, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                           uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                           uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                           prf_dotchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats);

#endif /* PRF_DOTCHAIN_H */
