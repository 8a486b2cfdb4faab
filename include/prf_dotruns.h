/*
 * prf_dotruns.h -- the entry points of libprf that list the diagonal runs of the dot plot of two ranges as coordinates: part of
 * the C ABI of include/prf.h, which includes this file inside its extern "C" block (include prf.h, not this file).  They live in
 * a header of their own so that the lists of entry points of prf.h proper, prf_period.h, prf_dotplot.h and prf_dotpair.h --
 * prf_native.EXPORTS, PERIOD_EXPORTS, DOTPLOT_EXPORTS and DOTPAIR_EXPORTS -- stay what they were; these are
 * prf_native.DOTRUNS_EXPORTS.
 */
#ifndef PRF_DOTRUNS_H
#define PRF_DOTRUNS_H
#ifndef PRF_H
#error "include prf.h, which includes prf_dotruns.h"
#endif

/* ---- the maximal diagonal and anti-diagonal runs of the dot plot of two ranges ----
 * A, B, na, nb, strand, comp, raw(i, j) and the clipping of each end to its contig are exactly those of prf_dotpair.h: N == N is
 * a match, any other letter matches itself, on the minus strand the row is compared with the complement of the column.
 * A MAIN run (dir 1) is a maximal set of cells (i + s, j + s), 0 <= s < len, that are all raw: its start (i, j) has i == 0 or
 * j == 0 or !raw(i - 1, j - 1), its end has i + len == na or j + len == nb or !raw(i + len, j + len).
 * An ANTI run (dir 2) is a maximal set (i + s, j - s): its start is the cell with the smallest row, i == 0 or j == nb - 1 or
 * !raw(i - 1, j + 1); col is the start cell's column, the largest of the run.
 * Maximality is taken in the whole na x nb rectangle: runs are clipped by the rectangle's bounds and by nothing else, not by the
 * window and not by a contig's end behind a_end / b_end.  Nothing at or behind either end is compared or read.
 * A call reports the runs whose START CELL lies in the window rows [row0, row1) (clipped to na) x columns [col0, col1) (clipped to
 * nb), whose direction is in `directions` (bit 0: main, bit 1: anti) and whose len >= min_len.  len is never clipped by the
 * window, so the lists of a partition of the rectangle into windows add up to the whole list, each run once.  row and col are
 * relative to a_begin and b_begin.  The rows come back sorted ascending by (row, col, dir).
 * With t = min_diagonal_run of prf_dotpair_bits: for t >= 3 the cells of all runs of both directions with len >= t - 1 are the
 * kept cells; the cells of the runs at min_len 1 are the raw cells.
 * *n_runs is always the number of runs found.  dst is written -- all *n_runs rows, sorted -- only if *n_runs <= capacity;
 * otherwise dst is left untouched and the call still returns PRF_OK: compare and call again.  dst == NULL with capacity == 0
 * counts only.
 * Refusals, judged before the context or the genome is looked at, in this order: PRF_EINVAL for a_begin > a_end, b_begin > b_end,
 * row0 > row1, col0 > col1, strand > 1, directions 0 or above 3, min_len == 0; PRF_EUNSUPPORTED for a capacity above
 * PRF_DOTRUN_MAX_ROWS; PRF_EINVAL for a NULL n_runs, or a NULL dst with a capacity other than 0.  Once the lengths are known (the
 * one-shot form: still before the context): PRF_EUNSUPPORTED for a window above PRF_DOT_MAX_CELLS cells.  PRF_EINVAL for a contig
 * the genome does not hold or a genome of another context.  PRF_EUNSUPPORTED, loudly and never a wrong list, if the runs longer
 * than PRF_DOTRUN_FOLLOW that start in the window outnumber the list the call keeps them in (PRF_DOTRUN_LONG_ROWS, or fewer where
 * the rectangle cannot hold that many): ask for smaller windows.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the other matrix products.
 * Stats: path = 7, scan_ms = HIP-event time of all launches, positions = na + nb, n_hits = *n_runs, n_launches.
 * The _ex form cuts the window's rows into launches of at most launch_cells cells (0: the default), for the tests.
 * The one-shot form takes two sequences of ASCII, which may be the same (prf_genome_load of both + the call + prf_genome_free;
 * PRF_ESYMBOL for a byte that is not a letter, found on the host before the context is looked at). */
typedef struct prf_dotrun {
    uint64_t row, col, len; /* the start cell, relative to a_begin / b_begin, and the cells of the run */
    uint32_t dir;           /* 1 main (i + s, j + s), 2 anti (i + s, j - s)                            */
    uint32_t reserved;      /* 0                                                                       */
} prf_dotrun;

#define PRF_DOTRUN_MAIN 1u
#define PRF_DOTRUN_ANTI 2u
#define PRF_DOTRUN_MAX_ROWS (1ull << 24)  /* rows of dst per call                                                              */
#define PRF_DOTRUN_LONG_ROWS (1ull << 20) /* runs longer than PRF_DOTRUN_FOLLOW a call can finish                              */
#define PRF_DOTRUN_PROBE 16u    /* cells a start is probed for in the tile before it is followed: min(min_len, this); <= 63      */
#define PRF_DOTRUN_FOLLOW 2048u /* cells a run is followed for by the thread that found it; longer runs are finished by one wave */

int prf_dotpair_runs(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                     uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                     uint64_t col1, uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity, uint64_t *n_runs,
                     prf_scan_stats *stats);
int prf_dotpair_runs_ex(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                        uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                        uint64_t col1, uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity,
                        uint64_t *n_runs, prf_scan_stats *stats, uint64_t launch_cells);
int prf_dotpair_runs_seq(prf_ctx *ctx, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                         uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                         uint64_t col1, uint32_t directions, uint64_t min_len, prf_dotrun *dst, uint64_t capacity,
                         uint64_t *n_runs, prf_scan_stats *stats);

#endif /* PRF_DOTRUNS_H */
