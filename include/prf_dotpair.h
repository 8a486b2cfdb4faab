/*
 * prf_dotpair.h -- the entry points of libprf for the dot plot of two ranges, on either strand: part of the C ABI of
 * include/prf.h, which includes this file inside its extern "C" block (include prf.h, not this file).  They live in a header of
 * their own so that the lists of entry points of prf.h proper, prf_period.h and prf_dotplot.h -- prf_native.EXPORTS,
 * PERIOD_EXPORTS and DOTPLOT_EXPORTS -- stay what they were; these are prf_native.DOTPAIR_EXPORTS.
 */
#ifndef PRF_DOTPAIR_H
#define PRF_DOTPAIR_H
#ifndef PRF_H
#error "include prf.h, which includes prf_dotpair.h"
#endif

/* ---- exact dot plot of two ranges of a resident genome ----
 * A = positions [a_begin, a_end) of contig a_contig (the rows), B = positions [b_begin, b_end) of contig b_contig (the columns),
 * both contigs of the same genome, both ranges upper-cased.  Each end is clipped to its contig: na = len(A), nb = len(B).  The
 * contigs may be the same one, the ranges may overlap or be equal.
 * strand 0 (plus):   raw(i, j) = (A[i] == B[j]), the plain comparison of symbols of prf_dotplot.h (N == N IS a match, any other
 *                    letter matches itself and nothing else);
 * strand 1 (minus):  raw(i, j) = (A[i] == comp(B[j])); comp maps A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H, and N, S, W and
 *                    every other letter to themselves.
 * Columns are in B's forward coordinates on both strands: an inverted repeat (u ... revcomp(u)) is an anti-diagonal run of the
 * minus matrix, a complemented direct copy a main-diagonal run of it.
 * With t = min_diagonal_run,
 *     kept(i, j)  <=>  raw(i, j) and (Lmain(i, j) + 1 >= t  or  Lanti(i, j) + 1 >= t)
 * Lmain / Lanti: the length of the maximal run of raw cells through (i, j) along (+1, +1) / (+1, -1) in the unfiltered na x nb
 * rectangle, clipped by the rectangle's bounds and by nothing else: not by the window, and not by a contig's end behind a_end /
 * b_end.  t <= 2 filters nothing.  Nothing at or behind either end is compared or read.
 * A call computes the window rows [row0, row1) (clipped to na) x columns [col0, col1) (clipped to nb); its cells equal the same
 * cells of the whole rectangle.
 * The layouts of the bits and of the counts, `block`, the limits (min_diagonal_run <= PRF_DOT_MAX_RUN, PRF_PERIOD_BITS_MAX_WORDS
 * entries of output, PRF_DOT_MAX_CELLS cells per call, launches of PRF_DOT_LAUNCH_CELLS / ceil(m^2 / 4) cells, the _ex forms'
 * launch_cells), the treatment of a selection of parts, a row sink and the rows of the last scan (all left alone) are those of
 * prf_dotplot.h.
 * pair(A, A, plus) is prf_dotplot_bits of the same range, bit for bit; pair(A, B, s) transposed is pair(B, A, s);
 * pair(A, B, minus)[i][j] = pair(A, revcomp(B), plus)[i][nb - 1 - j].
 * Refusals, judged before the context or the genome is looked at, in this order: PRF_EINVAL for a block that is no multiple of
 * 64 in 64 .. 32768 (counts), a_begin > a_end, b_begin > b_end, row0 > row1, col0 > col1, strand > 1; PRF_EUNSUPPORTED for
 * min_diagonal_run > 64; PRF_EINVAL for a NULL dst or size pointer.  Once the lengths are known (the one-shot forms: still before
 * the context): PRF_EINVAL if dst holds fewer than the output's entries, PRF_EUNSUPPORTED above the limits.  PRF_EINVAL for a
 * contig the genome does not hold or a genome of another context.
 * Stats: path = 6, scan_ms = HIP-event time of the launches, positions = na + nb, n_hits = 0, n_launches.
 * The one-shot forms take two sequences of ASCII, which may be the same (prf_genome_load of both + the call + prf_genome_free;
 * PRF_ESYMBOL for a byte that is not a letter, found on the host before the context is looked at). */
int prf_dotpair_bits(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                     uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                     uint64_t col1, uint32_t min_diagonal_run, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row,
                     prf_scan_stats *stats);
int prf_dotpair_counts(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                       uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                       uint64_t col1, uint32_t min_diagonal_run, uint64_t block, uint32_t *dst, uint64_t capacity,
                       uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats);
int prf_dotpair_bits_ex(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                        uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                        uint64_t col1, uint32_t min_diagonal_run, uint64_t *dst, uint64_t capacity_words,
                        uint64_t *words_per_row, prf_scan_stats *stats, uint64_t launch_cells);
int prf_dotpair_counts_ex(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end,
                          uint32_t b_contig, uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1,
                          uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t block, uint32_t *dst,
                          uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats,
                          uint64_t launch_cells);
int prf_dotpair_bits_seq(prf_ctx *ctx, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                         uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                         uint64_t col1, uint32_t min_diagonal_run, uint64_t *dst, uint64_t capacity_words,
                         uint64_t *words_per_row, prf_scan_stats *stats);
int prf_dotpair_counts_seq(prf_ctx *ctx, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                           uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                           uint64_t col1, uint32_t min_diagonal_run, uint64_t block, uint32_t *dst, uint64_t capacity,
                           uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats);

#endif /* PRF_DOTPAIR_H */
