/*
 * prf_dotplot.h -- the dot-plot entry points of libprf: part of the C ABI of include/prf.h, which includes this file inside
 * its extern "C" block (include prf.h, not this file).  They live in a header of their own so that the list of entry points
 * of prf.h proper -- prf_native.EXPORTS -- stays what it was; these are prf_native.DOTPLOT_EXPORTS.
 */
#ifndef PRF_DOTPLOT_H
#define PRF_DOTPLOT_H
#ifndef PRF_H
#error "include prf.h, which includes prf_dotplot.h"
#endif

/* ---- exact dot plot: the reference's generate_matrix + filter_out_noise (plot_dot_plot.py) on a resident genome ----
 * s = positions [begin, end) of one contig, upper-cased (end beyond the contig is clipped to its length), n = len(s).
 * raw(i, j) = (s[i] == s[j]) by plain comparison of symbols: N == N IS a match, any other letter matches itself and nothing
 * else.  With t = min_diagonal_run:
 *     kept(i, j)  <=>  raw(i, j) and (Lmain(i, j) + 1 >= t  or  Lanti(i, j) + 1 >= t)
 * Lmain / Lanti: the length of the maximal run of raw cells through (i, j) along (+1, +1) / (+1, -1), in the unfiltered n x n
 * matrix, clipped by 0 .. n-1 and by nothing else (not by the window): what the reference's in-place filter leaves.  t <= 2
 * filters nothing.  Rows and columns outside [0, n) are zero; nothing at or behind `end` is compared or read.
 * A call computes the window rows [row0, row1) x columns [col0, col1) of that matrix (indices relative to `begin`, both ends
 * clipped to n); its cells equal the same cells of the whole matrix.
 * prf_dotplot_bits: dst (host memory) receives (row1 - row0) rows of *words_per_row = ceil((col1 - col0) / 64) words; bit j of
 * word w of row r = kept(row0 + r, col0 + 64 w + j); tail bits behind col1 are zero.
 * prf_dotplot_counts: dst receives *n_block_rows x *n_block_cols sums; entry (R, C) = the kept cells of window rows
 * [row0 + R block, row0 + (R + 1) block) x window columns [col0 + C block, col0 + (C + 1) block), each clipped to the window.
 * block: a multiple of 64, 64 <= block <= 32768 (a count fits 32 bits), PRF_EINVAL otherwise.
 * Refusals, judged before the context or the genome is looked at: PRF_EINVAL for a NULL dst or size pointer, row0 > row1,
 * col0 > col1, begin > end; PRF_EUNSUPPORTED for min_diagonal_run > 64.  Once the length is known (the one-shot forms: still
 * before the context): PRF_EINVAL if dst holds fewer than the output's entries (capacity), PRF_EUNSUPPORTED for an output above
 * PRF_PERIOD_BITS_MAX_WORDS entries or a window above PRF_DOT_MAX_CELLS cells.
 * Both ignore a selection of parts (prf_genome_select) and leave a row sink and the rows of the last scan alone.
 * Stats: path = 5, scan_ms = HIP-event time of the launches, positions = end - begin, n_hits = 0, n_launches.
 * The host cuts a window into launches of at most PRF_DOT_LAUNCH_CELLS cells (whole tiles of rows), so that no single kernel
 * holds a shared device for long.  The filter costs (min_diagonal_run - 1)^2 steps per cell above min_diagonal_run = 3, so with
 * m = min_diagonal_run - 1 > 2 the default is PRF_DOT_LAUNCH_CELLS / ceil(m^2 / 4) cells: a launch stays a few milliseconds
 * long at every threshold (measured: DESIGN 11.5).  The _ex forms take the figure as an argument (0: that default; any other
 * value is used as it is) so that tests can place a cut inside a small window.
 * The one-shot forms take one sequence of ASCII (prf_genome_load + the call + prf_genome_free; PRF_ESYMBOL for a byte that is
 * not a letter, found on the host before the context is looked at).
 * prf_dotplot_shape: the launch shape for a threshold (the same for both plane sets) -- rows per workgroup tile, 64-column words per
 * workgroup span, halo rows on either side (host-only, no GPU): tile and span boundaries lie at multiples of these from
 * (row0, col0). */
#define PRF_DOT_LAUNCH_CELLS (1ull << 36)
#define PRF_DOT_MAX_CELLS (1ull << 42)
#define PRF_DOT_MAX_RUN 64u
int prf_dotplot_bits(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0,
                     uint64_t row1, uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t *dst,
                     uint64_t capacity_words, uint64_t *words_per_row, prf_scan_stats *stats);
int prf_dotplot_counts(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0,
                       uint64_t row1, uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t block, uint32_t *dst,
                       uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats);
int prf_dotplot_bits_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0,
                        uint64_t row1, uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t *dst,
                        uint64_t capacity_words, uint64_t *words_per_row, prf_scan_stats *stats, uint64_t launch_cells);
int prf_dotplot_counts_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0,
                          uint64_t row1, uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t block,
                          uint32_t *dst, uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols,
                          prf_scan_stats *stats, uint64_t launch_cells);
int prf_dotplot_bits_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                         uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t *dst, uint64_t capacity_words,
                         uint64_t *words_per_row, prf_scan_stats *stats);
int prf_dotplot_counts_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                           uint64_t col0, uint64_t col1, uint32_t min_diagonal_run, uint64_t block, uint32_t *dst,
                           uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats);
int prf_dotplot_shape(uint32_t min_diagonal_run, uint32_t *tile_rows, uint32_t *span_words, uint32_t *halo_rows);

#endif /* PRF_DOTPLOT_H */
