/*
 * prf_alignpath.h -- the entry points of libprf that say WHERE a tandem repeat differs from its motif: the alignment of
 * prf_align.h with its path, one entry per position, and the counts of the aligned columns.  Part of the C ABI of include/prf.h,
 * which includes this file inside its extern "C" block, directly behind prf_align.h (include prf.h, not this file).  They live in a
 * header of their own so that the lists of entry points of prf.h proper and of the eleven headers before this one stay what they
 * were; these are prf_native.ALIGNPATH_EXPORTS.
 */
#ifndef PRF_ALIGNPATH_H
#define PRF_ALIGNPATH_H
#ifndef PRF_H
#error "include prf.h, which includes prf_alignpath.h"
#endif

/* ---- alignments of the repeats of one range to their motifs, with their paths ----
 * The range, the rows prf_repeat (start, end, k), the motifs, the letters and what matches are those of prf_align.h, and dst
 * receives the same prf_alignment per row as prf_motif_align, bit for bit.
 * THE CELLS: position i (0 <= i < n_r) and column j (0 <= j < k) with D the cells of the position before (all 0 before the first)
 * and T, D' of prf_align.h's recurrence, compared as triples (edits, indels, consumed):
 *   from_ins[i][j] = D[j] + (1, 1, 0) <  D[(j - 1) mod k] + (sub, 0, 1)     strictly: ties go to the diagonal
 *   from_del[i][j] = D'[j] < T[j]                                            strictly; then D'[j] = D'[(j - 1) mod k] + (1, 1, 1)
 * THE PATH of a row: start at i = n_r - 1, j = end_column; while i >= 0:
 *   from_del[i][j]:       a deletion of column j;                                              j <- (j - 1) mod k
 *   else from_ins[i][j]:  path[i] = j | PRF_PATH_INS;                                          i <- i - 1
 *   else:                 path[i] = j | (PRF_PATH_SUB if position i does not match M[j]);      j <- (j - 1) mod k, i <- i - 1
 * Bits 10 .. 13 of an entry are 0.  An insertion's column is the state column: the last motif letter consumed in front of it.
 * Position 0 is never an insertion, the final cell never a deletion, path[0] & PRF_PATH_COLUMN == start_column, and a run of
 * deletions is shorter than k.
 * THE DELETIONS are read from the path alone: they sit directly behind the position in front of them.  With state_i =
 * path[i] & PRF_PATH_COLUMN, the deletions between i and i + 1 are (c - 1 - state_i) mod k if i + 1 is aligned at column c, and
 * (c - state_i) mod k if i + 1 is an insertion with column c; they are the columns behind state_i, in order.
 * The INS entries plus the deletions are `indels`; with the SUB entries, `edits`; the aligned entries plus the deletions,
 * `consumed`.
 * LAYOUT: `path` holds path_capacity entries; row r's n_r entries begin at the sum of end - start of the rows in front of it, in
 * the order of the input rows.
 * COUNTS (NULL: not wanted): six uint32_t per motif letter, at 6 * (offset + j) + c with offset the sum of the k of the rows in
 * front: c = 0 .. 3 the aligned (not INS) positions of column j whose upper-cased letter is A, C, G, T (N and positions with X
 * set count nowhere), c = 4 the deletions of column j, c = 5 the INS entries with column j.  6 * the sum of k are written.
 * LIMITS: PRF_ALIGN_MAX_K, PRF_ALIGN_MAX_LEN, and the sum of n_r <= PRF_ALIGNPATH_MAX_POSITIONS.
 * Refusals: those of prf_align.h in its order, with these additions:
 *   3. ... also PRF_EINVAL for a NULL path;
 *   5. ... then PRF_EUNSUPPORTED for a sum of n_r above PRF_ALIGNPATH_MAX_POSITIONS, then PRF_EINVAL for a sum of n_r above
 *      path_capacity.
 * n_rows == 0 behaves as in prf_align.h.  A refused call writes nothing.
 * TRACE MEMORY: the forward pass leaves 2 bits per cell in device scratch, whose layout is internal (a row of k > 512 and 2^19
 * positions, the limits, needs 128 MiB).  The host deals the rows into batches whose trace fits trace_bytes (the _ex form; 0:
 * PRF_ALIGNPATH_TRACE_BYTES); a row that alone needs more gets a batch of its own.  The results do not depend on trace_bytes.
 * The default of 1 GiB is a guess that nobody has measured.
 * Stats: path = 15, phase1_ms = HIP-event time of the forward kernels, phase2_ms = of the walk and the counts kernels, scan_ms =
 * their sum, positions = the sum of n_r, n_candidates = the sum of n_r k, n_hits = n_rows, n_launches.
 * The one-shot form takes one sequence of ASCII, as prf_motif_align_seq does, with the default trace_bytes. */
#define PRF_ALIGNPATH_MAX_POSITIONS (1ull << 30) /* entries of one call's path                                      */
#define PRF_ALIGNPATH_TRACE_BYTES (1ull << 30)   /* device scratch per batch: an unmeasured guess                   */
#define PRF_PATH_INS 0x8000u                     /* the position is an insertion behind column j                    */
#define PRF_PATH_SUB 0x4000u                     /* the position is aligned to column j and does not match it       */
#define PRF_PATH_COLUMN 0x03FFu                  /* j                                                               */

int prf_motif_align_path(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                         uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, uint16_t *path,
                         uint64_t path_capacity, uint32_t *counts, prf_scan_stats *stats);
int prf_motif_align_path_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                            uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, uint16_t *path,
                            uint64_t path_capacity, uint32_t *counts, prf_scan_stats *stats, uint64_t trace_bytes);
int prf_motif_align_path_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows,
                             uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, uint16_t *path,
                             uint64_t path_capacity, uint32_t *counts, prf_scan_stats *stats);

#endif /* PRF_ALIGNPATH_H */
