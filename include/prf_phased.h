/*
 * prf_phased.h -- the entry points of libprf that say WHAT a GAPPED tandem repeat is: consensus motifs counted over segments
 * with a phase instead of over one (start, end, k).  Part of the C ABI of include/prf.h, which includes this file inside its
 * extern "C" block (include prf.h, not this file).  They live in a header of their own so that the lists of entry points of prf.h
 * proper and of the nine headers before this one stay what they were; these are prf_native.PHASED_EXPORTS.
 */
#ifndef PRF_PHASED_H
#define PRF_PHASED_H
#ifndef PRF_H
#error "include prf.h, which includes prf_phased.h"
#endif

/* ---- consensus motifs over phased segments of one range ----
 * s: positions [begin, end) of one contig of a resident genome, `end` clipped to the contig; n = its length.  Nothing outside
 * the words of the planes that hold a segment's positions is read, so the genome's kmax_hint does not bound k.
 * ROWS: n_rows consensus rows; row r has ks[r] >= 1 columns.
 * SEGMENTS: n_segments of prf_segment (start, end, row, phase), relative to `begin`, with 0 <= start < end <= n, row < n_rows and
 * phase < ks[row].  Position q of a segment lies in column (phase + q - start) mod k of its row.  Segments may come in any order,
 * the rows' segments may interleave, segments may overlap or repeat: every (segment, position) pair counts once.  A segment names
 * a stretch of a repeat: an end behind n is refused, never clipped.
 * count[r][p][b], b = 0 .. 3 for A, C, G, T, is the number of (segment, position) pairs of row r in column p whose upper-cased
 * letter is b.  N and every other letter (X set in the planes) count for nothing; only the planes H, L, X are read.
 * OUTPUT: exactly prf_period_consensus' (prf_consensus.h), in row order: one prf_consensus per row in dst (offset = the sum of the
 * k in front, agree, acgt, k); motifs[offset .. offset + k) are the row's consensus letters, the largest count with ties to the
 * first of A, C, G, T, 'N' for a column without a count; if counts is not NULL, counts[4 (offset + p) + b] = count[r][p][b].
 * A row without segments is all 'N' with agree = acgt = 0.  One segment (start, end, r, 0) per row r gives what
 * prf_period_consensus gives for the rows (start, end, ks[r]).
 * Refusals, in this order; those of 1 .. 8 are judged from the arguments, before the context or the genome is looked at:
 *   1. PRF_EINVAL for begin > end;
 *   2. PRF_EUNSUPPORTED for n_rows above PRF_CONSENSUS_MAX_ROWS, then for n_segments above PRF_PHASED_MAX_SEGMENTS;
 *   3. PRF_EINVAL for NULL ks, dst or motifs with n_rows > 0, then for NULL segments with n_segments > 0;
 *   4. per row, in row order, naming the first offending index: PRF_EINVAL for k == 0;
 *   5. per segment, in segment order, naming the first offending index: PRF_EINVAL for start >= end, for row >= n_rows, for
 *      phase >= ks[row];
 *   6. PRF_EUNSUPPORTED for a row whose columns could hold more than 2^32 - 1 positions (the sum over its segments of
 *      ceil((end - start) / k) >= 2^32), naming the first such row;
 *   7. PRF_EUNSUPPORTED for a sum of k above PRF_CONSENSUS_MAX_LETTERS;
 *   8. PRF_EINVAL for a sum of k above letters_capacity;
 *   9. once the length of the sequence is known (the one-shot form: still before the context; on a genome: behind the NULL
 *      context, the contig and the genome of another context): PRF_EINVAL for a segment with end > n, naming the first such
 *      index; PRF_EUNSUPPORTED for a range of 2^40 positions or more;
 *  10. the refusals of the context and the genome that the list products have (NULL context, a contig the genome does not
 *      hold, a genome of another context, pipelined scans in flight);
 *  11. PRF_EUNSUPPORTED for segments that cut into more than PRF_CONSENSUS_MAX_ITEMS work items: ask for a larger slice.
 * n_rows == 0 (behind refusals 1 and 2) returns PRF_OK, writes nothing -- not the stats either -- and launches nothing; the
 * context is not looked at.  n_segments == 0 with rows is legal: every row is all 'N'.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the matrix and the list products.
 * Stats: path = 13, scan_ms = HIP-event time of all launches (phase1_ms: the count kernels', phase2_ms: the finish kernel's),
 * positions = the sum of end - start over the segments, n_candidates = the work items, n_hits = n_rows, n_launches.
 * The _ex form cuts segments into work items of at most slice_positions positions (0: PRF_CONSENSUS_SLICE), for the tests; the
 * results do not depend on it.
 * The one-shot form takes one sequence of ASCII (prf_genome_load + the call + prf_genome_free; PRF_ESYMBOL for a byte that is not
 * a letter, found on the host before the context is looked at). */
typedef struct prf_segment {
    uint64_t start;    /* first position, relative to begin                         */
    uint64_t end;      /* one past the last position                                */
    uint32_t row;      /* the consensus row the positions count for                 */
    uint32_t phase;    /* the column of position start; below the row's k           */
} prf_segment;

#define PRF_PHASED_MAX_SEGMENTS (1ull << 24)   /* segments per call; rows, letters and items: the limits of prf_consensus.h */

int prf_phased_consensus(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const uint32_t *ks,
                         uint64_t n_rows, const prf_segment *segments, uint64_t n_segments, prf_consensus *dst, char *motifs,
                         uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats);
int prf_phased_consensus_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const uint32_t *ks,
                            uint64_t n_rows, const prf_segment *segments, uint64_t n_segments, prf_consensus *dst, char *motifs,
                            uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats, uint64_t slice_positions);
int prf_phased_consensus_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, const uint32_t *ks, uint64_t n_rows,
                             const prf_segment *segments, uint64_t n_segments, prf_consensus *dst, char *motifs,
                             uint64_t letters_capacity, uint32_t *counts, prf_scan_stats *stats);

#endif /* PRF_PHASED_H */
