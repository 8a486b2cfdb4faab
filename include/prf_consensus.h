/*
 * prf_consensus.h -- the entry points of libprf that say WHAT a tandem repeat is: the consensus motif of each of a list of
 * repeats (start, end, k) of a range, column by column.  Part of the C ABI of include/prf.h, which includes this file inside its
 * extern "C" block (include prf.h, not this file).  They live in a header of their own so that the lists of entry points of prf.h
 * proper and of the eight headers before this one stay what they were; these are prf_native.CONSENSUS_EXPORTS.
 */
#ifndef PRF_CONSENSUS_H
#define PRF_CONSENSUS_H
#ifndef PRF_H
#error "include prf.h, which includes prf_consensus.h"
#endif

/* ---- consensus motifs of the repeats of one range ----
 * s: positions [begin, end) of one contig of a resident genome, `end` clipped to the contig; n = its length.  Nothing outside
 * the words of the planes that hold a row's positions is read, so the genome's kmax_hint does not bound k.
 * INPUT: n_rows repeats (start, end, k), relative to `begin`, with 0 <= start < end <= n and k >= 1.  Rows may overlap, repeat
 * or nest; end - start < k is allowed.  A row names a repeat: an end behind n is refused, never clipped.
 * COLUMN p (0 <= p < k) of a row holds the positions start + p + j k < end, j = 0, 1, ...; a column without a position is empty.
 * count[p][b], b = 0 .. 3 for A, C, G, T, is the number of those positions whose upper-cased letter is b.  N and every other
 * letter (X set in the planes) count for nothing; only the planes H, L, X are read, so genomes of three and of eight planes take
 * the same code.
 * consensus[p] is the letter with the largest count, ties to the first in the order A, C, G, T; 'N' if all four counts are 0.
 * agree = sum over p of max_b count[p][b]: the positions that carry their column's consensus.  acgt = sum over p, b of count[p][b].
 * OUTPUT, in the order of the input rows (nothing is sorted): one prf_consensus per row in dst; offset is the sum of the k of
 * the rows in front of it; motifs[offset .. offset + k) are the row's consensus letters (ASCII, no terminator); if counts is not
 * NULL, counts[4 (offset + p) + b] = count[p][b].  motifs and counts have room for letters_capacity letters (and four counts
 * per letter).
 * Refusals, in this order; those of 1 .. 6 are judged from the arguments, before the context or the genome is looked at:
 *   1. PRF_EINVAL for begin > end;
 *   2. PRF_EUNSUPPORTED for n_rows above PRF_CONSENSUS_MAX_ROWS;
 *   3. PRF_EINVAL for NULL rows, dst or motifs with n_rows > 0;
 *   4. per row, in row order, naming the first offending index: PRF_EINVAL for k == 0, for start >= end, for reserved != 0;
 *      PRF_EUNSUPPORTED for a row with more than 2^32 - 1 positions in a column (ceil((end - start) / k) >= 2^32);
 *   5. PRF_EUNSUPPORTED for a sum of k above PRF_CONSENSUS_MAX_LETTERS;
 *   6. PRF_EINVAL for a sum of k above letters_capacity;
 *   7. once the length of the sequence is known (the one-shot form: still before the context; on a genome: behind the NULL
 *      context, the contig and the genome of another context, as the siblings place what needs the length): PRF_EINVAL for a
 *      row with end > n, naming the first such index; PRF_EUNSUPPORTED for a range of 2^40 positions or more;
 *   8. the refusals of the context and the genome that the list products have (NULL context, a contig the genome does not
 *      hold, a genome of another context, pipelined scans in flight);
 *   9. PRF_EUNSUPPORTED for rows that cut into more than PRF_CONSENSUS_MAX_ITEMS work items: ask for a larger slice.
 * n_rows == 0 (behind refusals 1 and 2) returns PRF_OK, writes nothing -- not the stats either -- and launches nothing; the
 * context is not looked at.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the matrix and the list products.
 * Stats: path = 12, scan_ms = HIP-event time of all launches (phase1_ms: the count kernels', phase2_ms: the finish kernel's),
 * positions = the sum of end - start, n_candidates = the work items, n_hits = n_rows, n_launches.
 * The _ex form cuts rows into work items of at most slice_positions positions (0: PRF_CONSENSUS_SLICE), for the tests; the
 * results do not depend on it.
 * The one-shot form takes one sequence of ASCII (prf_genome_load + the call + prf_genome_free; PRF_ESYMBOL for a byte that is not
 * a letter, found on the host before the context is looked at). */
typedef struct prf_repeat {
    uint64_t start;    /* first position, relative to begin                         */
    uint64_t end;      /* one past the last position                                */
    uint32_t k;        /* the period: the number of columns                         */
    uint32_t reserved; /* 0                                                         */
} prf_repeat;

typedef struct prf_consensus {
    uint64_t offset;   /* of the row's letters in motifs: the sum of the k in front */
    uint64_t agree;    /* positions that carry their column's consensus             */
    uint64_t acgt;     /* positions that are A, C, G or T                           */
    uint32_t k;        /* the row's k: letters at motifs + offset                   */
    uint32_t reserved; /* 0                                                         */
} prf_consensus;

#define PRF_CONSENSUS_MAX_ROWS (1ull << 24)    /* rows per call                                                             */
#define PRF_CONSENSUS_MAX_LETTERS (1ull << 26) /* the sum of k per call                                                     */
#define PRF_CONSENSUS_MAX_ITEMS (1ull << 26)   /* work items per call                                                       */
#define PRF_CONSENSUS_SLICE 4096u              /* positions per work item by default: a guess that nobody has measured yet  */

int prf_period_consensus(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                         uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                         prf_scan_stats *stats);
int prf_period_consensus_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                            uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                            prf_scan_stats *stats, uint64_t slice_positions);
int prf_period_consensus_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows,
                             uint64_t n_rows, prf_consensus *dst, char *motifs, uint64_t letters_capacity, uint32_t *counts,
                             prf_scan_stats *stats);

#endif /* PRF_CONSENSUS_H */
