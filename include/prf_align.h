/*
 * prf_align.h -- the entry points of libprf that say HOW FAR a tandem repeat is from its motif: the alignment of each of a list
 * of repeats (start, end, k) of a range against the endless repetition of a motif of k letters, free at both ends of the motif
 * (wraparound dynamic programming, unit costs).  Part of the C ABI of include/prf.h, which includes this file inside its
 * extern "C" block (include prf.h, not this file).  They live in a header of their own so that the lists of entry points of prf.h
 * proper and of the ten headers before this one stay what they were; these are prf_native.ALIGN_EXPORTS.
 */
#ifndef PRF_ALIGN_H
#define PRF_ALIGN_H
#ifndef PRF_H
#error "include prf.h, which includes prf_align.h"
#endif

/* ---- alignments of the repeats of one range to their motifs ----
 * s, begin, end, n and the rows prf_repeat (start, end, k) are those of prf_consensus.h: positions [begin, end) of one contig of
 * a resident genome, `end` clipped to the contig, n its length; rows relative to `begin` with 0 <= start < end <= n and k >= 1;
 * rows may overlap, repeat or nest.  Only the planes H, L, X are read, and only the words that hold a row's positions.
 * MOTIFS: `motifs` holds the sum of k ASCII letters; row r's motif M is at the sum of the k of the rows in front of it -- the
 * layout prf_period_consensus and prf_phased_consensus write, so their output is this call's input.  letters_length is the length
 * of `motifs`.  Letters: A C G T N in either case.
 * MATCH: a position matches a motif letter iff both are the same one of A, C, G, T after upper-casing.  N, a position with X set
 * in the planes and a motif N match nothing; N does not match N.
 * THE ALIGNMENT of a row with S = its n_r = end - start positions: over every start column a (0 <= a < k), every C >= 0 and
 * every alignment of S with the C letters M[(a + t) mod k], t = 0 .. C - 1, the smallest triple, in lexicographic order,
 *   (edits, indels, consumed) = (substitutions + insertions + deletions, insertions + deletions, C)
 * where an insertion is a position against nothing and a deletion a motif letter against nothing.  end_column is the least
 * (a + C - 1) mod k of the alignments that reach that triple, start_column = (end_column + 1 - consumed) mod k.  consumed >= 1:
 * all substitutions cost (n_r, 0, n_r), all insertions (n_r, n_r, 0), which is larger.
 * From a row the caller derives: substitutions = edits - indels; insertions = (indels + n_r - consumed) / 2; deletions =
 * (indels - n_r + consumed) / 2; matches = n_r - substitutions - insertions; aligned identity = matches / (n_r + deletions);
 * aligned copies = consumed / k.
 * OUTPUT, in the order of the input rows (nothing is sorted): one prf_alignment per row in dst.
 * Refusals, in this order; those of 1 .. 6 are judged from the arguments, before the context or the genome is looked at:
 *   1. PRF_EINVAL for begin > end;
 *   2. PRF_EUNSUPPORTED for n_rows above PRF_CONSENSUS_MAX_ROWS;
 *   3. PRF_EINVAL for NULL rows, motifs or dst with n_rows > 0;
 *   4. per row, in row order, naming the first offending index: PRF_EINVAL for k == 0, for start >= end, for reserved != 0;
 *      PRF_EUNSUPPORTED for k above PRF_ALIGN_MAX_K, then for end - start above PRF_ALIGN_MAX_LEN;
 *   5. PRF_EUNSUPPORTED for a sum of k above PRF_CONSENSUS_MAX_LETTERS; PRF_EINVAL for a sum of k above letters_length;
 *   6. PRF_EINVAL for a motif letter that is not one of A C G T N a c g t n, naming the first such row and column;
 *   7. once the length of the sequence is known (the one-shot form: still before the context; on a genome: behind the NULL
 *      context, the contig and the genome of another context): PRF_EINVAL for a row with end > n, naming the first such index;
 *      PRF_EUNSUPPORTED for a range of 2^40 positions or more;
 *   8. the refusals of the context and the genome that the list products have (NULL context, a contig the genome does not
 *      hold, a genome of another context, pipelined scans in flight).
 * n_rows == 0 (behind refusals 1 and 2) returns PRF_OK, writes nothing -- not the stats either -- and launches nothing; the
 * context is not looked at.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the matrix and the list products.
 * Stats: path = 14, scan_ms = phase1_ms = HIP-event time of the kernels, positions = the sum of n_r, n_candidates = the sum of
 * n_r k (the cells of the dynamic programming), n_hits = n_rows, n_launches.
 * There is no _ex form: the kernel has no knob that a test would have to turn.
 * The one-shot form takes one sequence of ASCII (prf_genome_load + the call + prf_genome_free; PRF_ESYMBOL for a byte that is not
 * a letter, found on the host before the context is looked at). */
typedef struct prf_alignment {
    uint32_t edits;        /* substitutions + insertions + deletions                 */
    uint32_t indels;       /* insertions + deletions                                 */
    uint32_t consumed;     /* motif letters the alignment runs over                  */
    uint32_t start_column; /* the column of the first of them                        */
    uint32_t end_column;   /* the column of the last of them                         */
    uint32_t reserved;     /* 0                                                      */
} prf_alignment;

#define PRF_ALIGN_MAX_K 1024u          /* columns per row: sixteen per lane of a wave                               */
#define PRF_ALIGN_MAX_LEN (1ull << 19) /* positions per row: the three counts of a cell pack into 64 bits           */

int prf_motif_align(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                    uint64_t n_rows, const char *motifs, uint64_t letters_length, prf_alignment *dst, prf_scan_stats *stats);
int prf_motif_align_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows, uint64_t n_rows,
                        const char *motifs, uint64_t letters_length, prf_alignment *dst, prf_scan_stats *stats);

#endif /* PRF_ALIGN_H */
