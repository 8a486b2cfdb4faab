/*
 * prf_alignlocal.h -- the entry points of libprf that say WHERE a tandem repeat begins and ends and WHAT IT SCORES: the best local
 * alignment of a window around each of a list of repeats against the endless repetition of its motif, under weights for match,
 * mismatch and indel (the Smith-Waterman form of prf_align.h's wraparound dynamic programming).  Part of the C ABI of
 * include/prf.h, which includes this file inside its extern "C" block, directly behind prf_alignpath.h (include prf.h, not this
 * file).  They live in a header of their own so that the lists of entry points of prf.h proper and of the twelve headers before
 * this one stay what they were; these are prf_native.ALIGNLOCAL_EXPORTS.
 */
#ifndef PRF_ALIGNLOCAL_H
#define PRF_ALIGNLOCAL_H
#ifndef PRF_H
#error "include prf.h, which includes prf_alignlocal.h"
#endif

/* ---- local alignments of windows of one range to motifs ----
 * The range, the rows prf_repeat (start, end, k), the motifs' layout, the letters and what matches are those of prf_align.h: N, a
 * position with X set and a motif N match nothing.  A row's [start, end) is the WINDOW to search; padding a found repeat by a
 * flank is the caller's job.  The limits are PRF_ALIGN_MAX_K and PRF_ALIGN_MAX_LEN.
 * WEIGHTS: match, mismatch, indel, each 1 .. PRF_ALIGNLOCAL_MAX_WEIGHT, for the whole call.  The score of an alignment is
 *   match * matches - mismatch * substitutions - indel * (insertions + deletions).
 * THE RESULT of a row: over every tuple (p, q, a, C) of a first position p, a last position q >= p, a start column a and a number
 * C >= 1 of motif letters, scored by the best global alignment of positions p .. q with the C letters M[(a + t) mod k],
 * t = 0 .. C - 1, let S be the greatest score.  S <= 0 (no position matches any letter): the row is all zeros.  Otherwise, among
 * the tuples that reach S: the least q, then the least end column (a + C - 1) mod k, then the greatest p, then the greatest a -- of
 * equal scores, the alignment that ends first and begins last.
 * first and end are relative to the row's start (below 2^19), so that (start + first, start + end, k) with the same motif is a
 * row for prf_motif_align and prf_motif_align_path: the refined interval's edits and copies.  No rotation of the motif is needed,
 * prf_align.h being free at both ends of the motif.
 * OUTPUT, in the order of the input rows (nothing is sorted): one prf_local_alignment per row in dst.
 * Refusals: those of prf_align.h, in its order, with one addition directly behind the range refusal (1) and in front of the row
 * limit (2): PRF_EINVAL for a weight of 0, then PRF_EUNSUPPORTED for a weight above PRF_ALIGNLOCAL_MAX_WEIGHT, each naming the
 * first such weight of match, mismatch, indel.
 * n_rows == 0 (behind these and the row limit) returns PRF_OK, writes nothing -- not the stats either -- and launches nothing;
 * the context is not looked at.  A refused call writes nothing.
 * A selection of parts, a row sink and the rows of the last scan are left alone.
 * Stats: path = 16, scan_ms = phase1_ms = HIP-event time of the kernels, positions = the sum of end - start, n_candidates = the
 * sum of (end - start) k, n_hits = n_rows, n_launches.
 * There is no _ex form: the kernel has no knob.  The one-shot form takes one sequence of ASCII, as prf_motif_align_seq does. */
typedef struct prf_local_alignment {
    uint32_t score;        /* of the best local alignment; 0: nothing matches, the row is all zeros */
    uint32_t first;        /* its first position, relative to the row's start                       */
    uint32_t end;          /* one behind its last position, relative to the row's start             */
    uint32_t start_column; /* the column of the first motif letter it runs over                     */
    uint32_t end_column;   /* the column of the last                                                */
    uint32_t reserved;     /* 0                                                                     */
} prf_local_alignment;

#define PRF_ALIGNLOCAL_MAX_WEIGHT 16u  /* each of match, mismatch, indel: the score of 2^19 positions packs into 25 bits */

int prf_motif_align_local(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, const prf_repeat *rows,
                          uint64_t n_rows, const char *motifs, uint64_t letters_length, uint32_t match, uint32_t mismatch,
                          uint32_t indel, prf_local_alignment *dst, prf_scan_stats *stats);
int prf_motif_align_local_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, const prf_repeat *rows,
                              uint64_t n_rows, const char *motifs, uint64_t letters_length, uint32_t match, uint32_t mismatch,
                              uint32_t indel, prf_local_alignment *dst, prf_scan_stats *stats);

#endif /* PRF_ALIGNLOCAL_H */
