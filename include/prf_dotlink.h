/*
 * prf_dotlink.h -- the entry points of libprf that list the INDEL JUNCTIONS between the chains of prf_dotchain.h: "chain X ends
 * here, chain Y starts there, on another diagonal".  Part of the C ABI of include/prf.h, which includes this file inside its
 * extern "C" block (include prf.h, not this file).  They live in a header of their own so that the lists of entry points of
 * prf.h proper and of the five older product headers stay what they were; these are prf_native.DOTLINK_EXPORTS.
 */
#ifndef PRF_DOTLINK_H
#define PRF_DOTLINK_H
#ifndef PRF_H
#error "include prf.h, which includes prf_dotlink.h"
#endif

/* ---- links between chains on neighbouring lines of the dot plot of two ranges ----
 * A, B, na, nb, strand, raw(i, j), the clipping of each end to its contig, the window, `directions`, min_seed and max_gap are
 * exactly those of prf_dotchain.h.  The CHAINS are the chains of the whole rectangle at (min_seed, max_gap), with no min_len
 * filter.
 * Coordinates.  Per direction a cell is (i, c), with c = j on a main line and c = nb - 1 - j on an anti line: both grow along a
 * line.  A line's offset is delta = c - i.  A chain has a first cell (i_s, c_s) and a last cell (i_e, c_e) =
 * (i_s + len - 1, c_s + len - 1).
 * Candidate pair.  For two chains X and Y of the same direction: the shift s = delta_Y - delta_X, gi = i_s(Y) - i_e(X) - 1,
 * gc = gi + s (= c_s(Y) - c_e(X) - 1) and g = min(gi, gc).  (X, Y) is a CANDIDATE iff 1 <= |s| <= max_shift and
 * -ov <= g <= max_gap, where ov = min(min_seed - 1, PRF_DOTLINK_OVERLAP).
 * Overlap and gap.  The OVERLAP o = max(0, -g) is the number of cells of Y's first seed that lie in front of X's end in one
 * coordinate (an exact run overshoots a breakpoint by chance one time in four per base).  Because o < min_seed <= the length of
 * Y's first seed, those o cells are all raw: trimming them is exact.  The GAP m = max(0, g) is the number of cells between X and
 * the trimmed Y in the coordinate where they are closer.
 * Key.  key(X, Y) = (m + |s|, |s|, o, s < 0), compared lexicographically.  pred(Y) is the candidate X with the smallest key,
 * succ(X) the candidate Y with the smallest key.  X -> Y is a LINK iff pred(Y) = X and succ(X) = Y.
 * Facts the code and the tests rely on:
 *  - On one line at most one chain ends, and at most one begins, inside a stretch of max_gap + ov + 1 cells: two tails or two
 *    heads of a line lie at least max_gap + min_seed + 1 cells apart.  So a line holds at most one candidate, s differs between
 *    the candidates of a chain, and the smallest key is unique.
 *  - Among the seeds that end in such a stretch only the last can be a chain's end; among those that start in it only the first
 *    can be a chain's start.
 *  - Every chain has at most one link in and at most one link out.
 *  - i_s grows strictly along links (i_s(Y) >= i_e(X) + 1 - ov > i_s(X), because X holds a seed of min_seed > ov cells), so
 *    the links form paths.
 *  - Nothing depends on any order of evaluation.
 *  - Everything a link depends on lies within max_gap + max_shift + 2 min_seed cells of the junction.
 * A call reports the links whose (row, col) -- Y's first cell -- lies in the window rows [row0, row1) x columns [col0, col1) and
 * whose direction is in `directions`, sorted ascending by (row, col, dir).  Links are judged in the whole rectangle, never clipped
 * by the window: the lists of a partition of the rectangle into windows add up to the whole list, each link once.
 * *n_links is always the number of links found.  dst is written -- all *n_links rows, sorted -- only if *n_links <= capacity;
 * otherwise dst is left untouched and the call still returns PRF_OK: compare and call again.  dst == NULL with capacity == 0
 * counts only.
 * Refusals, judged before the context or the genome is looked at, in this order: PRF_EINVAL for a_begin > a_end, b_begin > b_end,
 * row0 > row1, col0 > col1, strand > 1, directions 0 or above 3, min_seed == 0; PRF_EUNSUPPORTED for max_gap above
 * PRF_DOTCHAIN_MAX_GAP; PRF_EINVAL for max_shift == 0; PRF_EUNSUPPORTED for max_shift above PRF_DOTLINK_MAX_SHIFT and for a
 * capacity above PRF_DOTCHAIN_MAX_ROWS; PRF_EINVAL for a NULL n_links, or a NULL dst with a capacity other than 0.  Everything
 * behind these is prf_dotchain.h's: the window above PRF_DOT_MAX_CELLS, the contigs, the genome's context, and, loudly and never
 * a wrong list, PRF_EUNSUPPORTED if more than PRF_DOTCHAIN_MAX_ROWS seeds start in the window or if the runs still going after
 * PRF_DOTRUN_FOLLOW cells outnumber the list the call keeps them in.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the other matrix products.
 * Stats: path = 9, scan_ms = HIP-event time of all launches (phase1_ms: the seed kernels', phase2_ms: the heads and the join
 * kernel's), positions = na + nb, n_candidates = the chain heads of the window, n_hits = *n_links, n_launches.
 * The _ex form cuts the window's rows into launches of the seed kernel of at most launch_cells cells (0: the default), for the
 * tests.  The one-shot form takes two sequences of ASCII, as prf_dotpair_chains_seq does. */
typedef struct prf_dotlink {
    uint64_t row, col;           /* Y's first cell (the key of Y's row in the chain list) */
    uint64_t from_row, from_col; /* X's last cell                                         */
    uint32_t dir;                /* 1 main, 2 anti                                        */
    int32_t shift;               /* s = delta_Y - delta_X                                 */
    uint32_t gap, overlap;       /* m and o                                               */
} prf_dotlink;                   /* 48 bytes, columns as j, not c */

#define PRF_DOTLINK_MAX_SHIFT 32u /* lines on either side of a chain's own that a junction may reach: one lane of a wave each */
#define PRF_DOTLINK_OVERLAP 16u   /* cells of a chain's first seed that may lie in front of its predecessor's end            */

int prf_dotpair_links(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                      uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                      uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift, prf_dotlink *dst,
                      uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats);
int prf_dotpair_links_ex(prf_ctx *ctx, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                         uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                         uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                         prf_dotlink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats, uint64_t launch_cells);
int prf_dotpair_links_seq(prf_ctx *ctx, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                          uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0,
                          uint64_t col1, uint32_t directions, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                          prf_dotlink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats);

#endif /* PRF_DOTLINK_H */
