/*
 * prf_periodlink.h -- the entry points of libprf that list the INDEL JUNCTIONS between the chains of prf_periodchain.h: "chain X
 * ends here on period line k_X, chain Y starts there on line k_Y": the step from diverged to GAPPED tandem repeats.  Part of the
 * C ABI of include/prf.h, which includes this file inside its extern "C" block (include prf.h, not this file).  They live in a
 * header of their own so that the lists of entry points of prf.h proper and of the seven product headers before this one stay
 * what they were; these are prf_native.PERIODLINK_EXPORTS.
 */
#ifndef PRF_PERIODLINK_H
#define PRF_PERIODLINK_H
#ifndef PRF_H
#error "include prf.h, which includes prf_periodlink.h"
#endif

/* ---- links between chains on neighbouring period lines of one range ----
 * The range [begin, end) of one contig, its length n, LINE k >= 1 with the cells t = 0 .. n - k - 1, raw_k(t) under either
 * n_matches, the SEEDS and the CHAINS at (min_seed, max_gap) are exactly those of prf_periodchain.h, with no min_len filter.
 * Coordinates.  A cell of line k is (i, c) = (t, t + k): the line's offset is delta = k, and the words of prf_dotlink.h apply
 * unchanged.  For two chains X (line k_X, last cell t_e) and Y (line k_Y, first cell t_s): the shift s = k_Y - k_X,
 * gi = t_s - t_e - 1, gc = gi + s and g = min(gi, gc).  (X, Y) is a CANDIDATE iff 1 <= |s| <= max_shift and -ov <= g <= max_gap,
 * where ov = min(min_seed - 1, PRF_DOTLINK_OVERLAP).  The OVERLAP o = max(0, -g), the GAP m = max(0, g), the key
 * key(X, Y) = (m + |s|, |s|, o, s < 0) compared lexicographically, pred(Y) = the candidate X with the smallest key, succ(X) = the
 * candidate Y with the smallest key, and X -> Y is a LINK iff pred(Y) = X and succ(X) = Y: all as in prf_dotlink.h.
 * The lines that take part are ALL lines k' with 1 <= k' <= n - 1 of the range, whatever kmin and kmax are.  Line 0 (every cell
 * matches itself) and the mirror lines k' < 0 never take part.  A line's edges behave as mismatches.
 * Facts the code and the tests rely on, those of prf_dotlink.h:
 *  - On one line at most one chain ends, and at most one begins, inside a stretch of max_gap + ov + 1 cells: two tails or two
 *    heads of a line lie at least max_gap + min_seed + 1 cells apart.  So a line holds at most one candidate, s differs between
 *    the candidates of a chain, and the smallest key is unique.
 *  - Among the seeds that end in such a stretch only the last can be a chain's end; among those that start in it only the first
 *    can be a chain's start.
 *  - Every chain has at most one link in and at most one link out.
 *  - t_s grows strictly along links (t_s(Y) >= t_e(X) + 1 - ov > t_s(X), because X holds a seed of min_seed > ov cells), so the
 *    links form paths.
 *  - Nothing depends on any order of evaluation.
 *  - Everything a link depends on lies within max_gap + max_shift + 2 min_seed cells of the junction.
 * Hence one base inserted into a repeat of period k >= min_seed gives two links: from line k out to the detour chain on line
 * k + 1 (shift +1) and back (shift -1).
 * A call reports the links whose Y has pos0 <= start < pos1 (clipped to n) and kmin <= k_Y <= kmax, sorted ascending by
 * (start, k).  Links are judged on the whole band, never clipped by the window or the range of k: the lists of any partition in
 * positions and / or in k add up to the whole list, each link once.  X may lie on a line outside [kmin, kmax].
 * *n_links is always the number of links found.  dst is written -- all *n_links rows, sorted -- only if *n_links <= capacity;
 * otherwise dst is left untouched and the call still returns PRF_OK: compare and call again.  dst == NULL with capacity == 0
 * counts only.
 * Refusals, judged before the context or the genome is looked at, in this order: PRF_EINVAL for begin > end, pos0 > pos1,
 * kmin == 0, kmin > kmax, n_matches > 1, min_seed == 0; PRF_EUNSUPPORTED for max_gap above PRF_DOTCHAIN_MAX_GAP; PRF_EINVAL for
 * max_shift == 0; PRF_EUNSUPPORTED for max_shift above PRF_DOTLINK_MAX_SHIFT and for a capacity above PRF_PCHAIN_MAX_ROWS;
 * PRF_EINVAL for a NULL n_links, or a NULL dst with a capacity other than 0.  Everything behind these is prf_periodchain.h's: the
 * window above PRF_DOT_MAX_CELLS, the contig, the genome's context, and, loudly and never a wrong list, PRF_EUNSUPPORTED if more
 * than PRF_PCHAIN_MAX_ROWS chains start in the window or if the runs and chains still going after PRF_DOTCHAIN_FOLLOW cells
 * outnumber the list the call keeps them in.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the other matrix products.
 * Stats: path = 11, scan_ms = HIP-event time of all launches (phase1_ms: the find and the long kernel's of prf_periodchain.h,
 * phase2_ms: the join kernel's), positions = n, n_candidates = the chain heads of the window, n_hits = *n_links, n_launches.
 * The call keeps room for 2^20 heads on the device; if more chains start in the window the find and the long kernel run a second
 * time in full with room for the exact number, and BOTH passes are counted in phase1_ms, scan_ms and n_launches: phase1_ms is then
 * about twice the time of prf_period_chains over the same window.
 * The _ex form cuts the window's positions into launches of the find kernel of at most launch_cells cells (0: the default), for
 * the tests.  The one-shot form takes one sequence of ASCII, as prf_period_chains_seq does. */
typedef struct prf_plink {
    uint64_t start;    /* Y's first cell t_s: (start, k) is the key of Y's row in the list of chains */
    uint64_t from_end; /* X's last cell t_e                                                          */
    uint32_t k;        /* k_Y                                                                        */
    int32_t shift;     /* s = k_Y - k_X, so k_X = k - shift                                          */
    uint32_t gap;      /* m                                                                          */
    uint32_t overlap;  /* o                                                                          */
} prf_plink;           /* 32 bytes */

int prf_period_links(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                     uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                     prf_plink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats);
int prf_period_links_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0,
                        uint64_t pos1, uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap,
                        uint32_t max_shift, prf_plink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats,
                        uint64_t launch_cells);
int prf_period_links_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                         uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint32_t max_shift,
                         prf_plink *dst, uint64_t capacity, uint64_t *n_links, prf_scan_stats *stats);

#endif /* PRF_PERIODLINK_H */
