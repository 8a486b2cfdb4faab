/*
 * prf_periodchain.h -- the entry points of libprf that list the DIVERGED TANDEM REPEATS of a range: the exact runs of the period
 * lines k = kmin .. kmax of the periodicity matrix, chained across short stretches of mismatches.  Part of the C ABI of
 * include/prf.h, which includes this file inside its extern "C" block (include prf.h, not this file).  They live in a header of
 * their own so that the lists of entry points of prf.h proper and of the six headers before this one stay what they were; these
 * are prf_native.PERIODCHAIN_EXPORTS.
 */
#ifndef PRF_PERIODCHAIN_H
#define PRF_PERIODCHAIN_H
#ifndef PRF_H
#error "include prf.h, which includes prf_periodchain.h"
#endif

/* ---- chains of exact runs on the period lines of one range ----
 * s: positions [begin, end) of one contig of a resident genome, `end` clipped to the contig; n = its length.  Nothing at or
 * behind `end` is compared or read, so the genome's kmax_hint does not bound k.
 * For k >= 1, LINE k has the cells t = 0 .. n - k - 1; a line with k >= n is empty, which is no error.  raw_k(t):
 *   n_matches = 1   s[t] == s[t + k] as the periodicity matrix has it (prf_period.h): N == N matches, every other letter matches
 *                   itself only.  Line k is then exactly the diagonal col - row = k of the rectangle s x s of prf_dotchain.h on
 *                   the plus strand.
 *   n_matches = 0   the same, and the symbol is not N: the rule of the scans (reference utils/perfect_repeat_tracker.py:53).
 * SEEDS (maximal raw runs of at least min_seed cells), LINKS (at most max_gap cells strictly between two consecutive seeds) and
 * CHAINS (maximal sequences of linked seeds) are those of prf_dotchain.h, word for word.
 * start: t of the first seed's first cell, relative to `begin`.  len: the cells from there to the last seed's last cell.
 * matches: the raw cells among them.  seeds: the chain's seeds.  The repeat covers positions [start, start + len + k).
 * A call reports the chains with pos0 <= start < pos1 (clipped to n), kmin <= k <= kmax and len >= min_len (0: no filter).
 * Chains are judged on the whole line, never clipped by the window: the lists of any partition in positions and / or in k add up
 * to the whole list, each chain once.  The rows come back sorted ascending by (start, k).
 * Hence: at max_gap = 0 and n_matches = 0 the list holds every row (start, end, k) of the perfect scan of the same range as
 * (start, k, len = end - start - k, matches = len, seeds = 1), if len >= min_seed.
 * *n_chains is always the number of chains found.  dst is written -- all *n_chains rows, sorted -- only if *n_chains <= capacity;
 * otherwise dst is left untouched and the call still returns PRF_OK: compare and call again.  dst == NULL with capacity == 0
 * counts only.
 * Refusals, judged before the context or the genome is looked at, in this order: PRF_EINVAL for begin > end, pos0 > pos1,
 * kmin == 0, kmin > kmax, n_matches > 1, min_seed == 0; PRF_EUNSUPPORTED for max_gap above PRF_DOTCHAIN_MAX_GAP and for a capacity
 * above PRF_PCHAIN_MAX_ROWS; PRF_EINVAL for a NULL n_chains, or a NULL dst with a capacity other than 0.  Once the lengths are
 * known (the one-shot form: still before the context): PRF_EUNSUPPORTED for (pos1 - pos0) x (kmax - kmin + 1) above
 * PRF_DOT_MAX_CELLS.  PRF_EINVAL for a contig the genome does not hold or a genome of another context.  PRF_EUNSUPPORTED, loudly
 * and never a wrong list, if the runs and chains that are still going after PRF_DOTCHAIN_FOLLOW cells outnumber the list the call
 * keeps them in: ask for a smaller window.
 * A selection of parts, a row sink and the rows of the last scan are left alone, as by the other matrix products.
 * Stats: path = 10, scan_ms = HIP-event time of all launches (phase1_ms: the find kernel's, phase2_ms: the kernel's that
 * finishes the long list), positions = n, n_candidates = the seeds that start in the window, n_hits = *n_chains, n_launches.
 * The _ex form cuts the window's positions into launches of at most launch_cells cells (0: PRF_DOT_LAUNCH_CELLS), for the tests.
 * The one-shot form takes one sequence of ASCII (prf_genome_load + the call + prf_genome_free; PRF_ESYMBOL for a byte that is not
 * a letter, found on the host before the context is looked at). */
typedef struct prf_pchain {
    uint64_t start;    /* the first seed's first cell t, relative to begin: s[t] is the repeat's first position */
    uint64_t len;      /* cells from the first seed's first cell to the last seed's last cell                  */
    uint64_t matches;  /* raw cells among them                                                                 */
    uint32_t k;        /* the line: the period                                                                 */
    uint32_t seeds;    /* exact runs of at least min_seed cells in the chain                                   */
} prf_pchain;

#define PRF_PCHAIN_MAX_ROWS (1ull << 24)  /* rows of dst per call                                                             */
#define PRF_PCHAIN_LONG_ROWS (1ull << 20) /* runs and chains still going after PRF_DOTCHAIN_FOLLOW cells a call can finish    */

int prf_period_chains(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                      uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                      prf_pchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats);
int prf_period_chains_ex(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t pos0,
                         uint64_t pos1, uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap,
                         uint64_t min_len, prf_pchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats,
                         uint64_t launch_cells);
int prf_period_chains_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t pos0, uint64_t pos1,
                          uint32_t kmin, uint32_t kmax, uint32_t n_matches, uint64_t min_seed, uint32_t max_gap, uint64_t min_len,
                          prf_pchain *dst, uint64_t capacity, uint64_t *n_chains, prf_scan_stats *stats);

#endif /* PRF_PERIODCHAIN_H */
