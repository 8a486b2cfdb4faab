/*
 * prf_period.h -- the periodicity entry points of libprf: part of the C ABI of include/prf.h, which includes this file inside
 * its extern "C" block (include prf.h, not this file).  They live in a header of their own so that the list of entry points
 * of prf.h proper -- prf_native.EXPORTS -- stays what it was; these four are prf_native.PERIOD_EXPORTS.
 */
#ifndef PRF_PERIOD_H
#define PRF_PERIOD_H
#ifndef PRF_H
#error "include prf.h, which includes prf_period.h"
#endif

/* ---- periodicity matrix: the reference's get_period_matrix (utils/plot_utils.py:12-25) on a resident genome ----
 * Cell (k, i) of a sequence s is set iff s[i] == s[i + k], 0 <= i < len(s) - k, by plain comparison of the upper-cased symbols:
 * unlike the scans, N == N IS a match here (and any other letter matches itself and nothing else).  s is positions
 * [begin, end) of one contig (end beyond the contig is clipped to its length); nothing at or behind `end` is compared, so a row
 * ends with the range, not with the guard gap behind the contig; rows of k >= end - begin are all zero.  k = kmin .. kmax,
 * kmax at most the genome's kmax_hint (PRF_EUNSUPPORTED above it).
 * prf_period_bits: the cells.  dst (host memory) receives (kmax - kmin + 1) rows of *words_per_k = ceil((end - begin) / 64)
 * words; bit j of word w of row k - kmin is cell (k, begin + 64 w + j); tail bits are zero.  capacity_words: words dst holds
 * (PRF_EINVAL if too few, or if dst is NULL).  An output of more than PRF_PERIOD_BITS_MAX_WORDS words (2 GiB) is
 * PRF_EUNSUPPORTED: ask for counts, or for fewer rows or positions per call.
 * prf_period_counts: the periodicity profile.  dst receives (kmax - kmin + 1) rows of *n_windows = ceil((end - begin) / window)
 * sums; entry (k - kmin, w) = the number of set cells (k, i) with begin + w * window <= i < begin + (w + 1) * window.  window: a
 * multiple of 64, at least 64 and at most 2^31 (PRF_EINVAL otherwise).  capacity: entries dst holds (PRF_EINVAL if too few, or if
 * dst is NULL).
 * Both ignore a selection of parts (prf_genome_select) and leave a row sink and the rows of the last scan alone.  The arguments
 * are judged before the context or the genome is looked at.  Stats: path = 4, scan_ms = HIP-event time of the kernel,
 * positions = end - begin, n_hits = 0.
 * The one-shot forms take one sequence of ASCII (prf_genome_load with kmax_hint = kmax + the call + prf_genome_free; PRF_ESYMBOL
 * for a byte that is not a letter, found on the host before the context is looked at), as prf_scan is to prf_scan_genome. */
#define PRF_PERIOD_BITS_MAX_WORDS (1ull << 28)
int prf_period_counts(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint32_t kmin,
                      uint32_t kmax, uint64_t window, uint32_t *dst, uint64_t capacity, uint64_t *n_windows,
                      prf_scan_stats *stats);
int prf_period_bits(prf_ctx *ctx, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint32_t kmin,
                    uint32_t kmax, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_k, prf_scan_stats *stats);
int prf_period_counts_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                          uint64_t window, uint32_t *dst, uint64_t capacity, uint64_t *n_windows, prf_scan_stats *stats);
int prf_period_bits_seq(prf_ctx *ctx, const prf_contig *seq, uint64_t begin, uint64_t end, uint32_t kmin, uint32_t kmax,
                        uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_k, prf_scan_stats *stats);

#endif /* PRF_PERIOD_H */
