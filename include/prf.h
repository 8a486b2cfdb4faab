/*
 * prf.h -- C ABI of libprf, the MI355X (gfx950) perfect-tandem-repeat scanner.
 *
 * This is the drop-in boundary for the ONE hot path of
 * broadinstitute/colab-repeat-finder: "for every motif size k in [min,max]
 * compare seq[i] with seq[i+k] and report every maximal run that passes
 * min_repeats / min_span and whose motif is primitive".
 *
 * The reference has no FFI of its own (it is pure Python); the seam this
 * library sits behind is the Python call
 *
 *     detect_repeats(input_sequence, filter_settings, ...)      reference perfect_repeat_finder.py:10-81
 *
 * which drives one PerfectRepeatTracker per motif size
 * (reference utils/perfect_repeat_tracker.py:3-142).  A maintainer of the
 * reference binds these entry points with ctypes -- see INTEGRATION.md for the
 * stub -- and replaces the body of detect_repeats() with one prf_scan() call.
 *
 * Conventions: plain C types only; every function returns PRF_OK (0) or a
 * negative prf_status; nothing throws or exits across the boundary;
 * prf_last_error() gives a thread-local message for the last failure.
 * A prf_ctx is bound to one GPU and one HIP stream; calls on one ctx must be
 * serialised by the caller (the reference is single-threaded, re-entrant and
 * has no module globals -- neither has this library beyond the error string).
 * There is NO CPU fallback: without a usable gfx950 device prf_open() fails.
 */
#ifndef PRF_H
#define PRF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRF_ABI_VERSION 4

typedef enum prf_status {
    PRF_OK = 0,
    PRF_EINVAL = -1,       /* bad argument (same conditions the reference raises ValueError for, :23-30)  */
    PRF_ENODEV = -2,       /* no HIP device / wrong architecture                                          */
    PRF_EHIP = -3,         /* a HIP runtime call failed (see prf_last_error)                              */
    PRF_ENOMEM = -4,       /* host or device allocation failed                                            */
    PRF_EUNSUPPORTED = -5, /* this entry point does not serve the regime (kmax > hint; min_repeats == 1 on parts of a genome) */
    PRF_ESYMBOL = -6,      /* a byte that is not a letter: refused loudly, never guessed                  */
    PRF_EINDEX = -7        /* the reference raises IndexError on this input (utils/perfect_repeat_tracker.py:87: the
                            * extension loop's seq[i+1-period] reaches in front of the sequence; only with min_repeats == 1
                            * and a motif size larger than the sequence + 1)                               */
} prf_status;

typedef struct prf_ctx prf_ctx;       /* device, stream, scratch                           */
typedef struct prf_genome prf_genome; /* contigs packed and resident in HBM                */

/* One input sequence; caller-owned, read-only for the duration of the call.
 * Replaces the Python str handed to detect_repeats() (reference :10, :33). */
typedef struct prf_contig {
    const uint8_t *ascii; /* raw bytes, any case; upper-casing (reference :33) is folded into the packer */
    uint64_t len;
} prf_contig;

/* One output row = one (start_0based, end, motif) tuple of the reference (:81, :101);
 * the motif text is seq.upper()[start:start+k], materialised by the caller. */
typedef struct prf_hit {
    uint64_t start;  /* 0-based, contig-local                                  */
    uint64_t end;    /* exclusive                                              */
    uint32_t k;      /* motif size                                             */
    uint32_t contig; /* index into the contigs array                           */
} prf_hit;

typedef struct prf_hits {
    prf_hit *rows; /* library-owned; sorted by (contig, start, end) like reference :81 (on the device, fused path) */
    uint64_t n;
} prf_hits;

/* Per-call counters for bench.py / --stats (none of this exists in the reference). */
typedef struct prf_scan_stats {
    double scan_ms;         /* HIP-event time on the ctx stream: first scan kernel start -> hit count ready */
    double phase1_ms;       /* candidate-finding kernel(s)                                               */
    double phase2_ms;       /* candidate verification / extension / filters / compaction                 */
    uint64_t positions;     /* sum of contig lengths scanned                                             */
    uint64_t packed_bytes;  /* ceil(positions/4): the algorithmic input bytes                            */
    uint64_t n_candidates;  /* phase-1 candidates                                                        */
    uint64_t n_hits;        /* rows                                                                      */
    uint32_t n_launches;    /* kernel launches in the timed region                                       */
    uint32_t path;          /* 0 = generic kernel, 1 = vertical bit-sliced kernel, 2 = literal lane, 3 = interrupted, 4 = periodicity, 5 = dot plot, 6 = dot plot of two ranges, 7 = its diagonal runs as a list, 8 = those runs chained across mismatches */
    uint64_t seq;           /* fused path: serial number of this scan on its context (prf_scan_timings)  */
    uint32_t sorted_on_device; /* 1: the rows left the device sorted by (contig, start, end), no host sort   */
    uint32_t tiles_launched;   /* fused path: 65536-position tiles scanned (tiles of nothing but N are skipped)     */
} prf_scan_stats;

/* prf_scan flags */
#define PRF_SCAN_DEFAULT 0u
#define PRF_SCAN_FORCE_GENERIC 1u /* use the generic (any k, any thresholds) kernel even if a tuned one exists */
#define PRF_SCAN_NO_FETCH 2u      /* leave rows on the device (out may be NULL); for timing loops               */
#define PRF_SCAN_DEFER_TIMING 4u  /* fused path: do not wait for this scan's HIP events; scan_ms / phase*_ms are
                                   * reported as 0 and read later, for up to the last PRF_TIMING_RING scans, with
                                   * prf_scan_timings()                                                         */
#define PRF_TIMING_RING 128

int prf_abi_version(void);
int prf_device_count(void);
const char *prf_last_error(void);

/* Bind a context to HIP device `device_id` (must be gfx950). */
int prf_open(int device_id, prf_ctx **out);
void prf_close(prf_ctx *ctx);

/* Upload + pack contigs: ASCII -> 2-bit planes (+ a not-ACGT plane) resident in HBM.
 * Replaces input_sequence.upper() and the three transient copies of reference :33-46.
 * kmax_hint: largest motif size later scans will use (sizes the inter-contig guard gap). */
int prf_genome_load(prf_ctx *ctx, const prf_contig *contigs, int n_contigs, uint32_t kmax_hint, prf_genome **out);
/* The same, with the contigs generated ON the device (BASELINE config C5: 10^10 bp never cross PCIe):
 * contig i is lens[i] bases of the counter-based generator of SURVEY 8(d) with seed seeds[i],
 * base j = "ACGT"[splitmix64(seed + (j+1)*0x9E3779B97F4A7C15) >> 62]. */
int prf_genome_synth(prf_ctx *ctx, const uint64_t *lens, const uint64_t *seeds, int n_contigs, uint32_t kmax_hint,
                     prf_genome **out);
/* The same with the stand-in recipe for a chromosome (synth.py::standin2; no genome FASTA exists offline): uniform
 * background, N blocks at both ends and a centromere-like gap, one planted perfect tandem repeat per 588 positions. */
int prf_genome_standin(prf_ctx *ctx, const uint64_t *lens, const uint64_t *seeds, int n_contigs, uint32_t kmax_hint,
                       prf_genome **out);
void prf_genome_free(prf_genome *g);
uint64_t prf_genome_positions(const prf_genome *g);

/* Sharding ONE resident genome over several GPUs (north_star: "contigs x motif-sizes shard embarrassingly"; the
 * reference's analogue is the 500 kb interval fan-out of hail_batch_pipeline/run_hail_batch_pipeline.py:76-77).
 * Every rank holds the genome and selects the parts it scans: position ranges of contigs, cut at multiples of
 * prf_tile_positions().  A row belongs to the part that holds its first position, so the row sets of disjoint parts
 * are disjoint and their union over a cover of the genome is exactly the whole scan -- no halo, no exchange, no
 * repair step.  The selection stays in force for every following scan of the genome (synchronous or pipelined);
 * n_parts == 0 selects the whole genome again.  prf_scan_stats.positions then counts the selected positions. */
typedef struct prf_part {
    uint32_t contig;
    uint64_t begin; /* contig-local, a multiple of prf_tile_positions()                         */
    uint64_t end;   /* exclusive; a multiple of prf_tile_positions(), or >= the contig's length */
} prf_part;
uint64_t prf_tile_positions(void);
int prf_genome_select(prf_genome *g, const prf_part *parts, int n_parts);
/* Cost classes of a contig's tiles, for planners: 0 = ordinary, 1 = not-ACGT symbols in reach (slower variant),
 * 2 = nothing but not-ACGT (never scanned).  *n_tiles = ceil(len / prf_tile_positions()); at most `capacity` bytes
 * are written. */
int prf_genome_tile_classes(const prf_genome *g, uint32_t contig, uint8_t *dst, uint64_t capacity, uint64_t *n_tiles);

/* The hot path on a resident genome: every k in [kmin,kmax], rows as reference :81.
 * min_repeats == 1 (outside the closed form of the packed kernels: the reference's rows then depend on the text in front of
 * a run, on where the sequence begins and ends and on Python's negative-index wrap-around) is served by the literal lane:
 * the upper-cased bytes of every contig are rebuilt on the device from the planes, trimmed of the N at both ends (reference
 * :40-46) and scanned as prf_scan_literal() does; whole contigs only (PRF_EUNSUPPORTED while a selection of parts or a row
 * sink is set), rows on the host only (prf_last_hits_* then have nothing to hand over), PRF_EINDEX as there. */
int prf_scan_genome(prf_ctx *ctx, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                    uint32_t min_span, uint32_t flags, prf_hits *out, prf_scan_stats *stats);

/* One-shot convenience = prf_genome_load + prf_scan_genome + prf_genome_free.
 * This is the call that replaces the body of reference detect_repeats() (:33-81).
 * min_repeats == 1 is served by the literal lane (prf_scan_literal, contig by contig, flags ignored). */
int prf_scan(prf_ctx *ctx, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax,
             uint32_t min_repeats, uint32_t min_span, uint32_t flags, prf_hits *out, prf_scan_stats *stats);

/* The literal lane: the reference's per-tracker flush call (utils/perfect_repeat_tracker.py:71-101) evaluated as written,
 * per (position, motif size) (round 3: a thread owns 64 positions and decides from bit masks which events can pass the
 * filters at all; motif sizes above 63 one thread per four positions), on the upper-cased bytes of ONE sequence -- for the regimes outside the
 * closed form of the packed kernels: min_repeats == 1 (:86-91 then depend on the text in front of the run, on the slice
 * clamp at the end of the sequence and on Python's negative-index wrap-around), and a lock-step loop that stops early
 * (interval mode, reference perfect_repeat_finder.py:66-74).  `stop` = the number of iterations that loop performs
 * (>= contig->len: it runs to the end): every tracker stands at min(stop, len - k) when done() is called (:79).  Any
 * min_repeats >= 1 is accepted (the rows equal prf_scan's for min_repeats >= 2 and stop >= len); work is O(len x motif
 * sizes) byte compares, so this is the slow lane.  Rows sorted by (start, end), one row per (start, end): the shortest motif,
 * as the reference's dictionary keeps it (:93-101); prf_hit.k = len(motif), which is smaller than the motif size only where
 * the motif slice was clamped at the end of the sequence (:82).  PRF_EINDEX where the reference raises IndexError.  No
 * N-trimming here (reference perfect_repeat_finder.py:40-46 is the caller's; prf_scan does it for min_repeats == 1). */
int prf_scan_literal(prf_ctx *ctx, const prf_contig *contig, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                     uint32_t min_span, uint64_t stop, prf_hits *out, prf_scan_stats *stats);

/* ---- interrupted repeats: the reference's RepeatTracker with max_interruptions > 0 (utils/repeat_tracker.py) ----
 * The reference has no driver for that class; the one this library implements: every contig upper-cased and trimmed
 * of the N at both ends (reference perfect_repeat_finder.py:33-46), then one RepeatTracker per motif size k = kmin .. kmax, in
 * ascending order, over the trimmed contig, all writing ONE (start, end) -> motif dictionary of that contig; each tracker runs
 * `while t.advance(): pass; t.done()`.  Rows are the dictionary sorted by (start, end), shifted by the trimmed head; the motif
 * is seq.upper()[start:start+k] with N at the phases set in nmask (the reference's final_motif).  Whole contigs, many per call;
 * min_repeats >= 2 and kmax <= 64 (PRF_EUNSUPPORTED otherwise), max_interruptions >= 1 (0 is prf_scan's perfect path:
 * PRF_EINVAL), PRF_ESYMBOL for a byte that is not a letter.  Rows sorted by (contig, start, end) on the device.
 * Stats: path = 3, phase1_ms = the walk kernel, phase2_ms = emission and sort.
 * prf_scan_interrupted_by_k gives every motif size a budget of its own, RepeatTracker(k, ..., m_k, ...), with the same driver and
 * the same ONE dictionary; the three calls with one max_interruptions are that call with the same budget for every motif size. */
typedef struct prf_ihit {
    uint64_t start;  /* 0-based, contig-local      */
    uint64_t end;    /* exclusive                  */
    uint32_t k;      /* motif size                 */
    uint32_t contig; /* index into the contigs array */
    uint64_t nmask;  /* bit i: phase i of the motif may vary (an N in the motif text) */
} prf_ihit;

typedef struct prf_ihits {
    prf_ihit *rows; /* library-owned; free with prf_free_ihits */
    uint64_t n;
} prf_ihits;

#define PRF_MEMO_STRIDE 8u          /* prf_scan_interrupted: a state is recorded every 8 positions ...          */
#define PRF_MEMO_SLOTS (1ull << 22) /* ... in a table of at most this many records per lane                     */

int prf_scan_interrupted(prf_ctx *ctx, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax,
                         uint32_t min_repeats, uint32_t min_span, uint32_t max_interruptions, prf_ihits *out,
                         prf_scan_stats *stats);
/* The same with the walk's memo table chosen by the caller (memo_stride: a power of two, 0 = no memo; memo_slots: records per
 * (contig, motif size), 0 = no memo) -- the rows do not depend on either.  counters (may be NULL) receives four words: walk
 * steps (tracker moves), memo lookups, memo hits, recorded episodes. */
int prf_scan_interrupted_ex(prf_ctx *ctx, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax,
                            uint32_t min_repeats, uint32_t min_span, uint32_t max_interruptions, uint32_t memo_stride,
                            uint64_t memo_slots, prf_ihits *out, prf_scan_stats *stats, uint64_t *counters);
/* The walk of each (contig, motif size) cut into chunks of `chunk` landing positions, one GPU wave per chunk (every
 * jump back lands in the clean state on the next position behind a match followed by a mismatch, so the episodes that start in
 * different chunks do not depend on each other).  The rows do not depend on `chunk`.  chunk == 0: one lane per (contig, motif
 * size), the engine of prf_scan_interrupted_ex; 0 < chunk < PRF_INT_CHUNK_MIN: PRF_EINVAL (a lane looks for its first landing
 * from position chunk - 2 on).  counters (may be NULL) receives six words: the four of prf_scan_interrupted_ex, the lanes
 * launched, and the lanes dropped because a lane of an earlier chunk of their (contig, motif size) reached the end of the
 * contig.  prf_scan_interrupted() is this call with PRF_MEMO_STRIDE, PRF_MEMO_SLOTS and PRF_INT_CHUNK. */
#define PRF_INT_CHUNK_MIN 2u
#define PRF_INT_CHUNK (1ull << 20)
int prf_scan_interrupted_chunked(prf_ctx *ctx, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax,
                                 uint32_t min_repeats, uint32_t min_span, uint32_t max_interruptions, uint32_t memo_stride,
                                 uint64_t memo_slots, uint64_t chunk, prf_ihits *out, prf_scan_stats *stats, uint64_t *counters);
/* prf_scan_interrupted_chunked with a budget per motif size: max_interruptions_by_k[j] is the max_interruptions of the tracker
 * of k = kmin + j, kmax - kmin + 1 entries, read during the call only; NULL: PRF_EINVAL.  Every value is valid, 0 included: such
 * a k is scanned by RepeatTracker with max_interruptions = 0 (no phase varies; it differs from prf_scan's PerfectRepeatTracker in
 * the homopolymer rule and the previous-output rule), and all entries may be 0.  One call is not the merge of one call
 * per budget: a row of a small k keeps the same (start, end) from a larger k.  The other refusals, the rows, the statistics and
 * the six counters are those of prf_scan_interrupted_chunked. */
int prf_scan_interrupted_by_k(prf_ctx *ctx, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax,
                              uint32_t min_repeats, uint32_t min_span, const uint32_t *max_interruptions_by_k, uint32_t memo_stride,
                              uint64_t memo_slots, uint64_t chunk, prf_ihits *out, prf_scan_stats *stats, uint64_t *counters);
void prf_free_ihits(prf_ihits *hits);

/* ---- periodicity matrix and windowed period counts (the reference's get_period_matrix, utils/plot_utils.py:12-25) on a
 * resident genome: four more entry points of this library, additions to ABI version 4, declared in prf_period.h, which this
 * header includes below; prf_scan_stats.path = 4 is theirs. */

/* Pipelined scans.  prf_scan_genome_async() enqueues a scan and returns its serial number at once;
 * prf_scan_wait() collects it (row count and candidate count in *stats; kernel time through prf_scan_timings;
 * rows through prf_last_hits_to_device, valid until the next-but-one scan is enqueued).  At most two scans are in
 * flight, so the launch and the host's share of scan i+1 overlap the kernel of scan i.  Served only where it needs no
 * decisions on the way: fused path, no row sink, buffers sized by an earlier prf_scan_genome() of the same genome and
 * parameters; PRF_EUNSUPPORTED otherwise, and from prf_scan_wait() if those buffers overflowed -- scan
 * synchronously then.  No other call on the context while scans are in flight. */
int prf_scan_genome_async(prf_ctx *ctx, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                          uint32_t min_span, uint64_t *seq_out);
int prf_scan_wait(prf_ctx *ctx, uint64_t seq, prf_scan_stats *stats);

/* Row sink: the rows of the following scans on this context are compacted straight into caller-owned device
 * memory (e.g. the send buffer of an RCCL gather) instead of the library's own array.  dst_device must hold
 * capacity_rows + 1 prf_hit records; record number capacity_rows receives {start = number of rows, 0, 0, 0}.
 * With a sink set, prf_scan_genome returns only when all rows are in place (it drains its stream), and fails with
 * PRF_EINVAL if the scan finds more than capacity_rows rows.  dst_device == NULL: back to the internal array. */
int prf_set_row_sink(prf_ctx *ctx, void *dst_device, uint64_t capacity_rows);

/* HIP-event times (ms) of the two kernels of the fused scans first_seq .. first_seq+n-1 of this context (prf_scan_stats.seq);
 * they must be among its last PRF_TIMING_RING fused scans.  Waits for those scans' events. */
int prf_scan_timings(prf_ctx *ctx, uint64_t first_seq, uint32_t n, float *kernel_ms);
/* The same, per kernel: the fused scan kernel and the row gather that follows it (a third event lies between them). */
int prf_scan_timings_split(prf_ctx *ctx, uint64_t first_seq, uint32_t n, float *scan_ms, float *gather_ms);

void prf_free_hits(prf_hits *hits);

/* Device-side hand-off of the rows of the LAST prf_scan_genome() on this context (unsorted, 24-byte
 * prf_hit records): copied device-to-device into caller-owned device memory (e.g. a torch tensor that
 * an RCCL gather then ships to rank 0).  *n_rows receives the row count; at most capacity_rows are copied.
 * count_row != 0: the record at index capacity_rows (the buffer must hold capacity_rows+1 records) receives
 * {start = number of rows copied, end = 0, k = 0, contig = 0}, so that a padded gather carries its own length.
 * The copy is complete when the call returns. */
int prf_last_hits_to_device(prf_ctx *ctx, void *dst_device, uint64_t capacity_rows, int count_row, uint64_t *n_rows);

/* The same hand-off in the 8-byte wire format of the multi-GPU gather (a third of the bytes on the xGMI links): word i =
 * tile << 41 | start in the tile << 25 | min(end - start, 65535) << 9 | k, where tile * prf_tile_positions() + start in the
 * tile is the row's first position in the genome's coordinate space (contig c begins at prf_genome_contig_bases()[c]).
 * The tile has 23 bits, so the packed hand-off addresses 2^39 positions, half of what prf_genome_load accepts (2^40): a
 * resident genome of that size does not fit the device's memory, and the host encoder multi_gpu.pack_rows() refuses a row at
 * or beyond global position 2^39 with ValueError.
 * dst_device holds capacity_rows words, then ONE count word (rows | long rows << 40), then side_capacity full rows of three
 * words (start, end, k | contig << 32) for the rows whose span does not fit 16 bits.  multi_gpu.unpack_rows() decodes.
 * Fails with PRF_EINVAL if the scan found more rows than capacity_rows (or more long rows than side_capacity), and with
 * PRF_EUNSUPPORTED if the last scan's max motif size exceeds 511 (k has 9 bits on the wire: hand such rows over whole). */
int prf_last_hits_packed_to_device(prf_ctx *ctx, const prf_genome *g, void *dst_device, uint64_t capacity_rows,
                                   uint64_t side_capacity, uint64_t *n_rows);
/* A pipelined scan (prf_scan_genome_async) whose rows leave in that wire format with no host step in between: the pack
 * kernels run behind the scan on the library's stream and take the row count from the device.  dst_device as above; a scan
 * with more rows than capacity_rows (or more long rows than side_capacity) leaves an all-ones count word, which
 * multi_gpu.unpack_rows() refuses.  So does a scan that overflowed the buffers sized by the last synchronous scan (the row
 * array or a tile's slab: another genome or other parameters than were sized for): the pack reads no row beyond the row array,
 * and prf_scan_wait() fails with PRF_EUNSUPPORTED for exactly the scans whose count word is all ones for that reason.
 * Collect the scan with prf_scan_wait() as usual. */
int prf_scan_genome_async_packed(prf_ctx *ctx, const prf_genome *g, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                                 uint32_t min_span, void *dst_device, uint64_t capacity_rows, uint64_t side_capacity,
                                 uint64_t *seq_out);
/* Order: everything enqueued on the context's stream so far happens before what is enqueued on other_stream (a hipStream_t,
 * e.g. torch.cuda.Stream().cuda_stream) from now on.  The hand-off of a send buffer to a communication stream. */
int prf_stream_wait_for(prf_ctx *ctx, void *other_stream);

/* First position of every contig in the genome's coordinate space (multiples of prf_tile_positions()). */
int prf_genome_contig_bases(const prf_genome *g, uint64_t *bases, uint64_t capacity, uint64_t *n_contigs);

/* Device memory a resident genome holds (bytes: the packed planes in both layouts, tile tables, launch lists) and the positions
 * of its coordinate space (contigs + guard gaps, what the planes cover).  Round 3: 0.625 bytes per position -- three linear
 * planes (H, L, not-ACGT) and two bit-sliced ones; genomes with letters outside ACGTN add five linear planes. */
int prf_genome_footprint(const prf_genome *g, uint64_t *device_bytes, uint64_t *positions);

/* ---- the data formats either side of the path (host code, no GPU) ------------------------------------------
 * FASTA reader: what the reference takes from pyfastx.Fasta (perfect_repeat_finder.py:117,130,136-143): entries in
 * file order, name = header up to the first white space, sequence = the record's lines joined (case kept).
 * Plain or gzip-compressed files. */
typedef struct prf_fasta prf_fasta;
int prf_fasta_open(const char *path, prf_fasta **out);
/* One record only (reference fasta[chrom].seq, :130): read by seeking if an uncompressed file has a samtools-style
 * index path + ".fai" next to it, else parsed and filtered.  *out holds one entry, or none if the name is absent. */
int prf_fasta_open_contig(const char *path, const char *name, prf_fasta **out);
int prf_fasta_count(const prf_fasta *f);
int prf_fasta_entry(const prf_fasta *f, int i, const char **name, const uint8_t **seq, uint64_t *len);
void prf_fasta_close(prf_fasta *f);

/* Row writers: the reference's BED lines "chrom\tstart\tend\tmotif\n" (:148-149; names[i] / contigs[i] belong to
 * hit.contig == i) and its TSV file with the header "start_0based\tend\tmotif" (:166-170).  The motif is
 * seq.upper()[start:start+k], taken from the contig bytes. */
int prf_write_bed(const char *path, int append, const char *const *names, const prf_contig *contigs, int n_contigs,
                  const prf_hits *hits, uint64_t *n_written);
int prf_write_tsv(const char *path, const prf_contig *contig, const prf_hits *hits, uint64_t *n_written);

/* Host-only: describe, as one line of JSON, how a scan with these parameters is dealt to the waves of the fused
 * kernel (tasks, motif sizes, examined-group strides) or that the generic kernel is used.  Needs no GPU; used by
 * the CPU tests to check that every motif size is covered exactly once and that the sampling strides are legal.
 * Returns the length written (excluding the NUL), or PRF_EINVAL if buf is too small. */
int prf_plan_describe(uint32_t kmin, uint32_t kmax, uint32_t min_repeats, uint32_t min_span, char *buf, uint64_t buf_len);

/* Roofline probe: streaming 16-byte-per-lane read of `bytes` bytes, best of `iters`; GB/s (1e9). */
int prf_measure_hbm_read(prf_ctx *ctx, uint64_t bytes, int iters, double *gbps);

#include "prf_period.h"

/* ---- exact dot plot (the reference's plot_dot_plot.py: generate_matrix + filter_out_noise) of a range of a resident genome, as
 * bits or as counts per block: seven more entry points, additions to ABI version 4, declared in prf_dotplot.h, which this header
 * includes here; prf_scan_stats.path = 5 is theirs. */
#include "prf_dotplot.h"

/* ---- exact dot plot of two ranges, on either strand: six more entry points, additions to ABI version 4, declared
 * in prf_dotpair.h, which this header includes here; prf_scan_stats.path = 6 is theirs. */
#include "prf_dotpair.h"

/* ---- the diagonal runs of that dot plot as coordinates: three more entry points, additions to ABI version 4,
 * declared in prf_dotruns.h, which this header includes here; prf_scan_stats.path = 7 is theirs. */
#include "prf_dotruns.h"

/* ---- those runs chained across short stretches of mismatches on one line: three more entry points, additions to
 * ABI version 4, declared in prf_dotchain.h, which this header includes here; prf_scan_stats.path = 8 is theirs. */
#include "prf_dotchain.h"

/* ---- the junctions between those chains across neighbouring lines (indels): three more entry points, additions to
 * ABI version 4, declared in prf_dotlink.h, which this header includes here; prf_scan_stats.path = 9 is theirs. */
#include "prf_dotlink.h"

/* ---- the diverged tandem repeats of a range: chains on the period lines k = kmin .. kmax: three more entry points,
 * additions to ABI version 4, declared in prf_periodchain.h, which this header includes here; prf_scan_stats.path = 10 is theirs. */
#include "prf_periodchain.h"

/* ---- the indel junctions between those chains across neighbouring period lines: three more entry points, additions
 * to ABI version 4, declared in prf_periodlink.h, which this header includes here; prf_scan_stats.path = 11 is theirs. */
#include "prf_periodlink.h"

/* ---- the consensus motifs of such repeats: what each column of a repeat of period k holds: three more entry points,
 * additions to ABI version 4, declared in prf_consensus.h, which this header includes here; prf_scan_stats.path = 12 is theirs. */
#include "prf_consensus.h"

/* ---- the consensus motifs of GAPPED repeats: the same columns counted over segments with a phase: three more entry
 * points, additions to ABI version 4, declared in prf_phased.h, which this header includes here; prf_scan_stats.path = 13 is theirs. */
#include "prf_phased.h"

/* ---- the alignment of such repeats to their motifs: substitutions, insertions and deletions against the endless repetition of
 * the motif: two more entry points, additions to ABI version 4, declared in prf_align.h, which this header includes
 * here; prf_scan_stats.path = 14 is theirs. */
#include "prf_align.h"

/* ---- ... and the alignment itself: the path through the dynamic programming, one entry per position, and the counts of the
 * aligned columns: three more entry points, additions to ABI version 4, declared in prf_alignpath.h, which this header
 * includes here; prf_scan_stats.path = 15 is theirs. */
#include "prf_alignpath.h"
#include "prf_alignlocal.h"

#ifdef __cplusplus
}
#endif
#endif /* PRF_H */
