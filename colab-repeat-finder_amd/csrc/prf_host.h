// prf_host.h -- launch wrappers shared between the kernel translation units and the host ones that call them (context.cpp, genome.cpp, scan_host.cpp, literal_host.cpp, handoff.cpp,
// interrupted.cpp, periodicity_host.cpp, dotplot_host.cpp, dotpair_host.cpp, dotruns_host.cpp, dotchain_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "prf_device.h"

// device counter block (u64 each)
enum {
    PRF_CNT_CAND = 0,      // generic path: phase-1 candidates
    PRF_CNT_HITS = 1,      // generic path: rows
    PRF_CNT_BADPOS = 2,    // packer: first byte that is not a letter
    PRF_CNT_EXOTIC = 7,    // packer: 1 = the input holds letters other than A, C, G, T, N
    PRF_CNT_UNSORTED = 3,  // fused path: a tile wrote rows past its LDS sort list -> the row array is not fully sorted
    PRF_CNT_HIT_OVF = 4,   // fused path: largest per-tile row demand above the slab capacity
    PRF_CNT_ROWS = 5,      // fused path: rows in the compact array (written by the gather kernel)
    PRF_CNT_TICKET = 6,    // fused path: gather workgroups finished (the last one hands the counters to the host)
    PRF_CNT_SHARD0 = 8,    // fused path: candidate-record counts (statistics), sharded over 16 cache lines by tile
    PRF_CNT_NSHARD = 16,
    PRF_CNT_SHARD_STRIDE = 8,
    PRF_SH_CAND = 1,
    PRF_SH_EARLY = 4,        // fused path: candidates verified on the spot because a tile's list was full (diagnostic)
    PRF_SH_TILE_TICKET = 2,  // fused path, shards 0..7: launch slots handed out to the persistent workgroups of XCD 0..7
    PRF_CNT_LONG_OVF = 8 + 3,  // fused path (shard 0, word 3): a tile held more than PRF_LONG_PER_TILE rows with a clipped span (cannot happen)
    PRF_CNT_N = 8 + 16 * 8
};

hipError_t prf_launch_pack_linear(hipStream_t s, const uint8_t *asc, u64 nwords, u64 *H, u64 *L, u64 *X,
                                  u64 *bad_pos, u64 *exotic);
hipError_t prf_launch_pack_exotic(hipStream_t s, const uint8_t *asc, u64 nwords, u64 *const *E);
hipError_t prf_launch_fill_u64(hipStream_t s, u64 *p, u64 n, u64 v);
hipError_t prf_launch_synth(hipStream_t s, uint8_t *asc, u64 n, u64 seed);
// stand-in recipe 2 (synth.py::standin2): background + N blocks + one planted repeat per 588-position slot
hipError_t prf_launch_standin2(hipStream_t s, uint8_t *asc, u64 n, u64 seed);

hipError_t prf_launch_scan_generic(hipStream_t s, const prf_planes &pl, u64 w_begin, u64 w_end, u32 kmin, u32 kmax,
                                   u32 min_repeats, u32 min_span, u64 *cand, u64 cand_cap, u64 *counters);

hipError_t prf_launch_verify(hipStream_t s, const prf_planes &pl, const u64 *cand, u64 cand_cap, u32 min_repeats,
                             u32 min_span, const u64 *contig_base, u32 n_contigs, prf_hit_dev *hits, u64 hit_cap,
                             u64 *counters);

hipError_t prf_launch_hbm_read(hipStream_t s, const void *p, u64 bytes, u32 *sink);
hipError_t prf_launch_pack_rows(hipStream_t s, const prf_hit_dev *rows, u64 n, const u64 *contig_base, u64 *dst, u64 cap, u64 side_cap,
                                u64 *side_cnt, u64 *host_word);

// the same with the row count read on the device (behind a scan that is still in flight); side_cnt must be zero and is zero again afterwards.
// counters: the base of the scan's counter block; rows_cap, slab_cap: the row array and the slabs the scan was launched with -- a scan
// that overflowed either leaves the all-ones count word, and no row beyond rows_cap is read
hipError_t prf_launch_pack_rows_dev(hipStream_t s, const prf_hit_dev *rows, const u64 *counters, u64 rows_cap, u64 slab_cap, u64 cap,
                                    const u64 *contig_base, u64 *dst, u64 side_cap, u64 *side_cnt);

// literal lane (scan_literal.hip): upper-case in place + first non-letter; one thread per (position, motif size) event
hipError_t prf_launch_lit_upper(hipStream_t s, uint8_t *seq, u64 n, u64 *bad_pos);
hipError_t prf_launch_lit_events(hipStream_t s, const uint8_t *seq, u64 L, u32 kmin, u32 kmax, u32 min_repeats, u32 min_span,
                                 u64 stop, u32 contig, prf_hit_dev *rows, u64 cap, u64 *counters);
// the same lane on a resident genome: first / one-past-last position of a contig that is not N (atomicMin / atomicMax into
// first_last[0..1]); the upper-cased bytes of n positions from global position g0 rebuilt from the linear planes
hipError_t prf_launch_lit_trim(hipStream_t s, const u64 *X, const u64 *const *E, u64 word0, u64 len, u64 *first_last);
hipError_t prf_launch_lit_unpack(hipStream_t s, const u64 *H, const u64 *L, const u64 *X, const u64 *const *E, u64 g0, u64 n,
                                 uint8_t *out);
// the rows of the event kernel sorted by (start, end) and reduced to the shortest motif per (start, end), on the device
hipError_t prf_lit_sort_unique(hipStream_t s, const prf_hit_dev *rows, u64 n, prf_hit_dev *out, u64 *n_out, void **scratch,
                               size_t *scratch_bytes);

// interrupted repeats (scan_interrupted.hip), one lane per (sequence, motif size, chunk of landing positions) -- DESIGN 9
struct prf_ilane {
    u64 seq_base;             // byte offset of the (upper-cased, untrimmed) sequence in the buffer, 16-byte aligned
    u64 cand_off, cand_cap;   // the lane's candidate list
    u64 memo_off, memo_slots; // its memo table (memo_slots == 0: no memo)
    u64 ep_off, ep_cap;       // its episode outcome words (episodes past ep_cap are not recorded)
    u32 seq, k;
    u64 lo, hi;               // the lane walks the episodes that land in [lo, hi) (trimmed positions); lo == 0: from position 0
    u32 chunk, kslot;         // its chunk's number within (sequence, k); index of that (sequence, k)
    u32 max_int, pad_;        // phases of the motif that may vary in this lane: the budget of its motif size (0: none)
};
struct prf_icand {            // an output check that passed both span tests with no N in the motif
    u64 start, end, mask;     // trimmed coordinates; mask: the phases allowed to vary
    u32 homo, k;
};
struct prf_imemo {            // a state an episode passed through
    u64 pos, mask, run;
    u64 ep;                   // index of that episode's outcome word
};
struct prf_ihit_dev {         // = prf_ihit
    u64 start, end;
    u32 k, contig;
    u64 nmask;
};
hipError_t prf_launch_int_trim(hipStream_t s, const uint8_t *buf, const u64 *seq_base, const u64 *chunks, u32 n_chunks,
                               u64 *first_last);
// what the walk writes and the emission reads
struct prf_int_lanes {
    const prf_ilane *lanes;
    u32 n_lanes;
    const u64 *first_last;    // per sequence: first / one-past-last position that is not N (first == ~0: nothing but N)
    prf_icand *cands;         // the lanes' candidate lists (prf_ilane::cand_off, cand_cap)
    u64 *cand_cnt;            // per lane: candidates the walk found (above cand_cap: the list holds the first cand_cap)
    u32 *lane_end;            // per lane: the walk ended in this lane
};
// counters[0..3] += steps, memo lookups, memo hits, recorded episodes.
// first_end == NULL: one lane per thread (one chunk per (sequence, k)).  Otherwise one lane per wave, and first_end[kslot]
// (set to ~0 by the caller) receives the first chunk of each (sequence, k) whose lane ended.
struct prf_int_walk_args {
    prf_int_lanes l;
    const uint8_t *buf;
    u32 min_repeats, min_span, stride;  // (the budget of varying phases travels with each lane)
    u32 *first_end;
    prf_imemo *memo;
    u32 *eps;
    u64 *counters;
};
hipError_t prf_launch_int_walk(hipStream_t s, const prf_int_walk_args &a);
// bcount[li] += the boundaries in lane li's [lo, hi): with one more for position 0, an upper bound of its episodes and candidates
hipError_t prf_launch_int_bound(hipStream_t s, const uint8_t *buf, const prf_ilane *lanes, u32 n_lanes, const u64 *first_last,
                                u64 *bcount);
// one thread per sequence: its lanes are lane0[s] + j * n_chunks[s] + c for motif size j of nk and chunk c; its hash of emitted
// (start, end) is keys[2 * hash_off[s] ..] with hash_size[s] slots (a power of two, zeroed by the caller); *row_cnt += its rows
struct prf_int_emit_args {
    prf_int_lanes l;
    u32 nk, n_seq;
    const u32 *lane0, *n_chunks;
    const u64 *hash_off, *hash_size;
    u64 *keys;
    prf_ihit_dev *rows;
    u64 *row_cnt;
};
hipError_t prf_launch_int_emit(hipStream_t s, const prf_int_emit_args &a);
size_t prf_int_sort_scratch_bytes(u64 n);
hipError_t prf_int_sort_rows(hipStream_t s, const prf_ihit_dev *rows, u64 n, prf_ihit_dev *out, void *scratch);

// periodicity matrix (periodicity.hip): cells seq[i] == seq[i + k] of `len` positions from global position g_begin,
// for k = kmin .. kmax; N == N matches, nothing at or behind g_begin + len is compared (or read)
struct prf_periodicity_args {
    prf_planes pl;
    u64 g_begin, len;
    u64 n_words;      // ceil(len / 64)
    u64 n_windows;    // counts: ceil(n_words / wpw)
    u32 kmin, kmax;
    u32 wpw;          // counts: words per window (window / 64); bits: 1
    u64 *bits;        // want_bits: (kmax - kmin + 1) x n_words words, every one written
    u32 *counts;      // otherwise: (kmax - kmin + 1) x n_windows sums, zeroed by the caller
    u32 span_words, kslice, lds_stride;  // set by the launch wrapper (prf_periodicity_shape)
};
#define PRF_PER_LDS_BYTES 65536u
// words of the range per workgroup, motif sizes per slice, LDS words per plane
void prf_periodicity_shape(bool exotic, u32 *span_words, u32 *kslice, u32 *lds_stride);
hipError_t prf_launch_periodicity(hipStream_t s, prf_periodicity_args a, bool want_bits);

// dot plot (dotplot.hip): kept cells (s[i] == s[j], filtered by diagonal runs) of window rows x columns of the
// n x n matrix of the n positions from global position g_begin; N == N matches, nothing at or behind g_begin + n is compared
// (or read), runs are judged on the whole matrix
struct prf_dotplot_args {
    prf_planes pl;
    u64 g_begin, n;
    u64 row0, col0, col1;   // the window (clipped to n); its rows end with lrow1 of the last launch
    u64 lrow0, lrow1;       // rows of this launch: lrow0 - row0 is a multiple of tile_rows
    u64 words_per_row;      // ceil((col1 - col0) / 64)
    u32 m;                  // cells a run must have: max(min_diagonal_run - 1, 1)
    u32 wpb;                // counts: words per block (block / 64)
    u64 n_block_cols;       // counts: ceil(words_per_row / wpb)
    u64 *bits;              // want_bits: rows x words_per_row words, every one written
    u32 *counts;            // otherwise: block rows x n_block_cols sums, zeroed by the caller
    u32 tile_rows, span_words, halo, n_spans;  // set by the launch wrapper (prf_dotplot_shape_for)
};
// rows per workgroup tile, words of 64 columns per workgroup span, halo rows above and below (= m - 1); the same for 3 and 8 planes
void prf_dotplot_shape_for(u32 min_diagonal_run, u32 *tile_rows, u32 *span_words, u32 *halo);
hipError_t prf_launch_dotplot(hipStream_t s, prf_dotplot_args a, bool want_bits);

// dot plot of two ranges (dotplot_pair.hip): kept cells of window rows x columns of the na x nb matrix A[i] == B[j]
// (strand 0) or A[i] == comp(B[j]) (strand 1), A = the na positions from global position a_g_begin, B = the nb from b_g_begin,
// both of the same planes; nothing at or behind either range's end is compared (or read), runs are judged on the whole rectangle.
// The fields that prf_dotplot_args has too mean the same.
struct prf_dotpair_args {
    prf_planes pl;
    u64 a_g_begin, na, b_g_begin, nb;
    u64 row0, col0, col1;
    u64 lrow0, lrow1;
    u64 words_per_row;
    u32 m;
    u32 wpb;
    u64 n_block_cols;
    u64 *bits;
    u32 *counts;
    u32 strand;
    u32 tile_rows, span_words, halo, n_spans;  // set by the launch wrapper (prf_dotplot_shape_for)
};
hipError_t prf_launch_dotpair(hipStream_t s, prf_dotpair_args a, bool want_bits);

// diagonal runs of the dot plot of two ranges as a list (dotruns.hip): the maximal runs of raw cells along (+1, +1)
// (dir 1) and (+1, -1) (dir 2) of the na x nb rectangle whose start cell lies in window rows x columns; the ranges, the strand and
// the fields that prf_dotpair_args has too mean the same.
struct prf_dotrun_dev {       // = prf_dotrun
    u64 row, col, len;
    u32 dir, reserved;
};
enum { PRF_DR_RUNS = 0, PRF_DR_LONG = 1, PRF_DR_N = 2 };   // the call's two counters: runs found, entries of the long list
struct prf_dotruns_args {
    prf_planes pl;
    u64 a_g_begin, na, b_g_begin, nb;
    u64 col0, col1;
    u64 lrow0, lrow1;         // rows of this launch (the last launch ends with the window); lrow0 - row0 is a multiple of 64
    u64 words_per_row;
    u64 min_len;
    u32 strand, directions;
    u32 p;                    // probe depth: min(min_len, PRF_DOTRUN_PROBE)
    u32 span_words, n_spans;  // set by the launch wrapper
    prf_dotrun_dev *dst;      // `capacity` rows; runs behind them are counted, not written
    u64 capacity;
    prf_dotrun_dev *longs;    // runs still going after PRF_DOTRUN_FOLLOW cells: start, cells so far, direction
    u64 long_cap;
    u64 *counters;            // PRF_DR_N words, zeroed by the caller
};
hipError_t prf_launch_dotruns_find(hipStream_t s, prf_dotruns_args a);
// one wave per entry of the long list; n_long = min(the list's count, long_cap), read by the caller
hipError_t prf_launch_dotruns_long(hipStream_t s, const prf_dotruns_args &a, u64 n_long);

// chains of those runs across short stretches of mismatches on one line (dotchain.hip).  The seeds are the rows the
// two kernels above wrote at min_len = min_seed, left on the device; the ranges, the strand and the planes are read from the same
// prf_dotruns_args, of which the chain kernels use pl, a_g_begin, na, b_g_begin, nb and strand only.
struct prf_dotchain_dev {     // = prf_dotchain
    u64 row, col, len, matches;
    u32 dir, seeds;
};
struct prf_dotchain_long {    // a chain that is still going after PRF_DOTCHAIN_FOLLOW cells, with the state of its walk
    u64 i0, j0;               // the line's first cell
    u64 t0;                   // the first seed's first cell, in cells of the line
    u64 end;                  // the last committed seed's last cell
    u64 matches, pending;     // raw cells up to `end`; raw cells of the short runs behind it
    u64 p;                    // the next cell to look at
    u64 run_start;            // in_run: the first cell of the run that holds cell p - 1
    u32 dir, seeds, in_run, reserved;
};
enum { PRF_DC_CHAINS = 0, PRF_DC_LONG = 1, PRF_DC_N = 2 };   // the chain kernels' two counters: chains found, entries of the long list
struct prf_dotchain_args {
    const prf_dotrun_dev *seed_rows;
    u64 n_seeds;
    u64 min_seed, min_len;
    u32 max_gap;
    prf_dotchain_dev *dst;    // `capacity` rows; chains behind them are counted, not written
    u64 capacity;
    prf_dotchain_long *longs;
    u64 long_cap;
    u64 *counters;            // PRF_DC_N words, zeroed by the caller
};
hipError_t prf_launch_dotchain_link(hipStream_t s, const prf_dotruns_args &a, const prf_dotchain_args &c);
// one wave per entry of the long list; n_long = min(the list's count, long_cap), read by the caller
hipError_t prf_launch_dotchain_long(hipStream_t s, const prf_dotruns_args &a, const prf_dotchain_args &c, u64 n_long);

// junctions between those chains across neighbouring lines (dotlink.hip).  The seeds are the same rows, left on the
// device; the heads kernel lists the seeds of the window that start a chain, the join kernel judges one head per wave.
struct prf_dotlink_dev {      // = prf_dotlink
    u64 row, col, from_row, from_col;
    u32 dir;
    int shift;
    u32 gap, overlap;
};
enum { PRF_DL_HEADS = 0, PRF_DL_LINKS = 1, PRF_DL_N = 2 };   // the link kernels' two counters: chain heads of the window, links found
struct prf_dotlink_args {
    const prf_dotrun_dev *seed_rows;
    u64 n_seeds;
    u64 min_seed;
    u32 max_gap, max_shift;
    u32 *heads;               // n_seeds entries: the indices of the seeds that start a chain, in no order
    prf_dotlink_dev *dst;     // `capacity` rows; links behind them are counted, not written
    u64 capacity;
    u64 *counters;            // PRF_DL_N words, zeroed by the caller
};
hipError_t prf_launch_dotlink_heads(hipStream_t s, const prf_dotruns_args &a, const prf_dotlink_args &c);
// one wave per head; n_heads = the heads' count, read by the caller
hipError_t prf_launch_dotlink_join(hipStream_t s, const prf_dotruns_args &a, const prf_dotlink_args &c, u64 n_heads);

// chains on the period lines of one range (periodchain.hip): the find kernel forms the cells of lines kmin .. kmax from
// planes staged in LDS, finds the run starts of the window, probes, measures, tests for a head and follows; the long kernel
// finishes, one wave per entry, what was still going after PRF_DOTCHAIN_FOLLOW cells.
struct prf_pchain_dev {       // = prf_pchain
    u64 start, len, matches;
    u32 k, seeds;
};
struct prf_pchain_long {      // a first run (phase 0) or a chain (phase 1) that is still going, with the state of its walk
    u64 t0;                   // the first seed's first cell
    u64 end, matches, pending, p, run_start;   // dc_state; phase 0: p only, the next cell of the run to look at
    u32 k, seeds, in_run, phase;
};
enum { PRF_PC_CHAINS = 0, PRF_PC_LONG = 1, PRF_PC_SEEDS = 2, PRF_PC_N = 3 };   // chains found, entries of the long list, seeds of the window
struct prf_periodchain_args {
    prf_planes pl;
    u64 g_begin, n;           // the range: n positions from global position g_begin
    u64 n_words;              // ceil(n / 64)
    u64 pos0, pos1;           // the window of starts (clipped to n)
    u64 word0, word1;         // words of the range this launch looks for starts in
    u32 kmin, kmax;           // kmax < n
    u32 n_matches, max_gap;
    u64 min_seed, min_len;
    prf_pchain_dev *dst;      // `capacity` rows; chains behind them are counted, not written
    u64 capacity;
    prf_pchain_long *longs;
    u64 long_cap;
    u64 *counters;            // PRF_PC_N words, zeroed by the caller
    u32 span_words, kslice, lds_stride;   // set by the launch wrapper (prf_periodchain_shape)
};
void prf_periodchain_shape(bool exotic, u32 *span_words, u32 *kslice, u32 *lds_stride);
hipError_t prf_launch_periodchain_find(hipStream_t s, prf_periodchain_args a);
// one wave per entry of the long list; n_long = the list's count (<= long_cap), read by the caller
hipError_t prf_launch_periodchain_long(hipStream_t s, const prf_periodchain_args &a, u64 n_long);

// junctions between those chains across neighbouring period lines (periodlink.hip).  The heads are the rows the two
// kernels above wrote at min_len = 0, left on the device; the join kernel judges one head per wave against ALL lines 1 .. n - 1.
struct prf_plink_dev {        // = prf_plink
    u64 start, from_end;
    u32 k;
    int shift;
    u32 gap, overlap;
};
struct prf_periodlink_args {
    prf_planes pl;
    u64 g_begin, n;           // the range, as prf_periodchain_args
    u32 n_matches, max_gap, max_shift;
    u64 min_seed;
    const prf_pchain_dev *heads;   // n_heads rows: the chains that start in the window, in no order
    u64 n_heads;
    prf_plink_dev *dst;       // `capacity` rows; links behind them are counted, not written
    u64 capacity;
    u64 *counter;             // one word, zeroed by the caller: links found
};
// one wave per head
hipError_t prf_launch_periodlink_join(hipStream_t s, const prf_periodlink_args &a);
