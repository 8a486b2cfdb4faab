// alignpath_launch.h -- the launch wrappers of alignpath.hip, shared between it and alignpath_host.cpp; nobody else
// includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "alignpath_word.h"

struct prf_alignpath_args {
    prf_planes pl;            // H, L and X are read
    u64 g_begin;              // the range begins at this global position; every row ends inside the contig
    const ap_row *rows;       // sorted by regime (al_regime of the row's k); k <= PRF_AL_MAX_K, end - start <= PRF_AL_MAX_LEN
    const char *motifs;       // the sum of k letters, all of them motif letters
    al_result *dst;           // n_results rows, written at the rows' own indices by the forward kernel, read by the walk
    u64 n_results;
    u32 *trace;               // trace_words u32: every row of a launch has [trace, trace + ap_trace_words) inside
    u64 trace_words;
    unsigned short *path;     // n_path entries: every row has [path, path + end - start) inside
    u64 n_path;
    u32 *counts;              // 6 per motif letter, or NULL
};

// the forward pass, one wave per row: rows row0 .. row0 + n_rows - 1 of a.rows, all of `regime`; writes dst and the trace
hipError_t prf_launch_alignpath_forward(hipStream_t s, const prf_alignpath_args &a, u32 regime, u64 row0, u64 n_rows);
// the walk, one wave per row, rows of any regime: writes the path without its SUB bits and adds the deletions into counts
hipError_t prf_launch_alignpath_walk(hipStream_t s, const prf_alignpath_args &a, u64 row0, u64 n_rows);

// what the counts kernel reads: the rows in INPUT order, row r's path at first[r] (first[n_rows] = n_path)
struct prf_alignpath_count_args {
    prf_planes pl;
    u64 g_begin;
    const u64 *first;         // n_rows + 1, ascending
    const u64 *start;         // n_rows: the rows' first positions of the range
    const u64 *offset;        // n_rows: of the rows' letters in the motifs
    u64 n_rows;
    const char *motifs;
    unsigned short *path;
    u64 n_path;
    u32 *counts;              // or NULL
};

// one thread per entry of the path: sets the SUB bits and adds into counts 0 .. 3 and 5
hipError_t prf_launch_alignpath_counts(hipStream_t s, const prf_alignpath_count_args &a);
