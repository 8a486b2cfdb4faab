// align_launch.h -- the launch wrapper of align.hip, shared between it and align_host.cpp; nobody else includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "align_word.h"

struct prf_align_args {
    prf_planes pl;            // H, L and X are read
    u64 g_begin;              // the range begins at this global position; every row ends inside the contig
    const al_row *rows;       // sorted by regime (al_regime of the row's k); k <= PRF_AL_MAX_K, end - start <= PRF_AL_MAX_LEN
    const char *motifs;       // the sum of k letters, all of them motif letters
    al_result *dst;           // n_results rows, written at the rows' own indices
    u64 n_results;
};

// one wave per row: rows row0 .. row0 + n_rows - 1 of a.rows, all of `regime`
hipError_t prf_launch_align(hipStream_t s, const prf_align_args &a, u32 regime, u64 row0, u64 n_rows);
