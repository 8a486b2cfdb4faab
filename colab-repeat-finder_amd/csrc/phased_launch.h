// phased_launch.h -- the launch wrapper of phased.hip, shared between it and phased_host.cpp; nobody else includes
// it.  The letters and the sums of a row are written by the finish kernel of consensus.hip (consensus_launch.h), from the same
// counts.
#pragma once
#include "consensus_launch.h"
#include "phased_word.h"

struct prf_phased_args {
    prf_planes pl;              // H, L and X are read
    u64 g_begin;                // the range begins at this global position; every segment ends inside the contig
    const cs_row *rows;         // offset and k are read
    u64 n_rows;
    const ph_segment *segments; // every segment names a row below n_rows and a phase below its k
    u64 n_segments;
    const ph_item *items;       // sorted by regime (cs_regime of the row's k); every item lies inside its segment
    u32 *counts;                // 4 x the sum of k, zeroed by the caller
};

// one wave per item: items item0 .. item0 + n_items - 1, all of `regime`
hipError_t prf_launch_phased_count(hipStream_t s, const prf_phased_args &a, u32 regime, u64 item0, u64 n_items);
