// consensus_launch.h -- the launch wrappers of consensus.hip, shared between it and consensus_host.cpp; nobody else
// includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "consensus_word.h"

struct prf_consensus_dev {    // = prf_consensus
    u64 offset, agree, acgt;
    u32 k, reserved;
};

struct prf_consensus_args {
    prf_planes pl;            // H, L and X are read
    u64 g_begin;              // the range begins at this global position; every row ends inside the contig
    const cs_row *rows;
    u64 n_rows;
    const cs_item *items;     // sorted by regime (cs_regime of the row's k); every item lies inside its row
    u32 *counts;              // 4 x the sum of k, zeroed by the caller
    char *motifs;             // the sum of k letters
    prf_consensus_dev *dst;   // n_rows rows
};

// one wave per item: items item0 .. item0 + n_items - 1, all of `regime`
hipError_t prf_launch_consensus_count(hipStream_t s, const prf_consensus_args &a, u32 regime, u64 item0, u64 n_items);
// one wave per row, behind all counts
hipError_t prf_launch_consensus_finish(hipStream_t s, const prf_consensus_args &a);
