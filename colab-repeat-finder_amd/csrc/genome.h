// genome.h -- what the host files of the perfect scan (genome.cpp, scan_host.cpp, literal_host.cpp, handoff.cpp) share and
// nobody else sees: the resident genome, what a scan of it launches, the parameters of a scan, and the three cold calls that
// cross between those files.  The matrix products see a genome through prf_contig_view (prf_ctx.h).
#pragma once
#include <utility>
#include <vector>

#include "prf_ctx.h"
#include "scan_vertical.h"

using tile_ranges = std::vector<std::pair<u64, u64>>;  // [first, last) tile ranges, ascending

struct prf_genome {
    prf_ctx *ctx = nullptr;
    std::vector<u64> base, len;
    u64 positions = 0;   // sum of contig lengths
    u64 G = 0;           // positions in the global coordinate space incl. gaps and the sentinel tile
    u64 nwords = 0;      // G / 64
    u64 padw = 0;        // readable words past nwords in every linear plane
    u32 kmax_hint = 0;
    u64 *H = nullptr, *L = nullptr, *X = nullptr;  // point PRF_FRONT_PAD words into their allocations
    // symbols outside ACGTN (ordinary symbols to the reference): five planes of their codes, present only if the input has
    // any; the tiles with such a symbol in reach (class 3) are scanned by the generic kernels
    u64 *E[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    u64 **d_E = nullptr;                            // the five pointers, on the device (fused kernel's general routine)
    tile_ranges exotic_tiles;                       // merged [first, last) ranges of class-3 tiles, ascending
    u64 *d_base = nullptr;
    uint4 *d_tile_info = nullptr;  // per tile: {contig, 0, contig base lo, hi}
    prf_vplanes vp;      // bit-sliced copy for scan_vertical
    // active selection (prf_genome_select): the scans of this genome cover only these tiles.  Off: the whole genome.
    bool sel_on = false;
    u32 *d_sel_list = nullptr;
    u32 sel_n = 0, sel_flat = ~0u;
    u64 sel_positions = 0;
    tile_ranges sel_tiles;       // merged [first, last) tile ranges, ascending
};

// the linear planes as the generic kernels and the matrix products take them
static inline prf_planes planes_of(const prf_genome *g) {
    return prf_planes{g->H, g->L, g->X, {g->E[0], g->E[1], g->E[2], g->E[3], g->E[4]}};
}

// what a scan of the genome launches
struct launch_view {
    const u32 *list;
    u32 n, flat;
    u64 positions;
};
static inline launch_view active_launch(const prf_genome *g) {
    if (g->sel_on) return launch_view{g->d_sel_list, g->sel_n, g->sel_flat, g->sel_positions};
    return launch_view{g->vp.launch_list, g->vp.n_launch, g->vp.flat_base, g->positions};
}

// the parameters of one scan
struct scan_params {
    u32 kmin, kmax, min_repeats, min_span;
};

// The cold calls between the files (everything on the path of a fused scan stays inside scan_host.cpp):
// literal_host.cpp -- min_repeats == 1 on a resident genome (from scan_impl), on sequences (stops == nullptr: from prf_scan)
__attribute__((visibility("hidden"))) int prf_literal_genome(prf_ctx *c, const prf_genome *g, const scan_params &p, prf_hits *out,
                                                             prf_scan_stats *stats);
__attribute__((visibility("hidden"))) int prf_literal_impl(prf_ctx *c, const prf_contig *contigs, int n_contigs, const u64 *stops,
                                                           const scan_params &p, prf_hits *out, prf_scan_stats *stats);
// handoff.cpp -- the count record behind a caller-owned row array
__attribute__((visibility("hidden"))) int prf_write_count_record(prf_ctx *c, prf_hit_dev *dst, u64 cap, u64 n);
