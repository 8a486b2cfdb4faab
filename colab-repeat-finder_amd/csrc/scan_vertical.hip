// scan_vertical.hip -- the fast path: fused bit-sliced ("vertical") scan + verification kernel for gfx950.
// (The row gather that follows it: scan_gather.hip.  The ASCII -> bit-sliced packer: pack.hip.  The work planner is host
// code: plan.cpp.)  The kernel's sections, included once each below: vscan_common.h, vscan_verify.h, vscan_tasks.h.
//
// What the kernels replace: the L x n_k calls of PerfectRepeatTracker.advance()
// (reference utils/perfect_repeat_tracker.py:43-61), the per-run filter/emit step (:71-101, :108-142) and -- with the
// gather -- the final sorted() of the rows (reference perfect_repeat_finder.py:81), for any kmin..kmax <= 480 and any
// thresholds with min_repeats >= 2.
//
// Layout.  A tile is 65536 consecutive positions, cut into 2048 streams of T = 32 positions.  Stream
// s = bit*64 + lane lives in bit `bit` of lane `lane`: the 32-bit word W[t][lane] holds, in bit b,
// position  tile*65536 + (b*64 + lane)*32 + t.  One wave-wide word row therefore advances 2048
// independent streams by one position, and "position j+k" is simply row t+k of the same lane (or,
// past the end of the stream, row (t+k)%32 of lane + (t+k)/32, because the next stream of a lane is the
// same bit of the next lane).  Lanes 64.. of that virtual lane axis are the first lanes again, moved up
// one bit, with bit 31 taken from the next tile; they are materialised once per tile in LDS.
// In HBM a plane of a tile is stored [t/4][lane][t%4] so that one lane reads 4 rows with one 16-byte
// access and a wave reads 1 KiB contiguously; the LDS image has the same shape with 64+J lanes.
// The shift by k therefore costs no instruction: it is an LDS address.
//
// One 256-thread workgroup per tile, SIX resident per CU (round 3; four before): <= 80 VGPRs and <= 27.3 KB of LDS.
// What made room: ONE 18 KB region R1 is the bit-sliced image while the tile is scanned and the window of the linear
// planes while its candidates are verified (before: two regions, 35 KB); the image arrives by LDS-DMA
// (global_load_lds_dwordx4: no staging registers, no ds_write pass) while the previous tile's rows are sorted, the
// window through the registers of the two waves that finish their tasks first; the exact tasks slide over the stream
// with a window of K + 4 rows in registers instead of all 60.
//  1. stage: the image arrived by DMA; 128 threads add the virtual lanes 64.. (one shift/or of two prefetched slots).
//  2. scan: every wave runs its share of the plan's tasks (host-built, balanced by cost).  A task answers one
//     question per (stream, motif size): "may a reportable run be found from this stream?" --
//      * exact task, one motif size k with M(k) = M <= 8 (compiled per (k, M)): mismatch word per row
//        (2 operations), sliding OR over exactly M rows; a row whose M successors all match and whose predecessor
//        does not is the start of a run of >= M.  k = 2, 3, 4 on a clean tile leave out the starts whose run is the
//        echo of a shorter motif (tested once per segment of start rows, vscan_tasks.h): never a row.  The echoes k = 2
//        leaves out are the homopolymer starts: where min_span >= 2 min_repeats they ARE the k = 1 task's answer on a
//        clean tile, and that task is not run there (prf_plan_derives_k1).
//      * coarse task, one motif size with 9 <= M <= 14: the same on aligned groups of 2 or 4 rows (a run of >= M rows
//        holds floor((M + 1) / G) - 1 consecutive all-match groups).
//      * group task, 8 motif sizes k0..k0+7 with M(k) >= 15: a run of >= 15 matches contains an aligned
//        group of 8 rows that all match.  Per (group, k) the 8 rows of (H^H')|(L^L') are OR-ed with 16
//        v_bitop3_b32; motif sizes with M >= 23 / 39 examine only every 2nd / 4th group.
//     The answer is ONE 32-bit word per lane, task and motif size (bit b = stream b*64+lane).
//     A tile with not-ACGT positions in reach ("mixed") is scanned on the same two planes, where such a position reads
//     as A: that can only add matches, so with the flag rule relaxed to "M matching rows start in this stream" (exact)
//     and "an all-match group lies in this stream" (group) no stream that holds a row is missed; the streams that
//     consist of nothing but N are masked out (they cannot hold the start of a run).  False flags cost time only.
//  3. verify: R1 is refilled with the window of the linear planes H and L (tile - 128 .. tile + 65536 + 1536
//     positions); for every flagged (stream, k) the candidates are re-derived EXACTLY from the linear planes -- a
//     mixed tile reads the not-ACGT plane from global memory -- and each becomes a row or nothing.  A row belongs
//     to the tile that holds its first position: a run whose first examined group lies in the next tile is
//     reported by a look at the tile's end (boundary pass), and dropped by the next tile.
//  4. rows: sorted by (start, end) in LDS, written to the tile's slab as 8-byte rows.
// Exactness argument: DESIGN.md.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "prf_host.h"
#include "prf_static_for.h"
#include "scan_vertical.h"
#include "verify_impl.h"

namespace {

#include "vscan_common.h"
#include "vscan_verify.h"
#include "vscan_tasks.h"

__device__ __forceinline__ void set_prio(u32 p) {  // (s_setprio takes an immediate; p is wave-uniform)
#ifdef PRF_NO_PRIO  // (diagnostic: what the priorities and the branches that select them cost)
    return;
#endif
    if (p == 0u) __builtin_amdgcn_s_setprio(0);
    else if (p == 1u) __builtin_amdgcn_s_setprio(1);
    else if (p == 2u) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}

__device__ __forceinline__ u32 lds_add(prf_lds_u32 *p, u32 v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// 16 bytes per lane, global memory -> LDS without a register in between (LDS-DMA): lane l's 16 bytes land at lds + 16 l
__device__ __forceinline__ void dma16(const void *src_lane, u32 lds_byte_off) {
    __builtin_amdgcn_global_load_lds((prf_glb_cvoid *)src_lane, (prf_lds_void *)(prf_smem + lds_byte_off), 16, 0, 0);
}

// Grid: persistent workgroups, as many as are resident at once (or one per entry of the launch list if that is fewer):
// workgroup b takes the launch slots b, then tickets of its XCD (tiles in position order; slabs and counts are indexed by
// slot, so the order of execution does not show in the output).
// What a tile needs from HBM arrives without waiting threads: the NEXT tile's bit-sliced image is sent to R1 by LDS-DMA
// when this tile's candidates are verified (R1 is dead then) and lands while the rows are sorted; the two slots per thread
// that become the virtual lanes 64.. are ordinary loads issued at the same point and held in 8 registers.  The window of the
// linear planes follows the scan by DMA: that wait is exposed to this workgroup and covered by the five others on the CU.
template <int NC>
struct NextRegs {
    static constexpr int extra = NC - 64;
    static constexpr u32 n_extra = (u32)(2 * RG * extra);  // virtual-lane slots of a tile: (plane, row group, first lanes again)
    static_assert(n_extra <= (u32)NTH, "one virtual-lane slot per thread");
    static_assert((RG * extra) % 64 == 0, "virtual-lane staging: one plane per wave");
    prf_u32x4 ev, en;
    u32 entry;  // the launch-list entry these registers belong to

    __device__ __forceinline__ static prf_u32x4 ld16(const void *ubase, u32 byte_off) {
        return *reinterpret_cast<const prf_u32x4 *>(reinterpret_cast<const char *>(ubase) + byte_off);
    }
    // Every address is a wave-uniform base (scalar registers) plus a 32-bit per-thread offset.
    __device__ __forceinline__ void load(const prf_vscan_args &g, u32 e, int tid, int wave, u32 r1_off) {
        e = (u32)__builtin_amdgcn_readfirstlane((int)e);
        entry = e;
        const u64 tile = e & ~PRF_LAUNCH_MIXED;
        const prf_u32x4 *ph = reinterpret_cast<const prf_u32x4 *>(g.VH) + tile * (RG * 64), *pL = reinterpret_cast<const prf_u32x4 *>(g.VL) + tile * (RG * 64);
        u32 ut = (u32)tid;
        asm volatile("" : "+v"(ut));  // (opaque: keeps the address arithmetic inside the loop)
        // the image: 2 planes x 8 row groups of 1 KiB, four pieces per wave; piece (p, rg) -> slots [(p RG + rg) NC, + 64)
        {
            const u32 p = (u32)wave >> 1, rg0 = ((u32)wave & 1u) * 4u;
            const prf_u32x4 *pp = p ? pL : ph;
            const u32 l16 = (ut & 63u) * 16u;
            static_for<0, 4>([&](auto ic) {
                constexpr u32 i = (u32)decltype(ic)::value;
                dma16(reinterpret_cast<const char *>(pp) + ((rg0 + i) * 64u * 16u + l16), r1_off + ((p * RG + rg0 + i) * (u32)NC) * 16u);
            });
        }
        const prf_u32x4 z = {0, 0, 0, 0};
        ev = z;
        en = z;
        if (ut < n_extra) {
            const u32 pw = (u32)__builtin_amdgcn_readfirstlane((int)(ut / (u32)(RG * extra)));
            const u32 erg = (ut / (u32)extra) % (u32)RG, el = ut % (u32)extra;
            const u32 i0 = (erg * 64u + el) * 16u, i1 = i0 + (u32)(RG * 64) * 16u;  // the same slot of the next tile
            if (pw == 0) {
                ev = ld16(ph, i0);
                en = ld16(ph, i1);
            } else {
                ev = ld16(pL, i0);
                en = ld16(pL, i1);
            }
        }
    }
    __device__ __forceinline__ void clear() {
        const prf_u32x4 z = {0, 0, 0, 0};
        ev = en = z;
        entry = 0;
    }
    // virtual lanes 64..: the first lanes again, one bit up, bit 31 from the next tile
    __device__ __forceinline__ void store(prf_lds_u4 *vimg, int tid) const {
        const u32 sx = (u32)tid;
        if (sx < n_extra) {
            const u32 p = sx / (u32)(RG * extra), erg = (sx / (u32)extra) % (u32)RG, el = sx % (u32)extra;
            vimg[p * RG * NC + erg * (u32)NC + 64u + el] = (ev >> 1) | (en << 31);
        }
    }
};

// The phases a diagnostic build leaves out (PRF_SKIP); the constant 0 in the product, where the branches compile away
__device__ __forceinline__ u32 vscan_skip(const prf_vscan_args &g) {
#ifdef PRF_DIAG
    return g.skip;
#else
    (void)g;
    return 0u;
#endif
}

template <int NC>
__global__ __launch_bounds__(NTH, 6) void prf_vscan_kernel(prf_vscan_args g) {
    constexpr u32 R1_OFF = (u32)SMEM_HDR, R1_BYTES = (u32)(2 * RG * NC * 16);
    // (the deferred candidates' list is written while the candidates are verified, the mask of the all-N streams of a mixed tile
    // is read before its scan: they share 512 bytes)
    constexpr u32 RECS_OFF = R1_OFF + R1_BYTES, KEYS_OFF = RECS_OFF + (u32)REC_CAP * 8u, SLOW_OFF = KEYS_OFF + 2u * (u32)ROW_CAP_LDS * 4u,
                  HOTW_OFF = SLOW_OFF + (u32)SLOW_CAP * 16u, BITEMS_OFF = HOTW_OFF + (u32)FLAG_CAP * 2u;
    static_assert(SLOW_CAP * 16 >= 256, "the all-N stream masks lie in the deferred candidates' list");
    static_assert(2 * LW * 8 <= (int)R1_BYTES, "the window of the linear planes must fit the image's region");
    static_assert((2 * LW / 2 + 63) / 64 <= 5 * MAX_WAVES, "window pieces per wave");
    static_assert(LEAD_OFF == R1_OFF + 2u * (u32)LW * 8u && LEAD_OFF + 2u * LEAD_CAP * 4u <= R1_OFF + R1_BYTES, "the record waves' stream lists lie in R1 behind the window");
    prf_lds_u4 *vimg = (prf_lds_u4 *)(prf_smem + R1_OFF);
    prf_lds_u64 *recs = (prf_lds_u64 *)(prf_smem + RECS_OFF);
    prf_lds_u32 *keys = (prf_lds_u32 *)(prf_smem + KEYS_OFF);
    prf_lds_u32 *nostart = (prf_lds_u32 *)(prf_smem + SLOW_OFF);
    prf_lds_u32 *hotw = (prf_lds_u32 *)(prf_smem + HOTW_OFF);      // exact tasks: the tile's list of (stream, task) flags, 2 bytes each
    prf_lds_u32 *bitems = (prf_lds_u32 *)(prf_smem + BITEMS_OFF);  // boundary items, plan.n_group_k of them

    const int tid0 = (int)threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    // (when the launch list is one contiguous range of clean tiles -- a contig without N blocks -- the tile index is
    // arithmetic: no dependent load in front of the staging loads)
    auto entry_of = [&](u32 sl) -> u32 { return g.flat_base != ~0u ? g.flat_base + sl : g.launch_list[sl]; };

    // ---- once per workgroup ----
    set_prio(g.plan.prio & 3u);
    NextRegs<NC> sr;
    sr.load(g, entry_of(blockIdx.x), tid0, wave, R1_OFF);
    // boundary items: (motif size, examined-group stride) of every motif size a group task scans
    for (u32 v = (u32)tid0; v < 8u * g.plan.n_tasks; v += (u32)NTH) {
        const prf_vtask task = g.plan.tasks[v >> 3];
        const u32 kk = v & 7u;
        if (task.kind == 0 && ((task.valid >> kk) & 1u))
            bitems[(u32)task.item0 + (u32)__builtin_popcount((u32)task.valid & ((1u << kk) - 1u))] = ((u32)task.k0 + kk) | ((u32)task.stride << 16);
    }
    {
        prf_lds_u32 *cof_lds = bitems + g.plan.n_group_k;
        for (int i = tid0; i < (int)g.plan.cof_words; i += NTH) cof_lds[i] = prf_cof_table.v[i];
    }
    if (tid0 == 0) {  // the constant part of the tile context
        TileCtx *tcw = reinterpret_cast<TileCtx *>(prf_smem);
        tcw->H = g.H; tcw->L = g.L; tcw->X = g.X;
        tcw->E = g.E;
        tcw->slab_cap = g.slab_cap;
        tcw->min_repeats = g.min_repeats;
        tcw->min_span = g.min_span;
        tcw->lin_off = R1_OFF;
        tcw->keys_off = KEYS_OFF;
        tcw->slow_off = SLOW_OFF;
        tcw->k_exact0 = g.plan.k_exact0;
        tcw->cof_off = BITEMS_OFF + 4u * g.plan.n_group_k;
    }

    // Launch slots are handed out dynamically (tiles differ in cost by a factor of three; a fixed stride leaves the last
    // workgroups running alone for 8 % of the scan): XCD x -- the workgroups b = x mod 8 -- takes the slots = x mod 8, the
    // first one per workgroup by index, the following ones by a ticket counter of its own (one atomic per tile on eight
    // separate words; the ticket is drawn behind the tile's scan and needed at its end).
    const u32 xcd = blockIdx.x & 7u;
    const u32 first_ticket = (gridDim.x - xcd + 7u) >> 3;  // workgroups of this XCD = slots taken without a ticket
    u64 *ticket_word = g.counters + (PRF_CNT_SHARD0 + xcd * PRF_CNT_SHARD_STRIDE + PRF_SH_TILE_TICKET);
    prf_lds_u32 *next_words = (prf_lds_u32 *)(prf_smem + HDR_NEXT);  // {next slot, its launch-list entry}
    u32 slot_next = 0;
    u32 parity = 0;
    // (thread 0) candidates looked at by this workgroup, and those verified on the spot by the general routine because a list was
    // full: ONE atomic each when the workgroup ends.  Kept in LDS: as registers they lived in scratch memory across the tile
    // loop -- two scratch loads and two stores per tile in front of wave 0's verification.
    prf_lds_u32 *wg_stats = (prf_lds_u32 *)(prf_smem + HDR_STATS);
    if (tid0 == 0) wg_stats[0] = wg_stats[1] = 0;
    for (u32 slot = blockIdx.x; slot < g.n_launch; slot = slot_next, parity ^= 1u) {
    // (opaque per round: what derives from the thread index is recomputed, not carried through the scan's calls in
    // registers that would have to be spilled)
    int wave_s = wave;
    asm volatile("" : "+s"(wave_s));  // (opaque: recomputed from a scalar and the hardware's lane index, two operations)
    u32 ones = ~0u;
    asm volatile("" : "+s"(ones));  // (opaque too: the lane index is not to be computed once and kept in scratch memory either)
    int tid = wave_s * 64 + (int)__builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const u32 entry = sr.entry;
    const bool hasx = (entry & PRF_LAUNCH_MIXED) != 0;
    const u64 tile = entry & ~PRF_LAUNCH_MIXED;
    prf_lds_u32 *cnt = smem_cnt(parity);

    PRF_STAMP(0);
#ifdef PRF_STAMPS
    if (g.dbg && lane == 0) g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + 12] = __builtin_amdgcn_s_memrealtime();  // 100 MHz, chip-wide
#endif
    // ---- 1. stage: the image is in R1 (DMA issued during the previous tile's rows phase, or above); the virtual lanes from
    // the two prefetched slots; a mixed tile's mask of the streams that hold nothing but N ----
    set_prio(g.plan.prio & 3u);
    {
        sr.store(vimg, tid);
        if (hasx && tid < 64) {
            // bit b = stream (b, lane) is all N: its 32 positions are one aligned dword of the LINEAR not-ACGT plane (round 3: the
            // bit-sliced copy of that plane existed for this mask alone -- 0.125 B per position of HBM; mixed tiles are rare)
            const u32 *px = reinterpret_cast<const u32 *>(g.X + tile * PRF_TILE_WORDS);
            u32 m = 0;
#pragma unroll 1
            for (u32 b0 = 0; b0 < 32u; b0 += 8u) {  // (eight loads in flight: the registers of 32 would be spilled around this block)
                u32 v[8];
                static_for<0, 8>([&](auto bc) { v[decltype(bc)::value] = *(prf_glb_cu32 *)(px + ((b0 + (u32)decltype(bc)::value) * 64u + (u32)tid)); });
                static_for<0, 8>([&](auto bc) { m |= (v[decltype(bc)::value] == ~0u ? 1u : 0u) << (b0 + (u32)decltype(bc)::value); });
            }
            nostart[tid] = m;
        }
        if (tid < (int)CNT_N) cnt[tid] = 0;  // rows, records, flags, ... (the other set is still read by slow waves)
        if (tid == 0) {  // the tile's part of the context (the rest was written once, above)
            TileCtx *tcw = reinterpret_cast<TileCtx *>(prf_smem);
            tcw->w0 = tile * PRF_TILE_WORDS - LIN_PRE;
            tcw->xz_lo = hasx ? 0 : tile * PRF_TILE;  // a clean tile and its successor hold no not-ACGT position
            tcw->xz_hi = hasx ? 0 : (tile + 2) * PRF_TILE;
            tcw->slab = (prf_glb_u64 *)(g.slabs + (u64)slot * g.slab_cap);
            tcw->tile_base = tile * PRF_TILE;
            tcw->has_lin = 0u;
            tcw->cnt_off = (u32)HDR_CNT + 4u * CNT_N * parity;
        }
    }
    PRF_STAMP(1);
    __syncthreads();  // (waits for the image's DMA too)
    PRF_STAMP(2);

    // ---- 2. scan ----
    set_prio(((g.plan.slack_waves >> wave) & 1u) ? (g.plan.prio >> 4) & 3u : (g.plan.prio >> 2) & 3u);
    Emit em;
    em.recs = recs;
    em.cnt = cnt;
    em.lane = lane;
#ifdef PRF_STAMPS
    u64 *task_dbg = g.dbg ? g.dbg + ((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS : nullptr;
#else
    u64 *task_dbg = nullptr;
#endif
    {
        u32 allow = hasx ? ~nostart[lane] : ~0u;
        if (vscan_skip(g) & 1u) allow = 0u;  // (diagnostic, PRF_SKIP: no flags, no records)
        run_tasks<NC>((prf_lds_cu4 *)vimg, hotw, nostart, g.plan, wave, lane, hasx, allow, em, task_dbg);  // (nostart: free on a clean tile)
    }
    PRF_STAMP(17);  // the wave's arrival: the end of its last task
    // From here to the second barrier -- arrival, window loads, window stores, pad loop, counters -- every wave of the workgroup waits
    // for the last one: the shortest and most latency-bound stretch of the tile has a priority of its own (at the scan's it
    // competed, at the lowest, with five other workgroups' scans).
    set_prio((g.plan.prio >> 12) & 3u);
    // ---- 3a. R1 <- the window of the linear planes H and L (tile - 128 .. tile + 65536 + 1536 positions), in 16-byte units: unit
    // u < LW/2 is H's word pair u, the others L's; piece = 64 units = 1 KiB.  R1 is the image until the LAST wave has finished its
    // tasks, so the window cannot be sent there earlier -- but the waves do not finish together (the plan's deal sees to that): the first
    // two to arrive load the window into registers (9 and 8 pieces: 36 / 32 VGPRs, free at this point) while they would
    // otherwise wait at the barrier, and store it behind the barrier.  The first version sent it by DMA behind the barrier: 2 - 4 k
    // cycles of HBM latency with every wave waiting.
    constexpr u32 WIN_UNITS = (u32)LW;  // 2 planes x LW / 2
    constexpr u32 WIN_PIECES = (WIN_UNITS + 63u) / 64u;
    static_assert(WIN_PIECES == 17, "the window's pieces are dealt 9 + 8 to the first two waves to arrive");
    prf_u32x4 wv[9];
    u32 order = 0;
    {
        if (lane == 0) order = atomicAdd((u32 *)(cnt + CNT_ROWS0), 1u);  // (the counter is free until the barrier: arrival order)
        order = (u32)__builtin_amdgcn_readfirstlane((int)order);
#ifdef PRF_STAMPS
        if (g.dbg && lane == 0) g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + 18] = order;
#endif
        const long long w0 = (long long)(tile * PRF_TILE_WORDS) - LIN_PRE;
        const u64 *wh = g.H + w0, *wl = g.L + w0;
        // (the window registers are defined without an instruction: zeroed, every wave ran 36 v_mov_b32 here -- the two that load
        // nothing as well -- in the stretch where all four are late; the stores behind the barrier sit under the loads' condition)
        asm("" : "=v"(wv[0]), "=v"(wv[1]), "=v"(wv[2]), "=v"(wv[3]), "=v"(wv[4]), "=v"(wv[5]), "=v"(wv[6]), "=v"(wv[7]), "=v"(wv[8]));
        if (order < 2u) {
            const u32 first = order * 9u, n = order ? 8u : 9u;
            static_for<0, 9>([&](auto ic) {
                constexpr u32 i = (u32)decltype(ic)::value;
                if (i < n) {  // wave-uniform
                    const u32 u = (first + i) * 64u + (u32)lane;
                    const u64 *src = u < (u32)LW / 2u ? wh + 2u * u : wl + 2u * (u - (u32)LW / 2u);
                    if (u < WIN_UNITS) wv[i] = *reinterpret_cast<const prf_u32x4 *>(src);
                }
            });
        }
    }
    // The ticket for the tile after this one is drawn by the wave that leaves the scan first, behind its window loads: it waits for
    // those at the barrier below anyway, and the atomic's round trip is no longer than theirs.  (Drawn at the top of the tile -- the
    // first version -- the value was waited for at once all the same: a function waits for every outstanding memory operation on
    // entry, and the first task is a call; kept across the tasks' calls it lived in scratch memory.  Drawn behind the scan by a
    // fixed thread it was waited for on the spot as well, by a wave with work to do.)
    u64 ticket = 0;
    const bool ticket_thread = order == 0u && lane == 0;
    if (ticket_thread) ticket = atomicAdd(ticket_word, 1ull);
#ifdef PRF_STAMPS
    {
        // (stamps build only) slot 3: the arrival atomic is back and the window loads are issued; slot 20: the loads are in
        // registers.  The loading waves wait for them HERE, where they would wait at the barrier anyway -- the product waits
        // behind the barrier, in front of the stores -- so that the loads' latency is measured whether it is exposed or not;
        // both clocks are read before either is stored (a stamp's store would be waited for with the loads).
        const u64 t3 = __builtin_amdgcn_s_memtime();
        if (order < 2u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 t20 = __builtin_amdgcn_s_memtime();
        if (g.dbg && lane == 0) {
            g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + 3] = t3;
            g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + 20] = t20;
        }
    }
#endif
    __syncthreads();  // the image is dead from here on
    PRF_STAMP(19);
    {
        if (order < 2u) {
            const u32 first = order * 9u, n = order ? 8u : 9u;
            static_for<0, 9>([&](auto ic) {
                constexpr u32 i = (u32)decltype(ic)::value;
                if (i < n) {
                    const u32 u = (first + i) * 64u + (u32)lane;
                    if (u < WIN_UNITS) *(prf_lds_u4 *)(prf_smem + R1_OFF + 16u * u) = wv[i];
                }
            });
        }
        PRF_STAMP(21);
        // every sublist is padded to its capacity with the largest key of its quarter: no bounds test per key when the rows are
        // ranked (rows that the scan's overflow paths have listed already stay; the verification appends behind them)
        const prf_u32x4 n0 = *(prf_lds_cu4 *)(cnt + CNT_ROWS);
        for (u32 i = (u32)tid; i < (u32)ROW_CAP_LDS; i += (u32)NTH) {
            const u32 q = i / (u32)QCAP, j = i - q * (u32)QCAP;
            const u32 n0q = q == 0u ? n0.x : (q == 1u ? n0.y : (q == 2u ? n0.z : n0.w));
            if (j >= n0q) keys[i] = quarter_pad(q);
        }
        if (tid == 0) {
            reinterpret_cast<TileCtx *>(prf_smem)->has_lin = 1u;
            cnt[CNT_ROWS0] = n0.x;
            cnt[CNT_ROWS0 + 1u] = n0.y;
            cnt[CNT_ROWS0 + 2u] = n0.z;
            cnt[CNT_ROWS0 + 3u] = n0.w;
            cnt[CNT_OVF0] = cnt[CNT_OVF];
            cnt[CNT_LONG0] = cnt[CNT_LONG];
        }
        PRF_STAMP(22);
    }
    // The next launch slot's entry (a load from the launch list unless the list is one run of clean tiles): issued here by the
    // thread that drew the ticket, looked at behind the verification.
    u32 slot_pre = 0, entry_pre = entry;
    if (ticket_thread) {
        slot_pre = (first_ticket + (u32)ticket) * 8u + xcd;
        if (slot_pre < g.n_launch) entry_pre = entry_of(slot_pre);  // (last round: this tile again, unused)
    }
    __syncthreads();
    PRF_STAMP(4);

    // ---- 3b. verify, all waves together: every candidate -> a row in the tile's list, or nothing ----
    // (wave 0's flags are the longest leg of this phase since the echoes went, the record waves follow: both kinds have a priority
    // field of their own)
    set_prio(wave < MAX_WAVES / 2 ? (g.plan.prio >> 6) & 3u : (g.plan.prio >> 8) & 3u);
    const u32 *xw = hasx ? reinterpret_cast<const u32 *>(g.X + ((long long)(tile * PRF_TILE_WORDS) - LIN_PRE)) : nullptr;
    typedef const unsigned short __attribute__((address_space(3))) prf_lds_cu16;
    u32 n_recs = cnt[CNT_RECS], n_flags = cnt[CNT_FLAGS];
    {
        if (tid == 0) {
            // statistics: candidates looked at = (stream, exact task) flags + group-task records (+ those verified on the spot)
            const u32 early = cnt[CNT_EARLY];
            wg_stats[0] += n_flags + n_recs + early;
            wg_stats[1] += early;
        }
        n_recs = n_recs < (u32)REC_CAP ? n_recs : (u32)REC_CAP;
        n_flags = n_flags < (u32)FLAG_CAP ? n_flags : (u32)FLAG_CAP;
#ifdef PRF_STAMPS
        if (g.dbg && tid == 0) g.dbg[((u64)slot * MAX_WAVES + 0) * PRF_STAMP_SLOTS + 23] = (u64)n_flags | ((u64)n_recs << 32);
#endif
        if (vscan_skip(g) & 2u) n_flags = 0;   // (diagnostic) the flags are listed but not verified
        if (vscan_skip(g) & 4u) n_recs = 0;    // (diagnostic) the same for the records
        verify_all((prf_lds_cu64 *)recs, n_recs, (prf_lds_cu32 *)bitems, (vscan_skip(g) & 8u) ? 0u : g.plan.n_group_k, (prf_lds_cu16 *)hotw, n_flags, xw, (u32)tid, task_dbg);
    }
    set_prio((g.plan.prio >> 10) & 3u);
    if (ticket_thread) {  // the next slot and its entry, for everybody behind the barrier
        next_words[0] = slot_pre;
        next_words[1] = entry_pre;
    }
    PRF_STAMP(5);
    __syncthreads();
    {
        // the candidates that could not be finished inside the window (rare: wave-uniform, read behind the barrier)
        const u32 n_slow = (u32)__builtin_amdgcn_readfirstlane((int)cnt[CNT_SLOW]);
        if (n_slow) {
            if (n_slow <= (u32)SLOW_CAP) {
                if ((u32)tid < n_slow) {
                    prf_lds_u64 *slow = (prf_lds_u64 *)(prf_smem + SLOW_OFF);
                    slow_item(slow[2u * (u32)tid], slow[2u * (u32)tid + 1u]);
                }
            } else {
                // more than the list holds: the tile's rows so far are dropped, the general routine does everything again
                if (tid == 0) {
                    for (u32 q = 0; q < 4u; q++) cnt[CNT_ROWS + q] = cnt[CNT_ROWS0 + q];
                    cnt[CNT_OVF] = cnt[CNT_OVF0];
                    cnt[CNT_LONG] = cnt[CNT_LONG0];
                }
                __syncthreads();
                verify_general((prf_lds_cu64 *)recs, n_recs, (prf_lds_cu32 *)bitems, g.plan.n_group_k, (prf_lds_cu16 *)hotw, n_flags, (u32)tid);
            }
            __syncthreads();
        }
    }
    // the window is dead from here on
    PRF_STAMP(6);
    const u64 nw = *(prf_lds_u64 *)next_words;  // (one read)
    slot_next = (u32)__builtin_amdgcn_readfirstlane((int)(u32)nw);
    const u32 entry_next = (u32)(nw >> 32);
    // rows per quarter of the tile (those behind a sublist's capacity included), wave-uniform; the tile's rows are their sum
    u32 nq0, nq1, nq2, nq3;
    {
        const prf_u32x4 c = *(prf_lds_cu4 *)(cnt + CNT_ROWS);
        const bool none = (vscan_skip(g) & 16u) != 0;  // (diagnostic: rows counted as none)
        nq0 = none ? 0u : (u32)__builtin_amdgcn_readfirstlane((int)c.x);
        nq1 = none ? 0u : (u32)__builtin_amdgcn_readfirstlane((int)c.y);
        nq2 = none ? 0u : (u32)__builtin_amdgcn_readfirstlane((int)c.z);
        nq3 = none ? 0u : (u32)__builtin_amdgcn_readfirstlane((int)c.w);
    }
    const u32 n_rows = nq0 + nq1 + nq2 + nq3;
    const bool dense = nq0 > (u32)QCAP || nq1 > (u32)QCAP || nq2 > (u32)QCAP || nq3 > (u32)QCAP;  // a sublist is full: rows in the slab
    const u32 n_long = (u32)__builtin_amdgcn_readfirstlane((int)cnt[CNT_LONG]);
    u64 *slab = g.slabs + (u64)slot * g.slab_cap;
    const u32 n_store = n_rows < g.slab_cap ? n_rows : g.slab_cap;
    bool unsorted = false;
    // The tile's row count, and its share of the sum the gather kernel starts from, leave NOW: a device-scope atomic stays
    // outstanding for ~3 k cycles when every CU issues them, and the tile's last barrier waits for it.  Issued behind the
    // ranking (first version) that wait was exposed: 7 % of the scan on the default workload, 27 % on random sequence
    // (PRF_SKIP=32, profiles/r03_notes.md); here it hides behind the rows phase.  ONE atomic per tile (the second level of sums
    // is gone: the gather adds the first level up itself).
    if (tid == 0) {
        g.slab_count[slot] = n_rows;
        if (n_store && !(vscan_skip(g) & 32u)) atomicAdd(&g.block_sum[slot >> g.gather_shift], n_store);
    }

    // ---- 4. the tile's rows, sorted by (start, end), into its slab.  Rank of a row = number of rows with a smaller key; keys
    // are distinct ((start, end) pairs never collide between motif sizes).
    if (dense) {
        // A dense tile -- a quarter with more rows than its sublist holds (the reference's golden chr22 BED has tiles of 750
        // rows): the rows behind the sublists went to the slab, from its first slot on, as they came.  All rows are collected in R1
        // -- the window is dead -- grouped by quarter: the four counts give every quarter's region, the rows read back from the slab
        // find their place in it with an LDS add.  A row is ranked against the 16-byte units that overlap its quarter's region:
        // every key in front of them is smaller; of the neighbours' keys inside them those of the lower quarter are smaller and
        // are counted, those of the higher one are not.
        constexpr u32 R1_ROWS = R1_BYTES / 8u;
        const u32 m0 = nq0 < (u32)QCAP ? nq0 : (u32)QCAP, m1 = nq1 < (u32)QCAP ? nq1 : (u32)QCAP, m2 = nq2 < (u32)QCAP ? nq2 : (u32)QCAP,
                  m3 = nq3 < (u32)QCAP ? nq3 : (u32)QCAP;
        const u32 n_ovf = n_rows - (m0 + m1 + m2 + m3);  // (= cnt[CNT_OVF])
        const u32 s1 = nq0, s2 = nq0 + nq1, s3 = s2 + nq2;  // first row of the quarters' regions
        auto pick = [](u32 q, u32 a0, u32 a1, u32 a2, u32 a3) -> u32 { return q == 0u ? a0 : (q == 1u ? a1 : (q == 2u ? a2 : a3)); };
        if (n_rows <= g.slab_cap && n_rows <= R1_ROWS) {
            prf_lds_u32 *k2 = (prf_lds_u32 *)(prf_smem + R1_OFF), *v2 = k2 + R1_ROWS;
            prf_lds_u32 *fill = cnt + CNT_ROWS0;  // (free from here on) rows placed in each region so far
            if (tid < 4) fill[tid] = pick((u32)tid, m0, m1, m2, m3);
            for (u32 i = (u32)tid; i < (u32)ROW_CAP_LDS; i += (u32)NTH) {
                const u32 q = i / (u32)QCAP, j = i - q * (u32)QCAP;
                if (j < pick(q, m0, m1, m2, m3)) {
                    const u32 at = pick(q, 0u, s1, s2, s3) + j;
                    k2[at] = keys[i];
                    v2[at] = keys[ROW_CAP_LDS + i];
                }
            }
            __syncthreads();
            for (u32 i = (u32)tid; i < n_ovf; i += (u32)NTH) {
                const u64 r = slab[i];
                const u32 q = (u32)r >> 30;
                const u32 at = pick(q, 0u, s1, s2, s3) + atomicAdd((u32 *)(fill + q), 1u);  // (< the region's end: the quarter's count holds these rows)
                k2[at] = (u32)r;
                v2[at] = (u32)(r >> 32);
            }
            for (u32 i = n_rows + (u32)tid; i < ((n_rows + 3u) & ~3u); i += (u32)NTH) k2[i] = 0xFFFFFFFFu;
            __syncthreads();  // (the slab's first slots have been read: the ranked rows may go there)
            typedef __attribute__((address_space(3))) const prf_u32x4 prf_lds_ckey4;
            prf_lds_ckey4 *k4 = (prf_lds_ckey4 *)k2;
            for (u32 r = (u32)tid; r < n_rows; r += (u32)NTH) {
                const u32 mine = k2[r], kv = v2[r];
                const u32 q = mine >> 30;
                const u32 lo = pick(q, 0u, s1, s2, s3), hi = lo + pick(q, nq0, nq1, nq2, nq3);
                const u32 u_lo = lo >> 2, u_hi = (hi + 3u) >> 2;
                u32 rank = 4u * u_lo;
#pragma unroll 4
                for (u32 u = u_lo; u < u_hi; u++) {
                    const prf_u32x4 v = k4[u];
                    rank += (v.x < mine ? 1u : 0u) + (v.y < mine ? 1u : 0u) + (v.z < mine ? 1u : 0u) + (v.w < mine ? 1u : 0u);
                }
                slab[rank] = (u64)mine | ((u64)kv << 32);
            }
            __syncthreads();  // R1 is refilled below
        } else {
            // more rows than R1 or the slab holds (no genome does the first; the host repeats the scan with larger slabs after the
            // second): the sublists go to the slab as they are, behind the rows that are there; the host sorts
            for (u32 i = (u32)tid; i < (u32)ROW_CAP_LDS; i += (u32)NTH) {
                const u32 q = i / (u32)QCAP, j = i - q * (u32)QCAP;
                const u32 at = n_ovf + pick(q, 0u, m0, m0 + m1, m0 + m1 + m2) + j;
                if (j < pick(q, m0, m1, m2, m3) && at < g.slab_cap) slab[at] = (u64)keys[i] | ((u64)keys[ROW_CAP_LDS + i] << 32);
            }
            unsorted = true;
        }
    }

    // the next tile's staging data: the image's DMA and the virtual lanes' loads are issued now and land while the rows are ranked
    // (every register is written on both paths: dead from the stage to here, not carried around the loop)
    if (slot_next < g.n_launch) sr.load(g, entry_next, tid, wave, R1_OFF);
    else sr.clear();

    PRF_RANK_DECL();
    {
        // Wave w ranks sublist w: rows of different quarters are never compared, a row's place in the slab is the number of rows
        // in the lower quarters plus its rank among its own.  P = 1, 2 or 4 adjacent lanes per row (the largest power of two
        // <= 64 / n; more than four would leave a lane less than one batch): lane `part` of a row reads the 16-byte units part,
        // part + P, ... of the sublist, four in flight (two at the sublist's tail), and the P shares are added up with DPP moves.  More than 64 rows in
        // the quarter: two passes.  Dependent LDS round trips are what this phase costs: the row's own key and motif size and the
        // first batch of keys are ONE batch of reads.
        // Smaller-than without the carry flag (a compare and an add through vcc stall on each other, one s_nop per key): two keys
        // of one sublist agree in their top two bits, so the sign of their difference is the answer; v_alignbit shifts it into a
        // word of verdicts that is counted once per batch.  (Sublists are padded with the largest key of their quarter.)
        // No read leaves the sublist: a batch starts below its ceil(n / 4) <= QCAP / 4 units and spans at most 4 P of them, and
        // what follows the last sublist are the motif-size words, which must not be counted.
        const u32 nq = wave_s == 0 ? nq0 : (wave_s == 1 ? nq1 : (wave_s == 2 ? nq2 : nq3));
        const u32 below = wave_s == 0 ? 0u : (wave_s == 1 ? nq0 : (wave_s == 2 ? nq0 + nq1 : nq0 + nq1 + nq2));
        if (nq && !dense) {
            const u32 lg = nq > 32u ? 0u : (nq > 16u ? 1u : 2u);
            const u32 P = 1u << lg, part = (u32)lane & (P - 1u);
            const u32 units = (nq + 3u) >> 2;
            prf_lds_u32 *sub = keys + (u32)wave_s * (u32)QCAP;
            typedef __attribute__((address_space(3))) const prf_u32x4 prf_lds_ckey4;
            prf_lds_ckey4 *k4 = (prf_lds_ckey4 *)sub + part;
            for (u32 row0 = 0; row0 < nq; row0 += 64u >> lg) {
                const u32 row = row0 + ((u32)lane >> lg);
                const u32 r = row < nq ? row : 0u;  // (lanes without a row read row 0: harmless)
                PRF_RANK_T0();
                const u32 mine = sub[r];
                const u32 kv = sub[ROW_CAP_LDS + r];
                u32 rank = 0;
                auto batch = [&](u32 u0, auto nc) {  // N reads in flight, then 2 operations per key and one count
                    constexpr u32 N = (u32)decltype(nc)::value;
                    prf_u32x4 v[N];
                    static_for<0, (int)N>([&](auto jc) { v[decltype(jc)::value] = k4[u0 + (u32)decltype(jc)::value * P]; });
                    // (all reads in flight before the first difference: left alone the compiler issues them two at a time)
                    if constexpr (N == 4u) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
                    else asm volatile("" : "+v"(v[0]), "+v"(v[1]));
                    u32 bits = 0;
                    static_for<0, (int)N>([&](auto jc) {
                        constexpr u32 j = (u32)decltype(jc)::value;
                        bits = __builtin_amdgcn_alignbit(bits, v[j].x - mine, 31);
                        bits = __builtin_amdgcn_alignbit(bits, v[j].y - mine, 31);
                        bits = __builtin_amdgcn_alignbit(bits, v[j].z - mine, 31);
                        bits = __builtin_amdgcn_alignbit(bits, v[j].w - mine, 31);
                    });
                    rank += (u32)__builtin_popcount(bits);
                };
                for (u32 u0 = 0; u0 < units; u0 += 4u * P) {  // (wave-uniform: scalar branches)
                    if (units - u0 > 2u * P) batch(u0, std::integral_constant<u32, 4>{});
                    else batch(u0, std::integral_constant<u32, 2>{});  // (the sublist's tail: one or two reads per lane are left)
                }
                // sum over the P adjacent lanes of a row (wave-uniform P): xor 1, xor 2 by quad permutes
                if (P >= 2u) rank += (u32)__builtin_amdgcn_update_dpp(0, (int)rank, 0xB1, 0xF, 0xF, true);
                if (P >= 4u) rank += (u32)__builtin_amdgcn_update_dpp(0, (int)rank, 0x4E, 0xF, 0xF, true);
                PRF_RANK_T1(rank);
                rank += below;
                if (row < nq && part == 0 && rank < g.slab_cap && !(vscan_skip(g) & 64u)) slab[rank] = (u64)mine | ((u64)kv << 32);
            }
        }
    }
    if ((u32)tid < n_long && (u32)tid < PRF_LONG_PER_TILE)
        g.long_ends[(u64)slot * PRF_LONG_PER_TILE + (u32)tid] = ((prf_lds_u64 *)(prf_smem + HDR_LONG))[tid];
    if (tid == 0) {
        if (n_rows > g.slab_cap) atomicMax(&g.counters[PRF_CNT_HIT_OVF], (u64)n_rows);
        if (unsorted) atomicMax(&g.counters[PRF_CNT_UNSORTED], 1ull);
        if (n_long > PRF_LONG_PER_TILE) atomicMax(&g.counters[PRF_CNT_LONG_OVF], (u64)n_long);
    }
    PRF_STAMP(7);
    PRF_RANK_STORE();
#ifdef PRF_STAMPS
    if (g.dbg && lane == 0) g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + 13] = __builtin_amdgcn_s_memrealtime();
#endif
    // (no barrier here: the next round's first barrier separates this tile's reads of the row list from the next tile's writes)
    }
    if (tid0 == 0) {
        const u64 cand_total = wg_stats[0], early_total = wg_stats[1];
        if (cand_total) atomicAdd(&g.counters[PRF_CNT_SHARD0 + (blockIdx.x % PRF_CNT_NSHARD) * PRF_CNT_SHARD_STRIDE + PRF_SH_CAND], cand_total);
        if (early_total) atomicAdd(&g.counters[PRF_CNT_SHARD0 + (blockIdx.x % PRF_CNT_NSHARD) * PRF_CNT_SHARD_STRIDE + PRF_SH_EARLY], early_total);
    }
}

}  // namespace

// persistent workgroups: as many as are resident at once (LDS- and register-bound: 6 per CU at most)
static u32 resident_per_cu(u32 nc, u32 lds) {
    int n = 0;
    hipError_t e = nc == 72 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, prf_vscan_kernel<72>, NTH, lds)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, prf_vscan_kernel<80>, NTH, lds);
    if (e != hipSuccess || n < 1) {
        (void)hipGetLastError();
        n = (int)std::max(1u, (160u * 1024u) / std::max(1u, lds + 1280u));
    }
    // (MI355X_MICROARCH.md: 256-thread workgroups are admitted up to floor(800 / (ceil(sgpr / 16) * 16 + 16)) per CU, which the
    // API overstates by one for 81 .. 112 SGPRs; the kernel is built for six.  A grid larger than what is resident is harmless
    // here -- no workgroup ever waits for another -- it only makes the launch slots taken "by index" start late.)
    return (u32)std::min(n, 6);
}

hipError_t prf_vertical_launch(hipStream_t s, const prf_vscan_args &args) {
    if (args.n_launch == 0) return hipSuccess;
    u32 lds = args.plan.lds_bytes;
#ifdef PRF_DIAG
    // PRF_LDS_PAD: extra dynamic LDS per workgroup, to measure the scan at a lower occupancy
    static const u32 lds_pad = getenv("PRF_LDS_PAD") ? (u32)atoi(getenv("PRF_LDS_PAD")) : 0u;
    lds += lds_pad;
#endif
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return hipErrorInvalidDevice;
        n_cu = prop.multiProcessorCount;
    }
    static u32 cache_lds = ~0u, cache_nc = 0, cache_per_cu = 0;
    if (cache_lds != lds || cache_nc != args.plan.nc) {
        cache_per_cu = resident_per_cu(args.plan.nc, lds);
        cache_lds = lds;
        cache_nc = args.plan.nc;
#ifdef PRF_DIAG
        if (getenv("PRF_DEBUG")) fprintf(stderr, "[prf] fused kernel: nc %u, %u bytes of LDS, %u workgroups per CU\n", args.plan.nc, lds, cache_per_cu);
#endif
    }
    const dim3 grid(std::min(args.n_launch, cache_per_cu * (u32)n_cu)), block(NTH);
    switch (args.plan.nc) {
        case 72: hipLaunchKernelGGL((prf_vscan_kernel<72>), grid, block, lds, s, args); break;
        case 80: hipLaunchKernelGGL((prf_vscan_kernel<80>), grid, block, lds, s, args); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
