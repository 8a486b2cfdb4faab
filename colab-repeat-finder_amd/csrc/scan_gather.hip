// scan_gather.hip -- the row gather that follows the fused scan kernel (scan_vertical.hip).
//
// A second, small kernel (prf_vgather_kernel) concatenates the slabs in launch (= position) order and expands the
// rows to 24 bytes: the row array leaves the device sorted by (contig, start, end), which is what the reference's
// sorted() returns (reference perfect_repeat_finder.py:81).
#include "prf_host.h"
#include "prf_static_for.h"
#include "scan_vertical.h"

namespace {

// Row gather: the slabs (8-byte rows, sorted per tile), in launch (= position) order, become ONE compact array of 24-byte
// rows.  Workgroup w owns the launch slots [w << shift, (w + 1) << shift).  The scan kernel adds each tile's stored rows to
// block_sum[its gather workgroup] (ONE atomic per tile); workgroup w adds up the sums of the workgroups 0 .. w-1 itself
// (four independent loads per thread and pass) to find where its rows begin, scans its own slots' counts, and writes its
// rows in rounds of 256: a thread decodes one row into three words in LDS, then the round's words leave as coalesced
// 16-byte stores; the slab rows of eight rounds are fetched in one batch.
// The workgroup that finishes last hands the counter block to the host (mapped memory, no copy call), and clears the sums
// and the counter block of the next scan (no memset call).
__global__ __launch_bounds__(256) void prf_vgather_kernel(prf_vgather_args g) {
    __shared__ u64 part[4];
    __shared__ u32 offs[PRF_GATHER_SLOTS_MAX + 1];   // in rows
    __shared__ u64 tbase[PRF_GATHER_SLOTS_MAX];      // first position of the slot's tile
    __shared__ u64 cbase[PRF_GATHER_SLOTS_MAX];      // first position of its contig
    __shared__ u32 contig[PRF_GATHER_SLOTS_MAX];
    __shared__ u64 ticket_lds;
    __shared__ u64 stage[2 * 3 * 256];
    __shared__ u32 fix_n;                                               // rows whose span is clipped: their true ends are filled in
    __shared__ u64 fix[PRF_GATHER_SLOTS_MAX * PRF_LONG_PER_TILE];       // behind the copy (row | slot << 32 | index of the end << 40)
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 n_slots = 1u << g.gather_shift;  // launch slots per workgroup: 8 (small launches: more workgroups) .. 64
    const u32 first = blockIdx.x << g.gather_shift;
    const u32 my_super = blockIdx.x / PRF_GATHER_SUPER;
    // The loads of the prologue are issued together: the slots' counts and tiles (-> tile table), then the sums of the workgroups
    // in front of this one.  (One after the other they were five to six L2 round trips before the first row moved.)
    const bool live = tid < n_slots && first + tid < g.n_launch;  // (n_slots <= 64: the first wave)
    u32 c = 0;
    uint4 ti = make_uint4(0, 0, 0, 0);
    u64 tile = 0;
    if (live) {
        c = g.slab_count[first + tid];
        tile = (g.flat_base != ~0u ? g.flat_base + first + tid : g.launch_list[first + tid]) & ~PRF_LAUNCH_MIXED;
        ti = g.tile_info[tile];
    }
    u64 before = 0;  // rows in front of this workgroup's slots: the sums of the workgroups before it (one atomic per tile in the scan)
    for (u32 i = tid; i < blockIdx.x; i += 1024u) {  // (four independent loads per pass)
        u32 v[4];
#pragma unroll
        for (u32 u = 0; u < 4u; u++) v[u] = i + 256u * u < blockIdx.x ? g.block_sum[i + 256u * u] : 0u;
        before += (u64)v[0] + v[1] + v[2] + v[3];
    }
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) part[wave] = before;
    if (tid == 0) fix_n = 0;
    if (tid < 64u) {  // exclusive scan of the counts, the slots' tiles and contigs
        c = c < g.slab_cap ? c : g.slab_cap;
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 up = __shfl_up(incl, o, 64);
            if ((int)tid >= o) incl += up;
        }
        offs[tid + 1] = incl;
        if (tid == 0) offs[0] = 0;
        if (live) {
            tbase[tid] = tile * PRF_TILE;
            cbase[tid] = (u64)ti.z | ((u64)ti.w << 32);
            contig[tid] = ti.x;
        }
    }
    __syncthreads();
    const u64 base0 = part[0] + part[1] + part[2] + part[3];  // rows in front of this workgroup's slots
    const u32 n_mine = offs[n_slots];
    // rows beyond the capacity stay behind: the host sees the total beyond the capacity, grows the array, rescans
    const u64 room_rows = base0 < g.rows_cap ? g.rows_cap - base0 : 0;
    const u32 n_copy = (u64)n_mine < room_rows ? n_mine : (u32)room_rows;  // rows
    u64 *dst = reinterpret_cast<u64 *>(g.rows + base0);
    // 256 rows per round: thread t decodes row r0 + t into three words in LDS, then the 768 words leave as coalesced stores; two
    // staging buffers used alternately, one barrier per round.  The slab rows of EIGHT rounds are fetched (slot search + load) in
    // one batch in front of them.  gfx950 counts loads and stores on ONE counter, in issue order (MI355X_MICROARCH.md), so a load's
    // data waits for every store issued before it -- and the compiler, once loads and stores are both in flight, waits for all of
    // them (vmcnt(0)): with a fetch per round every round ended with a full write round trip.  Now a workgroup waits for memory
    // once per eight rounds.  It bought 2 us of 49 on the default workload and costs 7 of 54 on ONE 10 Gbp sequence (a
    // workgroup with two rounds of rows still searches for eight): the kernel moves 183 MB in its 47 us, of which ~22 us do
    // not depend on the row count (profiles/r03_notes.md 2b).  (The rounds' barrier orders LDS only: s_waitcnt lgkmcnt(0) +
    // s_barrier -- which is also all that __syncthreads() is on this target.)
    constexpr u32 DEPTH = 8;
    u32 buf = 0;
    for (u32 R = 0; R < n_copy; R += DEPTH * 256u) {  // (n_copy is uniform: every thread takes the same barriers)
        u64 sr[DEPTH];
        u32 los[DEPTH];
        static_for<0, (int)DEPTH>([&](auto jc) {
            constexpr u32 j = (u32)decltype(jc)::value;
            const u32 row = R + j * 256u + tid;
            u32 lo = 0, hi = n_slots;  // the slot that holds the row: offs[lo] <= row < offs[lo + 1]
            while (hi - lo > 1) {
                const u32 mid = (lo + hi) >> 1;
                if (offs[mid] <= row) lo = mid; else hi = mid;
            }
            los[j] = lo;
            sr[j] = row < n_copy ? g.slabs[(u64)(first + lo) * g.slab_cap + (row - offs[lo])] : 0ull;
        });
        // (the ONE wait for memory of the eight rounds, outside their divergent blocks: a wait inside a block that a wave may skip
        // does not count behind it, and the compiler would wait again -- for every store issued since -- in each round)
        static_for<0, (int)DEPTH>([&](auto jc) {
            u64 &x = sr[decltype(jc)::value];
            asm volatile("" : "+v"(x));
        });
        static_for<0, (int)DEPTH>([&](auto jc) {
            constexpr u32 j = (u32)decltype(jc)::value;
            const u32 r0 = R + j * 256u;
            if (r0 < n_copy) {
                u64 *st = stage + buf * 768u;
                if (r0 + tid < n_copy) {
                    const u32 lo = los[j];
                    const u32 key = (u32)sr[j], kv = (u32)(sr[j] >> 32);
                    const u64 start = tbase[lo] + (key >> 16);
                    const u32 li = kv >> 16;  // 1 + index of the true end of a row whose span is clipped (at most PRF_LONG_PER_TILE per
                    // tile): listed, and filled in behind the copy -- a load in here, however rare, makes every round wait for memory
                    if (li) fix[atomicAdd(&fix_n, 1u)] = (u64)(r0 + tid) | ((u64)lo << 32) | ((u64)(li - 1u) << 40);
                    st[3u * tid] = start - cbase[lo];
                    st[3u * tid + 1u] = start + (key & 0xFFFFu) - cbase[lo];
                    st[3u * tid + 2u] = (u64)(kv & 0xFFFFu) | ((u64)contig[lo] << 32);
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                const u32 n_words = 3u * (n_copy - r0 < 256u ? n_copy - r0 : 256u);
                // 16-byte stores (8-byte ones run at 0.5 - 0.7 of their rate): the round's first word alone if it sits on an odd
                // 8-byte boundary, pairs from there on, the last word alone if one is left over
                u64 *d = dst + 3ull * r0;
                const u32 head = (u32)((reinterpret_cast<uintptr_t>(d) >> 3) & 1u);
                if (tid == 0 && head) d[0] = st[0];
                for (u32 p = tid; head + 2u * p + 1u < n_words; p += 256u) {
                    const u32 w = head + 2u * p;
                    ulonglong2 v;
                    v.x = st[w];
                    v.y = st[w + 1u];
                    *reinterpret_cast<ulonglong2 *>(d + w) = v;
                }
                if (tid == 1 && ((n_words - head) & 1u)) d[n_words - 1u] = st[n_words - 1u];
                buf ^= 1u;
            }
        });
    }
    // the workgroup of the last slots knows the total
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        atomicAdd(&g.counters[PRF_CNT_ROWS], base0 + n_mine);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // performed before this thread draws the finishing ticket below
    }
    __syncthreads();
    if (fix_n) {  // (uniform) the true ends of the clipped rows, over the clipped ones the rounds have stored
        // (a barrier does not wait for stores on this target: every wave waits for its own, then they meet)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (u32 i = tid; i < fix_n; i += 256u) {
            const u64 e = fix[i];
            const u32 row = (u32)e, lo = (u32)(e >> 32) & 255u, li = (u32)(e >> 40);
            dst[3ull * row + 1u] = g.long_ends[(u64)(first + lo) * PRF_LONG_PER_TILE + li] - cbase[lo];
        }
        __syncthreads();
    }
    // Finishing tickets in two levels (one word takes ~90 atomics per microsecond: thousands of workgroups on ONE ticket word
    // would cost more than the copy): a ticket per 64 workgroups, and the last of each 64 draws a global one.
    const u32 n_supers = (gridDim.x - 1u) / PRF_GATHER_SUPER + 1u;
    if (tid == 0) {
        const u32 in_super = my_super + 1u < n_supers ? PRF_GATHER_SUPER : gridDim.x - my_super * PRF_GATHER_SUPER;
        u64 t = 0;
        if (atomicAdd(&g.block_sum[g.super_off + n_supers + my_super], 1u) == in_super - 1u)
            t = atomicAdd(&g.counters[PRF_CNT_TICKET], 1ull) + 1ull;
        ticket_lds = t;  // n_supers: this workgroup is the last one of the whole grid
    }
    __syncthreads();
    // ---- the last workgroup hands the counter block to the host.  The counters are only ever touched
    // by device-scope atomics, performed at the coherence point, and the one this kernel adds (the row total) has been waited
    // for by the thread that draws its workgroup's ticket, so it precedes the last ticket.  Every
    // other workgroup has read its sums by then: they are cleared for the next scan.
    if (ticket_lds == (u64)n_supers) {
        for (u32 i = tid; i < 2u * n_supers; i += 256u) g.block_sum[g.super_off + i] = 0;
        for (u32 i = tid; i < gridDim.x; i += 256u) g.block_sum[i] = 0;
        for (u32 i = tid; i < (u32)PRF_CNT_N; i += 256u) {
            const u64 v = atomicAdd(&g.counters[i], 0ull);
            g.host_counters[i] = v;
            g.next_counters[i] = 0;
            if (i == (u32)PRF_CNT_ROWS && g.count_row) {  // a caller-owned row array carries its own length
                prf_hit_dev h;
                h.start = v < g.rows_cap ? v : g.rows_cap;
                h.end = 0;
                h.k = 0;
                h.contig = 0;
                g.rows[g.rows_cap] = h;
            }
        }
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&g.host_counters[PRF_CNT_N], g.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t prf_vertical_gather(hipStream_t s, const prf_vgather_args &args) {
    const u32 n_slots = 1u << args.gather_shift;
    const u32 nb = args.n_launch ? (args.n_launch + n_slots - 1u) / n_slots : 1u;
    hipLaunchKernelGGL(prf_vgather_kernel, dim3(nb), dim3(256), 0, s, args);
    return hipGetLastError();
}
