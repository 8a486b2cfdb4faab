// vscan_tasks.h -- a section of scan_vertical.hip, included exactly once inside its anonymous namespace; not an interface.
// Phase 2 of the fused kernel, image -> candidates: the tasks' answers to LDS lists (Emit), the group, exact and coarse tasks,
// their dispatch, and run_tasks, a wave's share of the plan.

// The tasks' answers -> LDS lists.  Every lane of the wave calls these together.
struct Emit {
    prf_lds_u64 *recs;       // the tile's record list in LDS, REC_CAP records
    prf_lds_u32 *cnt;        // this tile's counter set
    int lane;
#ifdef PRF_STAMPS
    u64 t_push_g = 0, t_push_f = 0;  // cycles this wave spent handing over the answers of its group / exact and coarse tasks (this tile)
#endif

    // Exact tasks: the lanes' words of ONE task -> flags (lane | stream bit << 6 | task << 11) appended to the tile's list.
    // Each lane reserves for itself, as emit_row does: the lanes with flags issue ONE returning LDS add on the list's counter in one
    // instruction (the hardware hands every lane its own base), then write their flags behind that base; the loop runs as often
    // as the wave's unluckiest lane has flags.  (The first version reserved per round of the loop: 2.7 k cycles per task in here
    // against 2 k in the task itself.)  That puts a lane's flags side by side in the list, where the old placement had them level
    // by level in tile order.  A task in which some lane has more than DENSE_FLAGS flags (a tile of clusters; 2 % of the tasks
    // otherwise) keeps the old placement (push_flags_levels): measured on chr22-real, whose kernel time is its densest tile, that
    // took the kernel from +7 % to +2 % against the parent.  Why the order matters there was not established (the verification
    // takes one flag per thread, and a lane's streams lie 256 bytes apart in the window, the same LDS bank: a guess); the
    // threshold was not swept.  Flags beyond the list's capacity (a tile of long runs) are verified on the spot with the general
    // routine.
    static constexpr u32 DENSE_FLAGS = 4;
    __device__ __forceinline__ void push_flags(u32 word, u32 e, u32 k, prf_lds_u32 *flag_words) {
        typedef __attribute__((address_space(3))) unsigned short prf_lds_u16;
        prf_lds_u16 *list = (prf_lds_u16 *)flag_words;
        const u32 pc = (u32)__builtin_popcount(word);
        if (__builtin_amdgcn_ballot_w64(pc > DENSE_FLAGS) != 0) {  // wave-uniform
            push_flags_levels(word, e, k, list);
            return;
        }
        if (word == 0) return;
        u32 at = atomicAdd((u32 *)(cnt + CNT_FLAGS), pc);
        const u32 tag = (u32)lane | (e << 11);
        if (at + pc <= (u32)FLAG_CAP) {
            prf_lds_u16 *p = list + at;
            do {
                *p++ = (unsigned short)(tag | ((u32)__builtin_ctz(word) << 6));
                word &= word - 1;
            } while (word);
            return;
        }
        do {  // the list is full: what still fits is listed
            const u32 bit = (u32)__builtin_ctz(word);
            word &= word - 1;
            if (at < (u32)FLAG_CAP) {
                list[at] = (unsigned short)(tag | (bit << 6));
            } else {
                atomicAdd((u32 *)(cnt + CNT_EARLY), 1u);
                verify_stream(reinterpret_cast<const TileCtx *>(prf_smem)->tile_base + (u64)(bit * 64u + (u32)lane) * T, k, 0u);
            }
            at++;
        } while (word);
    }

    // The placement for dense tasks: ONE reservation for the wave.  A first pass of ballots counts the flags level by level (level
    // j = the lanes with more than j flags), one atomic reserves them, a second pass places them -- level j behind the levels below
    // it, a lane's flag behind those of the lower lanes: neighbours in the list are neighbours in the tile.  About 70
    // wave-instructions for a task of two levels.
    __device__ __forceinline__ void push_flags_levels(u32 word, u32 e, u32 k, __attribute__((address_space(3))) unsigned short *list) {
        const u32 pc = (u32)__builtin_popcount(word);
        u32 total = 0;  // wave-uniform
        for (u32 j = 0;; j++) {
            const u64 bal = __builtin_amdgcn_ballot_w64(pc > j);
            if (bal == 0) break;
            total += (u32)__builtin_popcountll(bal);
        }
        u32 base = 0;
        if (lane == 0) base = atomicAdd((u32 *)(cnt + CNT_FLAGS), total);
        base = (u32)__builtin_amdgcn_readfirstlane((int)base);
        for (;;) {
            const u64 bal = __builtin_amdgcn_ballot_w64(word != 0);
            if (bal == 0) break;
            if (word) {
                const u32 bit = (u32)__builtin_ctz(word);
                word &= word - 1;
                const u32 at = base + __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0));
                if (at < (u32)FLAG_CAP) {
                    list[at] = (unsigned short)((u32)lane | (bit << 6) | (e << 11));
                } else {
                    atomicAdd((u32 *)(cnt + CNT_EARLY), 1u);
                    verify_stream(reinterpret_cast<const TileCtx *>(prf_smem)->tile_base + (u64)(bit * 64u + (u32)lane) * T, k, 0u);
                }
            }
            base += (u32)__builtin_popcountll(bal);
        }
    }

    // Group tasks: one 32-bit word per lane and motif size k0 + i (bit b = stream b*64 + lane is flagged for that size; zero for a
    // size the task does not have) -> one record per non-zero word, appended to the tile's list.  ONE reservation per task and
    // lane: a lane with n records adds n to the list's counter -- the lanes that have any do so in one instruction, without
    // ballot, readlane or mbcnt -- and writes them behind its base in size order.  (One reservation per SIZE through the first
    // lane with a record: 25 wave-instructions and an LDS round trip of its own for each of a task's 8 sizes.  One per task with
    // the eight ballots kept across the atomic: 37 more SGPRs than the kernel has, slower.)  A lane whose slots reach past the
    // list's capacity lists what fits and remembers the rest; those words are verified on the spot behind a wave-uniform test,
    // size by size with the general routine called from the kernel itself, as before.  (With the calls inside the lanes' own
    // branch the words lived in scratch memory around them; through a routine of their own every call saved and restored that
    // routine's registers in scratch memory, 3 k cycles in the scan phase of chr22-real's densest tile.)
    template <int N>  // 8, or 4 for a task of one half
    __device__ __forceinline__ void push_words(const u32 (&w)[N], u32 k0, u32 sc) {
        u32 n = 0;
        static_for<0, N>([&](auto ic) { n += w[decltype(ic)::value] != 0 ? 1u : 0u; });
        const u32 tag = make_rec_tag((u32)lane, k0, sc);
        u32 late = 0;  // bit i: word i found no room in the list
        if (n) {
            u32 idx = atomicAdd((u32 *)(cnt + CNT_RECS), n);
            if (idx + n <= (u32)REC_CAP) {
                prf_lds_u32x2 *at = (prf_lds_u32x2 *)(recs + idx);
                static_for<0, N>([&](auto ic) {
                    constexpr u32 i = (u32)decltype(ic)::value;
                    if (w[i]) *at++ = make_rec_halves(tag + (i << 6), w[i]);
                });
            } else {
                static_for<0, N>([&](auto ic) {
                    constexpr u32 i = (u32)decltype(ic)::value;
                    if (w[i]) {
                        if (idx < (u32)REC_CAP) ((prf_lds_u32x2 *)recs)[idx] = make_rec_halves(tag + (i << 6), w[i]);
                        else late |= 1u << i;
                        idx++;
                    }
                });
            }
        }
        // the list is full (wave-uniform test, cold): the words without a slot go size by size through the general routine
        if (__builtin_amdgcn_ballot_w64(late != 0) != 0) {
            const u64 tile_base = reinterpret_cast<const TileCtx *>(prf_smem)->tile_base;
            static_for<0, N>([&](auto ic) {
                constexpr u32 i = (u32)decltype(ic)::value;
                if ((late >> i) & 1u) {
                    atomicAdd((u32 *)(cnt + CNT_EARLY), 1u);
                    u32 word = w[i];
                    do {
                        const u32 bit = (u32)__builtin_ctz(word);
                        word &= word - 1;
                        verify_stream(tile_base + (u64)(bit * 64u + (u32)lane) * T, k0 + i, sc);
                    } while (word);
                }
            });
        }
    }
};

// v_bitop3_b32: any boolean function of three words in one VALU operation.  Truth-table operands:
constexpr u32 TA = 0xF0, TB = 0xCC, TC = 0xAA;
template <u32 TT>
__device__ __forceinline__ u32 bitop3(u32 a, u32 b, u32 c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
// acc | (b ^ c)
__device__ __forceinline__ u32 or_xor(u32 acc, u32 b, u32 c) { return bitop3<(TA | (TB ^ TC)) & 0xFF>(acc, b, c); }
// ~(a | b) & c
__device__ __forceinline__ u32 nor_and(u32 a, u32 b, u32 c) { return bitop3<(~(TA | TB) & TC) & 0xFF>(a, b, c); }
// a | b | c
__device__ __forceinline__ u32 or3(u32 a, u32 b, u32 c) { return bitop3<(TA | TB | TC) & 0xFF>(a, b, c); }

__device__ __forceinline__ void unpack4(u32 *dst, const prf_u32x4 v) {
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
}

// LDS image addressing.  The image is [plane][row group][virtual lane] of 16-byte slots, NC virtual lanes wide
// (compile-time, so plane and row-group strides are instruction immediates).  Row group gg of a lane's
// *extended* stream (gg >= 8: the stream continues in the next virtual lane) is slot (gg & 7) * NC + (gg >> 3)
// from the lane's own slot.
template <int NC, class P>
__device__ __forceinline__ P *slot_of(P *lane_base, int gg) {
    return lane_base + ((gg & 7) * NC + (gg >> 3));
}

// Slot g (compile-time) after a run-time first slot gg0 whose address `first` = slot_of(lane_base, gg0) and
// a = gg0 & 7 are computed once per block: the stream wraps into the next virtual lane at most once within a block.
template <int NC, int G>
__device__ __forceinline__ prf_lds_cu4 *slot_after(prf_lds_cu4 *first, int a) {
    return first + G * NC + (a + G >= 8 ? 1 - 8 * NC : 0);
}

// ---- group task: motif sizes k0 .. k0+7 (those in `valid`), the 8-row blocks 0 .. 3 of the stream ----
// S1: every block is examined (stride 1) and a group counts only if the group before it was not all-match; otherwise
// (stride 2 / 4, and every task of a mixed tile) every examined all-match group counts.  The per-size words are OR-ed over the
// blocks and leave as records at the end of the task, through one reservation per lane (Emit::push_words).  The eight sizes are
// computed as two halves of four, the rows of the second half's last slot loaded in between: 40 row registers instead of 48,
// four OR chains interleaved.
// HALF: only the sizes k0 .. k0+3 (a task whose second half wants another stride, or lies beyond the largest motif size).
template <int NC, bool S1, bool HALF>
__device__ __forceinline__ void group_task(prf_lds_cu4 *vimg, int lane, u32 k0, u32 valid, u32 stride, u32 allow, Emit &em) {
    constexpr int PS = RG * NC;  // slots per plane
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));  // (the address is recomputed here: hoisted out of the task loop it was kept in scratch memory)
    prf_lds_cu4 *lane_base = vimg + lane_o;
    u32 prev[8], acc[8];
    static_for<0, 8>([&](auto ic) {
        prev[decltype(ic)::value] = ~0u;  // first group of a stream: counts, verification decides
        acc[decltype(ic)::value] = 0u;
    });
#pragma unroll 1
    for (int tb = 0; tb < 4; tb += (int)stride) {
        u32 a[2][8];   // rows 8tb .. 8tb+7
        u32 w[2][16];  // rows 8tb+k0 .. 8tb+k0+15 (k0 % 4 == 0: whole 16-byte slots)
        const int g0 = 2 * tb + (int)(k0 >> 2);
        const int wa = g0 & 7;
        prf_lds_cu4 *pa = lane_base + 2 * tb * NC;
        prf_lds_cu4 *pw0 = slot_of<NC>(lane_base, g0);
        static_for<0, 2>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
            unpack4(&a[p][0], pa[p * PS]);
            unpack4(&a[p][4], pa[p * PS + NC]);
        });
        auto load_w = [&](auto gc) {
            constexpr int g = decltype(gc)::value;
            prf_lds_cu4 *pw = slot_after<NC, g>(pw0, wa);
            static_for<0, 2>([&](auto pc) {
                constexpr int p = decltype(pc)::value;
                unpack4(&w[p][4 * g], pw[p * PS]);
            });
        };
        // the four motif sizes 4h .. 4h+3 in one straight-line block: their independent OR chains interleave
        auto sizes = [&](auto hc) {
            constexpr int h = decltype(hc)::value;
            static_for<4 * h, 4 * h + 4>([&](auto kc) {
                constexpr int kk = decltype(kc)::value;
                // OR over the 8 rows of (H^H')|(L^L'): 16 operations, no per-row mismatch word
                u32 o = a[0][0] ^ w[0][kk];
                o = or_xor(o, a[1][0], w[1][kk]);
                static_for<1, 8>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    o = or_xor(o, a[0][i], w[0][kk + i]);
                    o = or_xor(o, a[1][i], w[1][kk + i]);
                });
                if constexpr (S1) {
                    acc[kk] = bitop3<(TA | (~TB & TC)) & 0xFF>(acc[kk], o, prev[kk]);  // acc | (~o & prev)
                    prev[kk] = o;
                } else {
                    acc[kk] |= ~o;
                }
            });
        };
        load_w(std::integral_constant<int, 0>{});
        load_w(std::integral_constant<int, 1>{});
        load_w(std::integral_constant<int, 2>{});
        sizes(std::integral_constant<int, 0>{});
        if constexpr (!HALF) {
            load_w(std::integral_constant<int, 3>{});
            sizes(std::integral_constant<int, 1>{});
        }
    }
    const u32 sc = stride == 1 ? 1u : (stride == 2 ? 2u : 3u);
#ifdef PRF_STAMPS
    asm volatile("" ::"v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]));  // (the body ends here)
    if constexpr (!HALF) asm volatile("" ::"v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]));
    const u64 tp0 = __builtin_amdgcn_s_memtime();
#endif
    static_for<0, (HALF ? 4 : 8)>([&](auto kc) {
        constexpr int kk = decltype(kc)::value;
        acc[kk] = ((valid >> kk) & 1u) ? acc[kk] & allow : 0u;  // (wave-uniform choice)
    });
    if constexpr (HALF) {
        const u32 w4[4] = {acc[0], acc[1], acc[2], acc[3]};
        em.push_words(w4, k0, sc);
    } else {
        em.push_words(acc, k0, sc);
    }
#ifdef PRF_STAMPS
    em.t_push_g += __builtin_amdgcn_s_memtime() - tp0;
#endif
}

// OR of the mismatch words of the M rows t .. t+M-1.  mm is indexed by row + 1 (mm[0] = the row before the stream),
// o3[i] = mm[i] | mm[i+1] | mm[i+2] (the rows i-1 .. i+1).
template <int M, int t, int LM, int LO>
__device__ __forceinline__ u32 window_or(const u32 (&mm)[LM], const u32 (&o3)[LO]) {
    constexpr int j = t + 1;  // first index
    if constexpr (M == 1) return mm[j];
    else if constexpr (M == 2) return mm[j] | mm[j + 1];
    else if constexpr (M == 3) return o3[j];
    else if constexpr (M <= 6) return o3[j] | o3[j + M - 3];
    else if constexpr (M <= 9) return or3(o3[j], o3[j + 3], o3[j + M - 3]);
    else if constexpr (M <= 12) return or3(o3[j], o3[j + 3], o3[j + 6]) | o3[j + M - 3];
    else return or3(or3(o3[j], o3[j + 3], o3[j + 6]), o3[j + 9], o3[j + M - 3]);
}

// ---- exact task: motif size K whose minimum run length is M < 15; the whole stream in one straight-line block ----
// Returns the lane's word: bit b set = stream (lane, b) holds a row t in 0..31 that starts a run of >= M matches:
// rows t .. t+M-1 all match and row t-1 does not, i.e. the window of M rows at t matches and the window at t-1 does not.
// The rows 0 .. 31+M-1+K of the extended stream are read ONCE, slot by slot (4 rows of both planes); a mismatch word is
// computed as soon as its partner row (K further on) is there, a window as soon as its last row is: the compiler sees
// straight-line code in that order and keeps only what is live -- K + 4 rows of two planes, M - 2 triple ORs, three
// mismatch words, the previous window -- under the 56 registers a function may use without saving any for its caller
// (round 2 read all 60 rows first: 128 VGPRs, four workgroups per CU).
// relax (mixed tile): a stream whose first M rows all match counts as well -- together with the starts that is "some M
// matching rows begin in this stream", which no added match (a not-ACGT position reads as A) can take away.
// K = 2, 3, 4 (ECHO) on a clean tile: a start whose run is the echo of a shorter motif -- its K letters have the period D = K / p,
// p the one prime in K; the verification would find that and drop the candidate -- is not flagged.  A run that starts at row t
// covers the rows t .. t+M-1+K, all of period K, so any K consecutive letters inside it are conjugates of one word and have the
// period D or none of them has: the test may be made at any row j in t .. t+M.  It is made once per segment of SEG start rows,
// (j - SEG, j] for j = 0, SEG, .. T, at row j (prim: the K - D mismatch words at distance D from row j on, OR-ed): SEG <= M + 1, so
// j <= t + M, and two starts lie at least M + 1 rows apart, so a segment holds at most one.  The starts are collected per
// segment with the one operation per row they cost anyway, and hot |= seg & prim closes the segment: 3 - 5 operations per
// segment instead of 3 - 4 per row.  A mixed tile suppresses nothing (a not-ACGT position reads as A: the true start may lie
// where the image sees the middle of a run).  Lane 0's conservative row -1 stays: an echo is never a row, wherever it began.
// K = 2 keeps what it throws away: its echo starts are the starts of the homopolymer runs, and those are the k = 1 task's
// answer.  A k = 1 run of L matches from position t (t .. t+L equal, t-1 different) is a k = 2 run of L - 1 matches from the
// same t (row t-1 fails: t-1 differs from t+1) whose two letters are equal; an echo start of >= M matches at distance 2 is,
// the other way round, a run of >= M + 1 matches at distance 1 that cannot have begun earlier.  So with M(1) = M(2) + 1 -- which
// is what min_span >= 2 min_repeats gives (prf_plan_derives_k1) -- hot1 |= seg & ~prim, one more operation per segment, is the
// word exact_stream<1, M + 1> would return, the conservative row -1 included: the plan then has no clean tile run the k = 1
// task (run_tasks hands it this word).  On a mixed tile prim is all ones and hot1 empty: there the k = 1 task runs.
// Returns hot in the low word and, for K = 2, hot1 in the high one.
// Not inlined: one compact function per (K, M), called by the one wave that runs the task.
template <int K, int M, int NC>
__device__ __attribute__((noinline)) u64 exact_stream(prf_lds_cu4 *vimg, int lane, bool relax) {
    constexpr int PS = RG * NC;
    constexpr bool ECHO = K >= 2 && K <= 4;
    constexpr int D = K == 4 ? 2 : 1;                               // K / p
    constexpr int SEG = M + 1 >= 8 ? 8 : (M + 1 >= 4 ? 4 : 2);      // largest power of two <= min(M + 1, 8)
    static_assert(!ECHO || (SEG <= M + 1 && T % SEG == 0 && K - 1 + T < T + M - 1 + K), "the sample lies inside the run and the rows read");
    constexpr int NM = T + M - 1;            // mismatch words of rows 0 .. NM-1
    constexpr int NG = (NM + K + 3) / 4;     // 16-byte slots of rows read
    static_assert(4 * NG <= 2 * T, "an exact task reads its own lane and the next one");
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));  // (the address is recomputed here: hoisted out of the task loop it was kept in scratch memory)
    prf_lds_cu4 *lane_base = vimg + lane_o;
    u32 r0[4 * NG], r1[4 * NG];
    u32 mm[NM + 1];
    u32 o3[NM + 1];
    u32 hot = 0, prev = 0;  // prev: the window one row earlier
    u32 seg = 0;            // (ECHO) the starts of the current segment
    u32 hot1 = 0;           // (K = 2) the echo starts: the k = 1 task's word
    u32 prim[ECHO ? T / SEG + 1 : 1];  // (ECHO) prim[j / SEG]: the K letters at row j are no power of a shorter word
    const u32 no_echo = relax ? ~0u : 0u;  // a mixed tile suppresses nothing (wave-uniform)
    auto load_slot = [&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (g < NG) {
            prf_lds_cu4 *ps = slot_of<NC>(lane_base, g);
            const prf_u32x4 v0 = ps[0], v1 = ps[PS];
            r0[4 * g] = v0.x; r0[4 * g + 1] = v0.y; r0[4 * g + 2] = v0.z; r0[4 * g + 3] = v0.w;
            r1[4 * g] = v1.x; r1[4 * g + 1] = v1.y; r1[4 * g + 2] = v1.z; r1[4 * g + 3] = v1.w;
        }
    };
    load_slot(std::integral_constant<int, 0>{});
    static_for<0, NG>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        load_slot(std::integral_constant<int, g + 1>{});  // one slot ahead of the rows that are computed: its latency hides behind them
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 4>([&](auto jc) {
            constexpr int i = 4 * g + decltype(jc)::value - K;  // the mismatch row whose partner row has just arrived
            if constexpr (ECHO && i >= 0 && i <= T && i % SEG == 0) {
                // the sample of the segment that ends at row i: the rows i .. i+K-1 (all here) against the ones D further on
                u32 n = no_echo;
                static_for<0, K - D>([&](auto qc) {
                    constexpr int q = i + decltype(qc)::value;
                    n = or_xor(n, r0[q], r0[q + D]);
                    n = or_xor(n, r1[q], r1[q + D]);
                });
                prim[i / SEG] = n;
            }
            if constexpr (i == -1) {
                // Row -1 of stream (lane, b) is row T-1 of stream (lane-1, b); for lane 0 it is row T-1 of stream (63, b-1):
                // lane 63's word one bit up, with bit 0 (the previous tile's last stream) unknown -> "mismatch", verification
                // decides.
                const int pl = (lane + 63) & 63;
                prf_lds_cu4 *pp = vimg + pl + (RG - 1) * NC;
                u32 p0 = pp[0].w, p1 = pp[PS].w;
                if (lane == 0) {
                    p0 <<= 1;
                    p1 <<= 1;
                }
                mm[0] = or_xor(p0 ^ r0[K - 1], p1, r1[K - 1]);
                if (lane == 0) mm[0] |= 1u;
                if constexpr (M == 1) prev = mm[0];  // (the window of one row at t = -1)
            } else if constexpr (i >= 0 && i < NM) {
                mm[i + 1] = or_xor(r0[i] ^ r0[i + K], r1[i], r1[i + K]);
                if constexpr (M >= 3 && i >= 1) o3[i - 1] = or3(mm[i - 1], mm[i], mm[i + 1]);
                constexpr int t = i - (M - 1);  // the window whose last row this is
                if constexpr (t >= -1 && t < T) {
                    const u32 win = window_or<M, t>(mm, o3);
                    if constexpr (!ECHO) {
                        if constexpr (t >= 0) hot = bitop3<(TA | (~TB & TC)) & 0xFF>(hot, win, prev);  // hot | (~win & prev)
                        if constexpr (t == 0) {
                            if (relax) hot |= ~win;
                        }
                    } else if constexpr (t >= 0) {
                        // the same operation per row, into the segment (t - SEG, t] that ends at the next multiple of SEG
                        if constexpr (t == 0 || t % SEG == 1) seg = ~win & prev;
                        else seg = bitop3<(TA | (~TB & TC)) & 0xFF>(seg, win, prev);  // seg | (~win & prev)
                        if constexpr (t == 0) {
                            if (relax) seg |= ~win;
                        }
                        // the segment's last start row (the one that ends at row T stops at T - 1): at most one start in it, and
                        // the sampled row lies inside that start's run
                        if constexpr (t % SEG == 0 || t == T - 1) {
                            hot = bitop3<(TA | (TB & TC)) & 0xFF>(hot, seg, prim[(t + SEG - 1) / SEG]);  // hot | (seg & prim)
                            if constexpr (K == 2) hot1 = bitop3<(TA | (TB & ~TC)) & 0xFF>(hot1, seg, prim[(t + SEG - 1) / SEG]);  // hot1 | (seg & ~prim)
                        }
                    }
                    prev = win;
                }
            }
        });
    });
    return (u64)hot | ((u64)hot1 << 32);
}

// ---- the same question answered more coarsely for M >= 9: rows in aligned groups of G = 2 (M <= 10) or 4 ----
// A run of >= M matching rows holds C = floor((M + 1) / G) - 1 consecutive aligned groups of G rows that match throughout:
// the first of them, group j0 = ceil(a / G), follows a group that does not (it holds row a - 1).  So the stream is
// flagged if, for some j in 0 .. T/G, the groups j .. j+C-1 all match and group j-1 does not.  j = T/G -- the first group of the
// NEXT stream -- is included because the run's first row may be one of the last G - 1 rows of this stream (the next stream's
// lane flags itself for the same group: a false flag there, which costs a look and nothing else).  Two operations per row
// for the groups' ORs, two or three per group for window and flag: 106 - 135 operations per task instead of 200 - 250; the price
// is false flags where G C rows match by chance without M doing so (6 rows: 8 per tile and motif size on random sequence,
// 8 rows: 0.5) -- the verification re-derives the run starts exactly either way (win_verify_flag uses M itself).  M = 7 and 8
// would get groups of 2 with C = 3: those 8 false flags per tile and motif size (52 per tile on the default workload, a third
// pass over the flags for one wave) cost more than the 70 operations they save: they keep the exact form.
// relax (mixed tile): also "the groups 0 .. C-1 match", which with the rule above is "some C matching groups begin here".
template <int K, int M, int NC>
__device__ __attribute__((noinline)) u32 coarse_stream(prf_lds_cu4 *vimg, int lane, bool relax) {
    constexpr int PS = RG * NC;
    constexpr int G = M >= 11 ? 4 : 2, C = (M + 1) / G - 1;
    constexpr int NJ = T / G + 1;                   // windows j = 0 .. T/G
    constexpr int NGRP = NJ + C;                    // groups -1 .. T/G + C - 1, stored at index + 1
    constexpr int NR = T + G * C;                   // mismatch rows -G .. NR - 1
    constexpr int NG = (NR + K + 3) / 4;            // 16-byte slots of rows read
    static_assert(C >= 2 && 4 * NG <= 2 * T, "a coarse task reads its own lane and the next one");
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));  // (the address is recomputed here: hoisted out of the task loop it was kept in scratch memory)
    prf_lds_cu4 *lane_base = vimg + lane_o;
    // rows -4 .. -1: the last slot of the previous stream, (lane-1, b); for lane 0 that is stream (63, b-1): lane 63's words one
    // bit up, with bit 0 (the previous tile's last stream) unknown -> "mismatch", verification decides
    u32 q0[4], q1[4];
    {
        const int pl = (lane + 63) & 63;
        prf_lds_cu4 *pp = vimg + pl + (RG - 1) * NC;
        prf_u32x4 v0 = pp[0], v1 = pp[PS];
        if (lane == 0) {
            v0 <<= 1;
            v1 <<= 1;
        }
        q0[0] = v0.x; q0[1] = v0.y; q0[2] = v0.z; q0[3] = v0.w;
        q1[0] = v1.x; q1[1] = v1.y; q1[2] = v1.z; q1[3] = v1.w;
    }
    u32 r0[4 * NG], r1[4 * NG];
    u32 grp[NGRP];
    u32 hot = 0;
    auto load_slot = [&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (g < NG) {
            prf_lds_cu4 *ps = slot_of<NC>(lane_base, g);
            const prf_u32x4 v0 = ps[0], v1 = ps[PS];
            r0[4 * g] = v0.x; r0[4 * g + 1] = v0.y; r0[4 * g + 2] = v0.z; r0[4 * g + 3] = v0.w;
            r1[4 * g] = v1.x; r1[4 * g + 1] = v1.y; r1[4 * g + 2] = v1.z; r1[4 * g + 3] = v1.w;
        }
    };
    // row r of plane p, r >= -4 (compile-time r)
    auto h = [&](auto rc) -> u32 { constexpr int r = decltype(rc)::value; if constexpr (r < 0) return q0[r + 4]; else return r0[r]; };
    auto l = [&](auto rc) -> u32 { constexpr int r = decltype(rc)::value; if constexpr (r < 0) return q1[r + 4]; else return r1[r]; };
    load_slot(std::integral_constant<int, 0>{});
    static_for<0, NG>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        load_slot(std::integral_constant<int, g + 1>{});  // one slot ahead of the rows that are computed
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 4>([&](auto jc) {
            constexpr int i = 4 * g + decltype(jc)::value - K;  // the mismatch row whose partner row has just arrived
            // the last row of group j = (i + 1) / G - 1 (groups -1 .. NGRP - 2): the whole group is there now
            if constexpr (i >= -1 && i < NR && (i + 1) % G == 0) {
                constexpr int j = (i + 1) / G - 1, first = G * j;
                u32 t = h(std::integral_constant<int, first>{}) ^ h(std::integral_constant<int, first + K>{});
                t = or_xor(t, l(std::integral_constant<int, first>{}), l(std::integral_constant<int, first + K>{}));
                static_for<1, G>([&](auto ic) {
                    constexpr int r = first + decltype(ic)::value;
                    t = or_xor(t, h(std::integral_constant<int, r>{}), h(std::integral_constant<int, r + K>{}));
                    t = or_xor(t, l(std::integral_constant<int, r>{}), l(std::integral_constant<int, r + K>{}));
                });
                if constexpr (j == -1) {
                    if (lane == 0) t |= 1u;
                }
                grp[j + 1] = t;
                constexpr int w = j - C + 1;  // the window whose last group this is
                if constexpr (w >= 0 && w < NJ) {
                    u32 win;
                    if constexpr (C == 2) win = grp[w + 1] | grp[w + 2];
                    else if constexpr (C == 3) win = or3(grp[w + 1], grp[w + 2], grp[w + 3]);
                    else if constexpr (C == 4) win = or3(grp[w + 1], grp[w + 2], grp[w + 3]) | grp[w + 4];
                    else win = or3(or3(grp[w + 1], grp[w + 2], grp[w + 3]), grp[w + 4], grp[w + 5]);
                    static_assert(C <= 5, "window of at most five groups");
                    hot = bitop3<(TA | (~TB & TC)) & 0xFF>(hot, win, grp[w]);  // hot | (~win & group w-1)
                    if constexpr (w == 0) {
                        if (relax) hot |= ~win;
                    }
                }
            }
        });
    });
    return hot;
}

// The (K, M) variants, K <= M < SMALL_M, numbered densely in (K, M) order; the dispatch is a binary search over that number
// (7 wave-uniform branches; a chain of `if (k == K)` tests cost a task about thirty taken branches).
constexpr int exact_variants() { return (SMALL_M - 1) * SMALL_M / 2; }
constexpr int exact_variant_of(int K, int M) { return (K - 1) * (2 * SMALL_M - K) / 2 + (M - K); }
constexpr int exact_variant_k(int v) {
    int K = 1;
    while (exact_variant_of(K + 1, K + 1) <= v) K++;
    return K;
}
template <int LO, int HI, int NC>
__device__ __forceinline__ u64 exact_dispatch(prf_lds_cu4 *vimg, int lane, bool relax, u32 v) {
    if constexpr (LO == HI) {
        constexpr int K = exact_variant_k(LO), M = K + (LO - exact_variant_of(K, K));
        static_assert(M >= K && M < SMALL_M && exact_variant_of(K, M) == LO, "variant numbering");
        if constexpr (M >= 9) return coarse_stream<K, M, NC>(vimg, lane, relax);  // (M = 7, 8: groups of 2 rows give 8 false flags per tile and size)
        else return exact_stream<K, M, NC>(vimg, lane, relax);
    } else {
        constexpr int MID = (LO + HI) / 2;
        if (v <= (u32)MID) return exact_dispatch<LO, MID, NC>(vimg, lane, relax, v);  // wave-uniform
        return exact_dispatch<MID + 1, HI, NC>(vimg, lane, relax, v);
    }
}

template <int NC>
__device__ __forceinline__ u64 exact_any(prf_lds_cu4 *vimg, int lane, bool relax, u32 k, u32 M) {
    // (min_repeats - 1) * k <= M < SMALL_M and min_repeats >= 2: k <= M
    const u32 v = (k - 1u) * (2u * (u32)SMALL_M - k) / 2u + (M - k);
    return exact_dispatch<0, exact_variants() - 1, NC>(vimg, lane, relax, v);
}

// relax: mixed tile (see the head of the file); allow = ~(streams of this lane that hold nothing but N), all ones on a clean tile
// k1w: 64 words of LDS that are free while a clean tile is scanned (the derived k = 1 flags pass through them, see below)
template <int NC>
__device__ __forceinline__ void run_tasks(prf_lds_cu4 *vimg, prf_lds_u32 *hotw, prf_lds_u32 *k1w, const prf_vplan &plan, int wave, int lane, bool relax,
                                          u32 allow, Emit &em, u64 *dbg) {
    const u32 t_end = plan.wave_begin[wave + 1];
    {   // (opaque: the exact tasks are functions, and a callee that knows the image's address as a constant looks the dynamic LDS
        // base up in a table in memory on every call -- handed over as an argument it is a register)
        u32 a = (u32)(__UINTPTR_TYPE__)vimg;
        asm volatile("" : "+s"(a));
        vimg = (prf_lds_cu4 *)(__UINTPTR_TYPE__)a;
    }
#ifdef PRF_STAMPS
    u64 t_call = 0;
#endif
    for (u32 ti = plan.wave_begin[wave]; ti < t_end; ti++) {
        // (the task as two dwords, decoded by hand: left to the compiler the one-byte fields came by vector loads from the kernel's
        // arguments -- a global-memory round trip, waited for on the spot, in front of every group task)
        static_assert(sizeof(prf_vtask) == 8 && alignof(prf_vtask) == 4, "a task is read as two dwords");
        const u32 *tw = reinterpret_cast<const u32 *>(&plan.tasks[ti]);
        const u32 tw0 = (u32)__builtin_amdgcn_readfirstlane((int)tw[0]), tw1 = (u32)__builtin_amdgcn_readfirstlane((int)tw[1]);
        prf_vtask task;
        task.k0 = (unsigned short)(tw0 & 0xFFFFu);
        task.kind = (unsigned char)((tw0 >> 16) & 0xFFu);
        task.valid = (unsigned char)(tw0 >> 24);
        task.stride = (unsigned char)(tw1 & 0xFFu);
        task.pad = (unsigned char)((tw1 >> 8) & 0xFFu);
        task.item0 = (unsigned short)(tw1 >> 16);
#ifdef PRF_STAMPS
        if (dbg && lane == 0 && ti - plan.wave_begin[wave] < 4u) dbg[8 + (ti - plan.wave_begin[wave])] = __builtin_amdgcn_s_memtime();
#endif
        if (task.kind == 0) {
            const bool half = (task.valid & 0xF0u) == 0;
            if (task.stride == 1 && !relax) {
                if (half) group_task<NC, true, true>(vimg, lane, task.k0, task.valid, 1u, allow, em);
                else group_task<NC, true, false>(vimg, lane, task.k0, task.valid, 1u, allow, em);
            } else {
                if (half) group_task<NC, false, true>(vimg, lane, task.k0, task.valid, task.stride, allow, em);
                else group_task<NC, false, false>(vimg, lane, task.k0, task.valid, task.stride, allow, em);
            }
        } else {
            // (wave-uniform) a plan that derives the k = 1 flags: on a clean tile the k = 2 task leaves its second word -- its echo
            // starts, see exact_stream -- in LDS (k1w: the words of the all-N masks, which only a mixed tile has), and the k = 1
            // task, which the plan puts directly behind it in the same wave, is not run: it pushes that word as its own.  (A second
            // push inside the k = 2 task kept the word and the task's fields alive across the first one's calls: 2 - 8 more spilled
            // SGPRs.)  A mixed tile suppresses no echo, so that word is empty there and the k = 1 task runs itself.
            u32 word;
#ifdef PRF_STAMPS
            const u64 tc0 = __builtin_amdgcn_s_memtime();
#endif
            if ((task.pad & PRF_TASK_DERIVED) && !relax) {
                word = k1w[lane];
            } else {
                const u64 words = exact_any<NC>(vimg, lane, relax, task.k0, task.kind);
                word = (u32)words & allow;
                if ((task.pad & PRF_TASK_RAISES_K1) && !relax) k1w[lane] = (u32)(words >> 32) & allow;
            }
#ifdef PRF_STAMPS
            asm volatile("" ::"v"(word));
            const u64 tc1 = __builtin_amdgcn_s_memtime();
            t_call += tc1 - tc0;
#endif
            em.push_flags(word, task.item0, task.k0, hotw);
#ifdef PRF_STAMPS
            em.t_push_f += __builtin_amdgcn_s_memtime() - tc1;
#endif
        }
    }
#ifdef PRF_STAMPS
    // slot 15: [21:0] cycles inside the exact-task functions, [42:22] in push_flags, [63:43] in the group tasks' pushes
    if (dbg && lane == 0) dbg[15] = (t_call & 0x3FFFFFull) | ((em.t_push_f & 0x1FFFFFull) << 22) | ((em.t_push_g & 0x1FFFFFull) << 43);
#endif
}
