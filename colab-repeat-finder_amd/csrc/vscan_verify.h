// vscan_verify.h -- a section of scan_vertical.hip, included exactly once inside its anonymous namespace; not an interface.
// Phase 3 of the fused kernel, candidates -> rows: the general routines over global memory, the lean ones over the LDS
// window, the list of deferred candidates, the boundary items, and verify_all / verify_general that drive them.

// One row, as 8 bytes (scan_vertical.h): the first QCAP of each quarter of a tile into that quarter's LDS sublist, the others
// straight to the slab from its first slot on (a tile that dense sorts all of them in R1 at its end).  Sort key: start in the tile (16 bits), then length
// clipped to 16 bits -- exact, because of the rows that share a start at most one is longer than two motif sizes (two
// periods on a long common stretch force their gcd, Fine and Wilf).  The true end of a clipped row goes to
// the tile's short list of long ends.
__device__ __forceinline__ void emit_row(const TileCtx &tc, u64 a, u64 b, u32 k) {
    const u64 span = b + k - a;
    prf_lds_u32 *cnt = (prf_lds_u32 *)(prf_smem + tc.cnt_off);
    u32 kv = k;
    if (span >= 65535ull) {
        const u32 j = atomicAdd((u32 *)(cnt + CNT_LONG), 1u);
        if (j < PRF_LONG_PER_TILE) {
            ((prf_lds_u64 *)(prf_smem + HDR_LONG))[j] = b + k;
            kv |= (j + 1u) << 16;
        }
    }
    const u32 key = ((u32)(a - tc.tile_base) << 16) | (span < 65535ull ? (u32)span : 65535u);
    const u32 q = key >> 30;  // the quarter of the tile the row starts in: rows of different quarters are never compared
    const u32 i = atomicAdd((u32 *)(cnt + CNT_ROWS + q), 1u);
    if (i < (u32)QCAP) {
        prf_lds_u32 *keys = (prf_lds_u32 *)(prf_smem + tc.keys_off) + q * (u32)QCAP;
        keys[i] = key;
        keys[ROW_CAP_LDS + i] = kv;
    } else {
        const u32 j = atomicAdd((u32 *)(cnt + CNT_OVF), 1u);
        if (j < tc.slab_cap) tc.slab[j] = (u64)key | ((u64)kv << 32);
    }
}

// One 64-position look: mismatch bits (1 = differs, or either side is not ACGT) of positions q .. q+63 against q+k ..,
// served from the LDS window where it covers both sides, from the global planes elsewhere.  NOT inlined: the general
// routine is a few looks per candidate in divergent code, and forty inlined copies of the look were 90 KB of kernel (the
// instruction cache is shared by two CUs).
__device__ __noinline__ u64 tile_mismatch64(u64 q, u32 k) {
    const TileCtx &tc = *reinterpret_cast<const TileCtx *>(prf_smem);
    prf_window_view view;
    view.lds = (prf_lds_cu64 *)(prf_smem + tc.lin_off);
    view.w0 = tc.w0;
    view.nwords = tc.has_lin ? LW : 0;  // 0: every look goes to the global planes (while R1 holds the image)
    view.xz_lo = tc.xz_lo;
    view.xz_hi = tc.xz_hi;
    view.x_in_lds = 0;
    view.P[0] = tc.H; view.P[1] = tc.L; view.P[2] = tc.X;
    view.E = tc.E;
    return view.mismatch64(q, k);
}

// run at motif size k, known to match up to `from`: where does it end?  (the guard gap guarantees an end)
__device__ __forceinline__ u64 run_end(u64 from, u32 k) {
    u64 b = from;
    for (;;) {
        const u64 m2 = tile_mismatch64(b, k);
        if (m2) return b + (u64)__builtin_ctzll(m2);
        b += 64;
    }
}

// Is seq[a : a+k] a whole number (>= 2) of copies of a shorter word?  (reference consists_of_perfect_repeats,
// utils/perfect_repeat_tracker.py:108-142, tries every divisor.)  A word of length k has a proper divisor period iff it has
// period k/p for some prime p | k: one period test per entry of cof[k].
__device__ __forceinline__ bool motif_is_repeat(u64 a, u32 k) {
    const TileCtx &tc = *reinterpret_cast<const TileCtx *>(prf_smem);
    for (u32 cf = ((prf_lds_cu32 *)(prf_smem + tc.cof_off))[k]; cf; cf >>= 8) {
        const u32 d = cf & 255u, need = k - d;  // period d: positions a .. a+need-1 equal the ones d later
        bool has = true;
        for (u32 off = 0; off < need; off += 64) {
            u64 mm = tile_mismatch64(a + off, d);
            const u32 left = need - off;
            if (left < 64) mm &= (1ull << left) - 1ull;
            if (mm) {
                has = false;
                break;
            }
        }
        if (has) return true;
    }
    return false;
}

// Every candidate of motif size k that the flagged stream [sp, sp+32) owns, re-derived from the linear planes.
//  sc == 0 (exact task, M = M(k) < 15): every position a in the stream that starts a maximal run of >= M matches.
//  sc >= 1 (group task, every S = 1 << (sc-1) th aligned group of 8 examined): every examined all-match group of the
//          stream that is the FIRST examined all-match group of its run; the run is dropped if it starts before the
//          tile (the previous tile reports it, see boundary_pass).
__device__ __noinline__ void verify_stream(u64 sp, u32 k, u32 sc) {
    const TileCtx &tc = *reinterpret_cast<const TileCtx *>(prf_smem);
    const long long M = prf_min_matches(k, tc.min_repeats, tc.min_span);
    if (sc == 0) {
        // bit i of m = mismatch at position sp - 1 + i
        const u64 m = sp ? tile_mismatch64(sp - 1, k) : ((tile_mismatch64(0, k) << 1) | 1ull);
        u64 r = ~m;  // bit i: positions i .. i+len-1 all match
        u32 len = 1;
        while (2 * len <= (u32)M) {
            r &= r >> len;
            len *= 2;
        }
        if (len < (u32)M) r &= r >> ((u32)M - len);
        u64 st = r & (m << 1) & 0x1FFFFFFFEull;  // starts at bits 1 .. 32 = the stream's own positions
        while (st) {
            const u32 i = (u32)__builtin_ctzll(st);
            st &= st - 1;
            const u64 a = sp - 1 + i;
            const u64 after = m >> i;  // bit j = mismatch at a + j, known for j < 64 - i
            const u64 b = after ? a + (u64)__builtin_ctzll(after) : run_end(a + (64 - i), k);
            if (!motif_is_repeat(a, k)) emit_row(tc, a, b, k);
        }
        return;
    }
    const u32 S = 1u << (sc - 1u);
    const u32 back = 8u * S;  // distance between examined groups
    for (u32 j = 0; j < 4u; j += S) {
        const u64 p = sp + 8u * j;
        const u32 look = p >= back ? back : (u32)p;   // the arrays start less than `back` before p (first tile only)
        const u64 mm = tile_mismatch64(p - look, k);  // bit i = mismatch at p - look + i
        if ((mm >> look) & 0xFFull) continue;         // the group [p, p+8) does not match throughout
        const u64 lead = mm & ((1ull << look) - 1ull);
        u64 a;
        if (lead == 0) {
            if (look == back) continue;  // the previous examined group lies in the same run: it reports
            a = p - look;                // the run starts at position 0
        } else {
            a = p - (u64)__builtin_clzll(lead << (64 - look));  // matches directly before p
        }
        if (a < tc.tile_base) continue;  // owned by the tile that holds the start
        const u64 seen = (mm >> look) >> 8;  // bit i = mismatch at p + 8 + i, known for i < 56 - look
        const u64 b = seen ? p + 8 + (u64)__builtin_ctzll(seen) : run_end(p + (64 - look), k);
        if ((long long)(b - a) < M) continue;
        if (!motif_is_repeat(a, k)) emit_row(tc, a, b, k);
    }
}

// ---- lean verification for the common case: a candidate whose looks stay inside the LDS window ----
// Window positions: bit 0 of the window = WIN_LEAD positions before the tile; the window holds H and L.  The not-ACGT plane is
// known to be zero there for a clean tile; a mixed tile reads it from global memory (L2), 32 bits at a time like the window.
constexpr u32 WIN_POS = (u32)LW * 64u;  // positions in the window

__device__ __forceinline__ u32 look32(prf_lds_cu32 *plane, u32 q) {
    const u32 w = q >> 5;
    return __builtin_amdgcn_alignbit(plane[w + 1], plane[w], q & 31u);
}
__device__ __forceinline__ u64 look64(prf_lds_cu32 *plane, u32 q) {
    const u32 w = q >> 5, sft = q & 31u;
    const u32 w0 = plane[w], w1 = plane[w + 1], w2 = plane[w + 2];
    return (u64)__builtin_amdgcn_alignbit(w1, w0, sft) | ((u64)__builtin_amdgcn_alignbit(w2, w1, sft) << 32);
}
// the same on the global not-ACGT plane: xw = the plane's 32-bit words from window position 0 on (wave-uniform), q per thread
__device__ __forceinline__ u32 xword(const u32 *xw, u32 w) {
    return *(prf_glb_cu32 *)(reinterpret_cast<const char *>(xw) + 4u * w);
}
__device__ __forceinline__ u32 xlook32(const u32 *xw, u32 q) {
    const u32 w = q >> 5;
    return __builtin_amdgcn_alignbit(xword(xw, w + 1), xword(xw, w), q & 31u);
}
__device__ __forceinline__ u64 xlook64(const u32 *xw, u32 q) {
    const u32 w = q >> 5, sft = q & 31u;
    const u32 w0 = xword(xw, w), w1 = xword(xw, w + 1), w2 = xword(xw, w + 2);
    return (u64)__builtin_amdgcn_alignbit(w1, w0, sft) | ((u64)__builtin_amdgcn_alignbit(w2, w1, sft) << 32);
}
// A 64-position look in two steps, for code that wants several looks in flight at once: raw64 issues the three reads, cut64
// shifts the words into place.  Between the two, looks_in_flight() names every raw look as an operand of one empty asm
// statement: left alone the compiler waits for each look before it issues the next (a round trip each).
typedef u32 prf_u32x3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ prf_u32x3 raw64(prf_lds_cu32 *plane, u32 q) {
    const u32 w = q >> 5;
    const prf_u32x3 r = {plane[w], plane[w + 1], plane[w + 2]};
    return r;
}
__device__ __forceinline__ u64 cut64(prf_u32x3 r, u32 q) {
    const u32 sft = q & 31u;
    return (u64)__builtin_amdgcn_alignbit(r.y, r.x, sft) | ((u64)__builtin_amdgcn_alignbit(r.z, r.y, sft) << 32);
}
struct WinCtx {
    prf_lds_cu32 *h, *l, *cof;
    const u32 *xw;  // mixed tile: the not-ACGT plane from window position 0 on (global memory); nullptr for clean tiles
    u64 win0;       // global position of window bit 0
    u32 min_repeats, min_span;
};

// mismatch bits of window positions q .. q+31 / q+63 against q+k ..; the caller guarantees q + k + 96 <= WIN_POS
__device__ __forceinline__ u32 win_mismatch32(const WinCtx &wc, u32 q, u32 k) {
    u32 r = (look32(wc.h, q) ^ look32(wc.h, q + k)) | (look32(wc.l, q) ^ look32(wc.l, q + k));
    if (wc.xw) r |= xlook32(wc.xw, q) | xlook32(wc.xw, q + k);
    return r;
}
__device__ __forceinline__ u64 win_mismatch64(const WinCtx &wc, u32 q, u32 k) {
    u64 r = (look64(wc.h, q) ^ look64(wc.h, q + k)) | (look64(wc.l, q) ^ look64(wc.l, q + k));
    if (wc.xw) r |= xlook64(wc.xw, q) | xlook64(wc.xw, q + k);
    return r;
}

__device__ __forceinline__ u32 min_matches32(u32 k, u32 min_repeats, u32 min_span) {
    const u32 a = (min_repeats - 1u) * k, b = min_span > k ? min_span - k : 0u;
    return a > b ? a : b;
}

// The verification loops below contain NO call: a call site in a loop makes the register allocator keep everything that is
// live around it in the 24 callee-saved registers a six-workgroup kernel has, or in scratch memory -- the first version of
// this kernel spilled the loops' own state that way (412 scratch operations per tile).  The few candidates that cannot be
// finished inside the LDS window (a run that reaches past it, the first stream of a clean tile, whose look-back lies in
// front of the tile) are put on a short list and finished by the general routine once the loops are over; a tile with more
// of them than the list holds is verified again from its flags and records by the general routine alone.
//   word 0: [39:0] start a (or the stream's first position), [48:40] k, [50:49] sc, [51] 1 = a whole stream (verify_stream),
//           [52] the primitive-motif test is still to be done;   word 1: position the run is known to match up to
__device__ __forceinline__ void defer(const TileCtx &tc, u64 a, u32 k, u32 sc, u32 whole_stream, u32 need_motif, u64 from) {
    const u32 i = atomicAdd((u32 *)((prf_lds_u32 *)(prf_smem + tc.cnt_off) + CNT_SLOW), 1u);
    if (i < (u32)SLOW_CAP) {
        prf_lds_u64 *slow = (prf_lds_u64 *)(prf_smem + tc.slow_off);
        slow[2u * i] = a | ((u64)k << 40) | ((u64)sc << 49) | ((u64)whole_stream << 51) | ((u64)need_motif << 52);
        slow[2u * i + 1u] = from;
    }
}

// one deferred candidate, by the general routine
__device__ __noinline__ void slow_item(u64 w0, u64 from) {
    const TileCtx &tc = *reinterpret_cast<const TileCtx *>(prf_smem);
    const u64 a = w0 & ((1ull << 40) - 1ull);
    const u32 k = (u32)(w0 >> 40) & 511u, sc = (u32)(w0 >> 49) & 3u;
    if ((w0 >> 51) & 1ull) {
        verify_stream(a, k, sc);
        return;
    }
    if (((w0 >> 52) & 1ull) && motif_is_repeat(a, k)) return;
    const u64 b = run_end(from, k);
    if ((long long)(b - a) < prf_min_matches(k, tc.min_repeats, tc.min_span)) return;
    emit_row(tc, a, b, k);
}

// end of the run at motif size k that matches up to window position `from`: true and the end (global position), or false
// and `from` = the window position at which the walk leaves the window
__device__ __forceinline__ bool win_run_end(const WinCtx &wc, u32 &from, u32 k, u64 &b) {
    for (;;) {
        if (from + k + 96u > WIN_POS) return false;
        const u64 m2 = win_mismatch64(wc, from, k);
        if (m2) {
            b = wc.win0 + from + (u64)__builtin_ctzll(m2);
            return true;
        }
        from += 64u;
    }
}

// motif [a, a+k) at window position a with a + 2 k + 96 <= WIN_POS: a power of a shorter word?  (see motif_is_repeat)
__device__ __forceinline__ bool win_motif_is_repeat(const WinCtx &wc, u32 a, u32 k) {
    for (u32 cf = wc.cof[k]; cf; cf >>= 8) {
        const u32 d = cf & 255u, need = k - d;
        bool has = true;
        for (u32 off = 0; off < need; off += 32) {
            u32 mm = win_mismatch32(wc, a + off, d);
            const u32 left = need - off;
            if (left < 32) mm &= (1u << left) - 1u;
            if (mm) {
                has = false;
                break;
            }
        }
        if (has) return true;
    }
    return false;
}

// funnel shift right of the 128-bit value hi:lo by s in [1, 63]
__device__ __forceinline__ u64 shr128(u64 lo, u64 hi, u32 sft) { return (lo >> sft) | (hi << (64u - sft)); }

// cofactors k/p of the distinct primes p | k for k <= 15, two 4-bit fields per byte (see CofTable): no table look for the exact tasks
__device__ __forceinline__ u32 small_cof(u32 k) {
    const u64 t = k < 8u ? 0x0123010201010000ull : 0x0027014601250304ull;
    return (u32)(t >> (8u * (k & 7u))) & 255u;
}

// One (stream, exact task) flag: stream (lane rl, bit `bit`), motif size k.  128 positions of both planes
// from the position in front of the stream are read; the mismatch word, the run starts, the run ends and the periods of the
// primitive-motif test are funnel shifts of those registers.
__device__ __forceinline__ void win_verify_flag(const TileCtx &tc, const WinCtx &wc, u32 rl, u32 bit, u32 k) {
    const u32 q = WIN_LEAD + (bit * 64u + rl) * T;  // window position of the stream's first position
    const u32 w = (q - 1u) >> 5, sft = (q - 1u) & 31u;
    const u32 a0 = wc.h[w], a1 = wc.h[w + 1], a2 = wc.h[w + 2], a3 = wc.h[w + 3], a4 = wc.h[w + 4];
    const u32 b0 = wc.l[w], b1 = wc.l[w + 1], b2 = wc.l[w + 2], b3 = wc.l[w + 3], b4 = wc.l[w + 4];
    // bit i = window position q - 1 + i
    const u64 hlo = (u64)__builtin_amdgcn_alignbit(a1, a0, sft) | ((u64)__builtin_amdgcn_alignbit(a2, a1, sft) << 32);
    const u64 hhi = (u64)__builtin_amdgcn_alignbit(a3, a2, sft) | ((u64)__builtin_amdgcn_alignbit(a4, a3, sft) << 32);
    const u64 llo = (u64)__builtin_amdgcn_alignbit(b1, b0, sft) | ((u64)__builtin_amdgcn_alignbit(b2, b1, sft) << 32);
    const u64 lhi = (u64)__builtin_amdgcn_alignbit(b3, b2, sft) | ((u64)__builtin_amdgcn_alignbit(b4, b3, sft) << 32);
    u64 xlo = 0, xhi = 0;
    if (wc.xw) {
        const u32 c0 = xword(wc.xw, w), c1 = xword(wc.xw, w + 1), c2 = xword(wc.xw, w + 2), c3 = xword(wc.xw, w + 3), c4 = xword(wc.xw, w + 4);
        xlo = (u64)__builtin_amdgcn_alignbit(c1, c0, sft) | ((u64)__builtin_amdgcn_alignbit(c2, c1, sft) << 32);
        xhi = (u64)__builtin_amdgcn_alignbit(c3, c2, sft) | ((u64)__builtin_amdgcn_alignbit(c4, c3, sft) << 32);
    }
    const u32 M = min_matches32(k, wc.min_repeats, wc.min_span);
    // bit i = mismatch at window position q - 1 + i
    const u64 m = (hlo ^ shr128(hlo, hhi, k)) | (llo ^ shr128(llo, lhi, k)) | xlo | shr128(xlo, xhi, k);
    u64 r = ~m;  // -> bit i: positions i .. i+M-1 all match (M <= 14: three doublings and a rest)
    if (M >= 2) r &= r >> 1;
    if (M >= 4) r &= r >> 2;
    if (M >= 8) r &= r >> 4;
    {
        const u32 len = M >= 8 ? 8u : (M >= 4 ? 4u : (M >= 2 ? 2u : 1u));
        r &= r >> (M - len);
    }
    u64 st = r & (m << 1) & 0x1FFFFFFFEull;  // starts at bits 1 .. 32 = the stream's own positions
    const u32 cof_k = small_cof(k);
    while (st) {
        const u32 i = (u32)__builtin_ctzll(st);
        st &= st - 1;
        // primitive motif: no period k/p for a prime p | k (k - d <= 13 positions from the start on)
        bool rep = false;
        for (u32 cf = cof_k; cf && !rep; cf >>= 4) {
            const u32 d = cf & 15u;
            const u64 md = (hlo ^ shr128(hlo, hhi, d)) | (llo ^ shr128(llo, lhi, d));  // (no N inside a run of >= M >= k matches)
            rep = ((md >> i) & ((1ull << (k - d)) - 1ull)) == 0;
        }
        if (rep) continue;
        const u32 a = q - 1u + i;
        const u64 after = m >> i;  // bit j = mismatch at a + j, known for j < 64 - i
        if (after) {
            emit_row(tc, wc.win0 + a, wc.win0 + a + (u64)__builtin_ctzll(after), k);
        } else {
            u32 from = a + (64u - i);
            u64 b;
            if (win_run_end(wc, from, k, b)) emit_row(tc, wc.win0 + a, b, k);
            else defer(tc, wc.win0 + a, k, 0u, 0u, 0u, wc.win0 + from);
        }
    }
}

// ---- group-task records, in two stages (the upper half of the workgroup; verify_all drives them) ----
// Stage A lists the wave's flagged streams, 4 bytes each: [10:0] stream (bit * 64 + lane), [19:11] k, [21:20] stride code.  The
// list lies in R1 behind the window.  Stage B takes one stream per lane: ONE 64-position look says which of its examined
// groups are all-match, the first examined one of their run, with the run's start inside the tile -- the LEADERS --, and
// each leader is verified with the looks of its period tests issued in ONE batch before any of them is used.  A leader
// goes into that batch as two registers (passed as its six fields it costs seven, and the kernel spills):
//   [16:0] window position a of the run's start, [25:17] k, [30:26] nb = matches between a and the group, [31] k has a
//   fourth cofactor;  [55:32] the cofactors k/p of k's first three primes (cof[k]: read beside the stream's look, so that
//   nothing waits for the table), [57:56] j = the group's index in its stream, [62:58] e = matches seen directly behind
//   the group by the stream's look (31: no mismatch seen there).
constexpr u32 LEAD_CAP = 192u;  // flagged streams of one wave's list; a full list is worked off (stage B) and filled again
constexpr u32 LEAD_OFF = (u32)SMEM_HDR + 2u * (u32)LW * 8u;  // byte offset of the two lists: R1 behind the window
constexpr u32 LEAD_NO_END = 31u;

// One flagged stream at window position q, every S-th aligned group of 8 examined.  Returns the leaders (bit j =
// group j) whose looks stay inside the window, `far` = those whose looks may not (-> defer), nbs = 5 bits per group:
// matches directly before it; m = mismatch bits of window positions q - 32 .. q + 31.
__device__ __forceinline__ u32 win_leaders(const WinCtx &wc, u32 q, u32 k, u32 S, u64 m, u32 &nbs, u32 &far) {
    const u32 back = 8u * S;
    u32 leaders = 0;
    nbs = 0;
    far = 0;
#pragma unroll
    for (u32 j = 0; j < 4u; j++) {
        const u32 gb = 32u + 8u * j;  // bit of the group's first position
        const u64 lead = m << (64u - gb);  // bit 63 = the position directly before the group
        const u32 nb = lead ? (u32)__builtin_clzll(lead) : 64u;  // matches directly before it (>= 32 seen)
        const u32 a = q - 32u + gb - nb;
        const bool ok = (j & (S - 1u)) == 0u && ((m >> gb) & 0xFFull) == 0 && nb < back && a >= WIN_LEAD;
        const bool out = a + 2u * k + 96u > WIN_POS;
        leaders |= (ok && !out ? 1u : 0u) << j;
        far |= (ok && out ? 1u : 0u) << j;
        nbs |= (nb & 31u) << (5u * j);
    }
    return leaders;
}

__device__ __forceinline__ u64 make_leader(u32 q, u32 k, u32 cof_k, u32 j, u32 nb, u64 m) {
    const u32 gb = 32u + 8u * j;
    const u64 seen = gb + 8u < 64u ? m >> (gb + 8u) : 0ull;  // bit i = mismatch at group end + i (24 - 8 j positions known)
    const u32 e = seen ? (u32)__builtin_ctzll(seen) : LEAD_NO_END;
    const u32 lo = (q - 32u + gb - nb) | (k << 17) | (nb << 26) | ((cof_k >> 24) ? 1u << 31 : 0u);
    const u32 hi = (cof_k & 0xFFFFFFu) | (j << 24) | (e << 26);
    return (u64)lo | ((u64)hi << 32);
}

// period d of the motif at window position a (positions a .. a+k-d-1 equal the ones d later), mm = the test's first 64
// positions; a + 2 k + 96 <= WIN_POS.  Motif sizes up to 64 + d are decided by mm alone.
__device__ __forceinline__ bool win_has_period(const WinCtx &wc, u32 a, u32 k, u32 d, u64 mm) {
    const u32 need = k - d;
    if (need < 64u) mm &= (1ull << need) - 1ull;
    bool has = mm == 0;
    for (u32 off = 64; off < need && has; off += 64) {
        u64 m2 = win_mismatch64(wc, a + off, d);
        const u32 left = need - off;
        if (left < 64u) m2 &= (1ull << left) - 1ull;
        has = m2 == 0;
    }
    return has;
}

// One leader.  One batch of looks, issued together (one LDS round trip): the first 64 positions of the period test of the
// first two cofactors -- the whole test for k <= 64 + d.  (A third cofactor's look and the look for the run's end are not in
// the batch: with them the kernel needs more than its 80 registers, and few leaders get that far.)  Then: primitive motif
// (most group candidates are echoes of a short motif and end here), run end, length filter, row.
__device__ __forceinline__ void win_verify_leader(const TileCtx &tc, const WinCtx &wc, u64 item) {
    const u32 lo = (u32)item, hi = (u32)(item >> 32);
    const u32 a = lo & 0x1FFFFu, k = (lo >> 17) & 511u, nb = (lo >> 26) & 31u;
    const u32 d1 = hi & 255u, d2 = (hi >> 8) & 255u, d3 = (hi >> 16) & 255u, j = (hi >> 24) & 3u, e = (hi >> 26) & 31u;
    const u32 ge = a + nb + 8u;            // the group's end
    const u32 q32 = ge + 24u - 8u * j;     // the end of the stream's look (q + 32 + k + 96 <= WIN_POS for every stream of the tile)
    const u32 p1 = a + (d1 ? d1 : 1u), p2 = a + (d2 ? d2 : 1u);
    prf_u32x3 ra = raw64(wc.h, a), sa = raw64(wc.l, a), r1 = raw64(wc.h, p1), s1 = raw64(wc.l, p1), r2 = raw64(wc.h, p2), s2 = raw64(wc.l, p2);
    asm volatile("" : "+v"(ra), "+v"(sa), "+v"(r1), "+v"(s1), "+v"(r2), "+v"(s2));
    const u64 ha = cut64(ra, a), la = cut64(sa, a);
    u64 mm1 = (ha ^ cut64(r1, p1)) | (la ^ cut64(s1, p1)), mm2 = (ha ^ cut64(r2, p2)) | (la ^ cut64(s2, p2));
    if (wc.xw) {
        const u64 xa = xlook64(wc.xw, a);
        mm1 |= xa | xlook64(wc.xw, p1);
        mm2 |= xa | xlook64(wc.xw, p2);
    }
    bool rep = d1 && win_has_period(wc, a, k, d1, mm1);
    if (!rep && d2) rep = win_has_period(wc, a, k, d2, mm2);
    if (!rep && d3) rep = win_has_period(wc, a, k, d3, win_mismatch64(wc, a, d3));  // a third prime: k = 30, 42, 60, ...
    if (!rep && (lo >> 31)) {  // a fourth: k >= 210
        const u32 d4 = wc.cof[k] >> 24;
        rep = win_has_period(wc, a, k, d4, win_mismatch64(wc, a, d4));
    }
    if (rep) return;
    u64 b;
    if (e != LEAD_NO_END) {
        b = wc.win0 + ge + e;
    } else {
        u32 from = q32;
        if (!win_run_end(wc, from, k, b)) {
            defer(tc, wc.win0 + a, k, 0u, 0u, 0u, wc.win0 + from);
            return;
        }
    }
    if (b - (wc.win0 + a) < (u64)min_matches32(k, wc.min_repeats, wc.min_span)) return;
    emit_row(tc, wc.win0 + a, b, k);
}

// Boundary pass.  A group task's run is found at the FIRST examined all-match group it contains.  For a run that starts
// in the last 8S-1 positions of this tile that group lies in the next tile, whose workgroup drops the run because it does
// not start there; this tile reports it: per motif size one look at the 32 positions in front of the
// tile's end.  c = matches directly in front of the end: 1 <= c < 8S <=> such a run exists and starts at end - c.
__device__ __forceinline__ void boundary_item(const TileCtx &tc, const WinCtx &wc, u32 k, u32 S) {
    const u64 tile_end = tc.tile_base + PRF_TILE;
    const u32 back = 8u * S;
    const u64 mm = win_mismatch64(wc, WIN_LEAD + PRF_TILE - 32u, k);
    const u32 lo = (u32)mm;  // bit i = mismatch at tile_end - 32 + i
    const u32 c = lo ? (u32)__builtin_clz(lo) : 32u;
    if (c == 0 || c >= back) return;
    const u64 a = tile_end - c;
    const u64 hi = mm >> 32;  // bit i = mismatch at tile_end + i
    u64 b;
    if (hi) {
        b = tile_end + (u64)__builtin_ctzll(hi);
    } else {
        u32 from = WIN_LEAD + PRF_TILE + 32u;
        if (!win_run_end(wc, from, k, b)) {
            defer(tc, a, k, 0u, 0u, 1u, wc.win0 + from);
            return;
        }
    }
    if (b - a < (u64)min_matches32(k, tc.min_repeats, tc.min_span)) return;
    static_assert(WIN_LEAD + PRF_TILE + 2u * PRF_VMAX_K + 96u <= WIN_POS, "the motif of a boundary item lies inside the window");
    if (!win_motif_is_repeat(wc, WIN_LEAD + PRF_TILE - c, k)) emit_row(tc, a, b, k);
}

// the same by the general routine (a tile that is verified again, see defer())
__device__ __forceinline__ void boundary_general(const TileCtx &tc, u32 k, u32 S) {
    const u64 tile_end = tc.tile_base + PRF_TILE;
    const u32 back = 8u * S;
    const u64 mm = tile_mismatch64(tile_end - 32, k);
    const u32 lo = (u32)mm;
    const u32 c = lo ? (u32)__builtin_clz(lo) : 32u;
    if (c == 0 || c >= back) return;
    const u64 a = tile_end - c;
    const u64 hi = mm >> 32;
    const u64 b = hi ? tile_end + (u64)__builtin_ctzll(hi) : run_end(tile_end + 32, k);
    if (b - a < (u64)min_matches32(k, tc.min_repeats, tc.min_span)) return;
    if (!motif_is_repeat(a, k)) emit_row(tc, a, b, k);
}

__device__ __forceinline__ prf_lds_u32 *smem_cnt(u32 parity) { return (prf_lds_u32 *)(prf_smem + HDR_CNT) + CNT_N * parity; }

// Candidates -> rows, all waves together once the window is staged.
//  * exact tasks left ONE ballot-compacted list of (stream, task) flags in LDS, dealt to the threads from thread 0 up;
//  * group-task records (one list) are taken by the upper two waves, alternately; the boundary items by the lower half, from
//    its last thread down.
__device__ __forceinline__ void verify_all(prf_lds_cu64 *recs, u32 n_recs, prf_lds_cu32 *bitems, u32 n_bitems, const unsigned short __attribute__((address_space(3))) *flags,
                                           u32 n_flags, const u32 *xw, u32 tid, u64 *dbg) {
#ifdef PRF_STAMPS
#define PRF_VSTAMP(i) do { if (dbg && (tid & 63u) == 0) dbg[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PRF_VSTAMP(i) do { } while (0)
#endif
    const TileCtx &tc = *reinterpret_cast<const TileCtx *>(prf_smem);
    WinCtx wc;
    wc.h = (prf_lds_cu32 *)(prf_smem + tc.lin_off);
    wc.l = wc.h + 2 * LW;
    wc.xw = xw;
    wc.cof = (prf_lds_cu32 *)(prf_smem + tc.cof_off);
    wc.win0 = tc.tile_base - WIN_LEAD;
    wc.min_repeats = tc.min_repeats;
    wc.min_span = tc.min_span;
    // The two halves of the workgroup run different code side by side: a pass over the group-task records (upper half) takes
    // about as long as two passes over the flags plus one over the boundary items (lower half); a wave's pass costs the same
    // with 1 or 64 candidates.
    if (tid >= (u32)NTH / 2u) {
        // ---- group-task records, alternating between the two waves.  A record's word has a bit per flagged stream, and a loop
        // over a lane's own bits runs as often as the wave's unluckiest lane has bits.  So each wave first lists its flagged streams
        // (stage A: a prefix sum of the lanes' bit counts, no look), then takes them one per lane from lane 0 up (stage B).  No
        // barrier between the stages: a wave's LDS operations are carried out in the order it issues them, so stage B's reads of
        // the wave's list follow stage A's writes to it, whichever lanes they come from (the fences only keep the compiler from
        // moving them).  Every loop that holds a look is wave-uniform: lanes without work are masked.
        const u32 up = (u32)NTH - 1u - tid;  // 0 .. 127: thread 255, 254, ...
        const u32 hwl = tid & 63u;
        prf_lds_u32 *list = (prf_lds_u32 *)(prf_smem + LEAD_OFF) + (up >> 6) * LEAD_CAP;
        u32 idx = 2u * (up & 63u) + (up >> 6), word = 0, head = 0;
        for (;;) {  // one round, unless the wave has more flagged streams than its list holds
            u32 n_items = 0;  // wave-uniform
            bool more;
            // ---- stage A: (stream, k, stride code) of every flagged stream -> the wave's list; a lane's streams lie together
            for (;;) {
                if (word == 0u && idx < n_recs) {
                    const u64 rec = recs[idx];
                    idx += (u32)NTH / 2u;
                    head = (u32)rec & 0x1FFFFu;  // lane, k, stride code
                    word = (u32)(rec >> 17);
                }
                const u32 pc = (u32)__builtin_popcount(word);
                u32 at = n_items, total = 0;
#pragma unroll
                for (u32 b = 0; b < 6u; b++) {  // (pc <= 32)
                    const u64 bal = __builtin_amdgcn_ballot_w64(((pc >> b) & 1u) != 0);
                    at += __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0)) << b;
                    total += (u32)__builtin_popcountll(bal) << b;
                }
                u32 room = at < LEAD_CAP ? LEAD_CAP - at : 0u;  // (a lane keeps the streams that do not fit for the next round)
                for (; word && room; room--) {
                    const u32 bit = (u32)__builtin_ctz(word);
                    word &= word - 1;
                    list[at++] = (bit * 64u + (head & 63u)) | ((head >> 6) << 11);
                }
                n_items = n_items + total < LEAD_CAP ? n_items + total : LEAD_CAP;
                more = __builtin_amdgcn_ballot_w64(word != 0u || idx < n_recs) != 0ull;
                if (!more || n_items == LEAD_CAP) break;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            PRF_VSTAMP(14);
            // ---- stage B: one listed stream per lane: one look says which of its groups are leaders; then leader by leader
            // (almost always one per stream)
            for (u32 i0 = 0; i0 < n_items; i0 += 64u) {
                u32 leaders = 0, nbs = 0, far = 0, cof_k = 0, q = 0, k = 0;
                u64 m = 0;
                if (i0 + hwl < n_items) {
                    const u32 it = list[i0 + hwl], sq = (it & 2047u) * T, sc = (it >> 20) & 3u;
                    k = (it >> 11) & 511u;
                    q = WIN_LEAD + sq;
                    if (sq >= 32u || xw) {
                        // bit i = mismatch at window position q - 32 + i; one round trip with the cofactors
                        prf_u32x3 r0 = raw64(wc.h, q - 32u), r1 = raw64(wc.l, q - 32u), r2 = raw64(wc.h, q - 32u + k), r3 = raw64(wc.l, q - 32u + k);
                        cof_k = wc.cof[k];
                        asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(cof_k));
                        m = (cut64(r0, q - 32u) ^ cut64(r2, q - 32u + k)) | (cut64(r1, q - 32u) ^ cut64(r3, q - 32u + k));
                        if (xw) m |= xlook64(xw, q - 32u) | xlook64(xw, q - 32u + k);
                        leaders = win_leaders(wc, q, k, 1u << (sc - 1u), m, nbs, far);
                        while (far) {  // (the group itself is known to match)
                            const u32 j = (u32)__builtin_ctz(far);
                            far &= far - 1;
                            defer(tc, wc.win0 + (q + 8u * j - ((nbs >> (5u * j)) & 31u)), k, 0u, 0u, 1u, wc.win0 + (q + 8u * j + 8u));
                        }
                    } else {
                        defer(tc, tc.tile_base, k, sc, 1u, 0u, 0ull);  // (a clean tile's first stream: see the flags below)
                    }
                }
                while (__builtin_amdgcn_ballot_w64(leaders != 0u) != 0ull) {
                    if (leaders) {
                        const u32 j = (u32)__builtin_ctz(leaders);
                        leaders &= leaders - 1;
                        win_verify_leader(tc, wc, make_leader(q, k, cof_k, j, (nbs >> (5u * j)) & 31u, m));
                    }
                }
            }
            if (!more) break;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    } else {
        // ---- exact tasks' flags: (lane, stream bit, task), dealt to the threads one by one: a wave runs the body once per 64
        // flags, not as often as its unluckiest lane has flags
        for (u32 idx = tid; idx < n_flags; idx += (u32)NTH / 2u) {
            const u32 f = flags[idx], frl = f & 63u, fbit = (f >> 6) & 31u, k = tc.k_exact0 + (f >> 11);
            // (a clean tile's first stream looks at positions in front of the tile, where N is possible and nothing says so
            // in the window: general routine, later)
            if ((frl | fbit) || xw) win_verify_flag(tc, wc, frl, fbit, k);
            else defer(tc, tc.tile_base, k, 0u, 1u, 0u, 0ull);
        }
        PRF_VSTAMP(14);
        // ---- boundary items: from the half's last thread down (the last round of flags fills it from the first thread up)
        for (u32 idx = (u32)NTH / 2u - 1u - tid; idx < n_bitems; idx += (u32)NTH / 2u) {
            const u32 it = bitems[idx];
            boundary_item(tc, wc, it & 0xFFFFu, it >> 16);
        }
    }
}

// A tile with more deferred candidates than their list holds: everything again, by the general routine alone (the rows the
// first attempt listed have been dropped by the caller).  Cold code: not inlined.
__device__ __noinline__ void verify_general(prf_lds_cu64 *recs, u32 n_recs, prf_lds_cu32 *bitems, u32 n_bitems,
                                            const unsigned short __attribute__((address_space(3))) *flags, u32 n_flags, u32 tid) {
    const TileCtx &tc = *reinterpret_cast<const TileCtx *>(prf_smem);
    for (u32 idx = tid; idx < n_flags; idx += (u32)NTH) {
        const u32 f = flags[idx], frl = f & 63u, fbit = (f >> 6) & 31u, k = tc.k_exact0 + (f >> 11);
        verify_stream(tc.tile_base + (u64)(fbit * 64u + frl) * T, k, 0u);
    }
    for (u32 idx = tid; idx < n_recs; idx += (u32)NTH) {
        const u64 rec = recs[idx];
        const u32 rl = (u32)rec & 63u, k = ((u32)rec >> 6) & 511u, sc = ((u32)rec >> 15) & 3u;
        u32 word = (u32)(rec >> 17);
        while (word) {
            const u32 bit = (u32)__builtin_ctz(word);
            word &= word - 1;
            verify_stream(tc.tile_base + (u64)(bit * 64u + rl) * T, k, sc);
        }
    }
    for (u32 idx = tid; idx < n_bitems; idx += (u32)NTH) {
        const u32 it = bitems[idx];
        boundary_general(tc, it & 0xFFFFu, it >> 16);
    }
}
