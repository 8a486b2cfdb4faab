// scan_interrupted.hip -- interrupted repeats (the reference's RepeatTracker with max_interruptions > 0), DESIGN 9.
//
// The tracker walks left to right but jumps back to its first interruption after every decision, so a literal replay walks
// each position many times.  Its path does not depend on the shared dictionary or on its previous output, so the work splits:
//   1. the walk, one lane per (sequence, k, chunk of landing positions): the tracker's path, appending a candidate (start,
//      end, phase mask, homopolymer) at every output check that passes both span tests with no N in the motif.  Every jump back
//      lands clean on the next boundary (a mismatch right behind a match), so a lane that starts clean on the first
//      boundary of its chunk and stops at the first landing behind it walks a piece of the whole walk.  prf_int_walk_kernel
//      (one lane per thread, one chunk per (sequence, k)) and prf_int_walk_chunk_kernel (one lane per wave) share walk_lane().
//      A memo table of states (position, run, phase set) recorded every `stride` positions lets an episode that meets a state an earlier episode
//      passed through take that episode's outcome and jump at once (exact: inside an episode the path depends on the state
//      only; the first interruption picks the jump target and nothing else).
//   2. prf_int_emit_kernel, one lane per sequence: the dictionary (an open-addressing hash of (start, end)), the
//      previous-output rule and the homopolymer rule, k in ascending order.
//   3. prf_int_sort_rows: the rows sorted by (contig, start, end) with three stable radix passes.
#include "prf_host.h"

#include <hipcub/hipcub.hpp>

namespace {

typedef long long i64;

constexpr u32 OUT_PENDING = 0xffffffffu;  // episode outcome words: pending, or
constexpr u32 OUT_END = 0x80000000u;      //   the walk ended in this episode (done())
constexpr u32 OUT_NONE = 0x40000000u;     //   no candidate; otherwise the low 30 bits index the lane's candidate list
constexpr u32 OUT_IDX = 0x3fffffffu;

// one aligned 8-byte word per stream, reloaded when the position leaves it (the walk is sequential between jumps)
struct word_cache {
    i64 blk;
    u64 w;
};
__device__ __forceinline__ u32 cbyte(const uint8_t *__restrict__ base, i64 a, word_cache &c) {
    const i64 blk = a >> 3;
    if (blk != c.blk) {
        c.blk = blk;
        c.w = *reinterpret_cast<const u64 *>(base + (blk << 3));
    }
    return (u32)(c.w >> ((a & 7) << 3)) & 0xffu;
}

__host__ __device__ __forceinline__ u64 memo_slot(u64 pos, u64 run, u64 mask, u64 slots) {
    u64 h = pos * 0x9E3779B97F4A7C15ull + run * 0xC2B2AE3D27D4EB4Full + mask * 0x165667B19E3779F9ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return (h >> 32) % slots;
}

// One lane: the walk of (sequence, k) restricted to the landings in [ln.lo, ln.hi).  lane_end[li] = 1 if the walk ended in one
// of this lane's episodes (at the end of the sequence).  first_end (may be NULL): per (sequence, k) the smallest chunk whose lane
// ended; a lane behind that chunk is dropped by the host and stops when it sees so (polled every 64 positions).
// The budget of varying phases is the lane's own (prf_ilane::max_int); 0: no phase is ever added, the first
// interruption is still recorded and the reset still jumps to it.
// SKIP_ABSORBED: a run whose phase set holds all k phases (k <= the lane's max_int) absorbs every mismatch, so it only ends with the sequence:
// the lane moves to n - k at once, counting the moves it did not make (the memo records of that stretch are not written, so the
// lookup and hit counters differ from a walk that makes them; the one-lane engine keeps making them).
template <bool SKIP_ABSORBED>
__device__ __forceinline__ void walk_lane(const uint8_t *__restrict__ buf, const prf_ilane *__restrict__ lanes, u32 li,
                                          const u64 *__restrict__ first_last, u32 min_repeats, u32 min_span, u32 stride,
                                          prf_icand *__restrict__ cands, u64 *__restrict__ cand_cnt, u32 *__restrict__ lane_end,
                                          u32 *__restrict__ first_end, prf_imemo *__restrict__ memo, u32 *__restrict__ eps,
                                          u64 *__restrict__ counters) {
    const prf_ilane ln = lanes[li];
    const u64 f0 = first_last[2 * ln.seq], f1 = first_last[2 * ln.seq + 1];
    const i64 head = f0 == ~0ull ? 0 : (i64)f0;
    const i64 n = f0 == ~0ull ? 0 : (i64)(f1 - f0);
    const uint8_t *__restrict__ base = buf + ln.seq_base;  // 16-byte aligned; position p of the trimmed sequence is base[head + p]
    const i64 k = ln.k;
    const u32 max_int = ln.max_int;
    const i64 span = min_span, r_span = (i64)min_repeats * k;
    prf_icand *__restrict__ my_cands = cands + ln.cand_off;
    prf_imemo *__restrict__ my_memo = memo + ln.memo_off;
    u32 *__restrict__ my_eps = eps + ln.ep_off;
    const bool use_memo = stride != 0 && ln.memo_slots != 0 && ln.ep_cap != 0;

    i64 pos = 0, run = 0, first = -1;
    u64 mask = 0;
    u32 n_int = 0;
    u64 n_cand = 0, steps = 0, lookups = 0, hits = 0, n_ep = 0;
    bool rec_ep = false;  // the current episode has an outcome word
    word_cache ca{-1, 0}, cb{-1, 0};
    const i64 hi = (i64)ln.hi;
    const u64 full_mask = k >= 64 ? ~0ull : (1ull << k) - 1ull;
    u32 *__restrict__ my_end = (first_end && ln.chunk > 0) ? first_end + ln.kslot : nullptr;
    u32 ended = 0;

    if (ln.lo > 0) {  // the first boundary >= lo: q + 1 with match(q - 1) and not match(q), 1 <= lo - 1 <= q < n - k
        i64 q = (i64)ln.lo - 1;
        bool found = false;
        bool prev = q < n - k && cbyte(base, head + q - 1, ca) == cbyte(base, head + q - 1 + k, cb);
        for (; q < n - k && q + 1 < hi; q++) {
            const bool m = cbyte(base, head + q, ca) == cbyte(base, head + q + k, cb);
            if (prev && !m) {
                found = true;
                break;
            }
            prev = m;
        }
        if (!found) {  // no landing in [lo, hi): nothing to walk
            cand_cnt[li] = 0;
            lane_end[li] = 0;
            return;
        }
        pos = q + 1;
    }

    auto open_ep = [&]() {
        rec_ep = use_memo && n_ep < ln.ep_cap;
        if (rec_ep) my_eps[n_ep++] = OUT_PENDING;
    };
    auto close_ep = [&](u32 out) {
        if (rec_ep) my_eps[n_ep - 1] = out;
        rec_ep = false;
    };
    auto push = [&](const prf_icand &c) -> u32 {
        if (n_cand < ln.cand_cap) my_cands[n_cand] = c;
        return (u32)(n_cand++ & OUT_IDX);
    };

    open_ep();
    for (;;) {
        if (use_memo && ((u64)pos & (stride - 1u)) == 0) {  // stride: a power of two
            prf_imemo *rec = my_memo + memo_slot((u64)pos, (u64)run, mask, ln.memo_slots);
            if (first >= 0) {
                lookups++;
                const prf_imemo m = *rec;
                if (m.pos == (u64)pos && m.run == (u64)run && m.mask == mask) {
                    const u32 out = my_eps[m.ep];
                    if (out != OUT_PENDING) {
                        hits++;
                        if (!(out & OUT_NONE)) {
                            const u64 src = out & OUT_IDX;
                            if (src < ln.cand_cap) push(my_cands[src]);
                            else n_cand++;  // an overflowing attempt only counts
                        }
                        close_ep(out);
                        if (out & OUT_END) {
                            ended = 1;
                            break;
                        }
                        if (first + 1 >= hi) break;  // the next lane's first landing
                        pos = first + 1;
                        first = -1;
                        run = 0;
                        mask = 0;
                        n_int = 0;
                        open_ep();
                        continue;
                    }
                }
            }
            if (rec_ep) *rec = prf_imemo{(u64)pos, mask, (u64)run, n_ep - 1};
        }
        if (my_end && ((u64)pos & 63u) == 0 && __atomic_load_n(my_end, __ATOMIC_RELAXED) < ln.chunk) break;  // dropped anyway

        if (SKIP_ABSORBED && run > 0 && mask == full_mask && pos < n - k) {
            const i64 d = n - k - pos;
            steps += (u64)d;
            run += d;
            pos += d;
        }
        const bool at_end = pos >= n - k;  // advance() returns False
        if (!at_end) {
            steps++;
            if (cbyte(base, head + pos, ca) == cbyte(base, head + pos + k, cb)) {
                run++;
                pos++;
                continue;
            }
            if (run > 0) {
                if (first < 0) first = pos;
                const u32 ph = (u32)(run % k);
                if (n_int < max_int && !((mask >> ph) & 1ull)) {
                    mask |= 1ull << ph;
                    n_int++;
                }
                if ((mask >> ph) & 1ull) {
                    run++;
                    pos++;
                    continue;
                }
            }
        }

        // output_interval_if_it_passes_filters()
        if (run + k < span || run + k < r_span) {  // returns without reset_traversal(): first interruption and phase set stay
            if (at_end) {
                close_ep(OUT_END | OUT_NONE);
                ended = 1;
                break;
            }
            run = 0;
            pos++;
            continue;
        }
        u32 out = OUT_NONE;
        const i64 start = pos - run;  // run >= (min_repeats - 1) * k >= k: start + k <= pos, pos - k >= start
        bool has_n = false;
        for (i64 t = 0; t < k; t++) has_n |= base[head + start + t] == 'N';
        if (!has_n) {
            while (pos < n && (base[head + pos] == base[head + pos - k] || ((mask >> (u32)(run % k)) & 1ull))) {
                run++;
                pos++;
                steps++;
            }
            if (run >= span && run >= r_span) {
                // a homopolymer once the varying phases are N (k > 1, one distinct base among the others)
                int b0 = -1;
                bool homo = k > 1;
                for (i64 t = 0; t < k && homo; t++) {
                    if ((mask >> t) & 1ull) continue;
                    const int b = base[head + start + t];
                    if (b0 < 0) b0 = b;
                    else if (b != b0) homo = false;
                }
                homo = homo && b0 >= 0;
                out = push(prf_icand{(u64)start, (u64)pos, mask, homo ? 1u : 0u, (u32)k});
            }
        }
        close_ep(out | (at_end ? OUT_END : 0u));
        if (at_end) {
            ended = 1;
            break;
        }
        if (first >= 0) pos = first;  // reset_traversal()
        if (pos + 1 >= hi) break;     // the next lane's first landing
        first = -1;
        run = 0;
        mask = 0;
        n_int = 0;
        pos++;
        open_ep();
    }
    cand_cnt[li] = n_cand;
    lane_end[li] = ended;
    if (ended && first_end) atomicMin(first_end + ln.kslot, ln.chunk);
    atomicAdd(counters + 0, steps);
    atomicAdd(counters + 1, lookups);
    atomicAdd(counters + 2, hits);
    atomicAdd(counters + 3, n_ep);
}

__global__ void __launch_bounds__(64) prf_int_walk_kernel(const uint8_t *__restrict__ buf, const prf_ilane *__restrict__ lanes,
                                                          u32 n_lanes, const u64 *__restrict__ first_last, u32 min_repeats,
                                                          u32 min_span, u32 stride, prf_icand *__restrict__ cands,
                                                          u64 *__restrict__ cand_cnt, u32 *__restrict__ lane_end,
                                                          prf_imemo *__restrict__ memo, u32 *__restrict__ eps,
                                                          u64 *__restrict__ counters) {
    const u32 li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n_lanes) return;
    walk_lane<false>(buf, lanes, li, first_last, min_repeats, min_span, stride, cands, cand_cnt, lane_end, nullptr, memo, eps, counters);
}

// One lane per wave (the first thread of each 64-thread workgroup): a lane is a chain of dependent loads, and lanes that share a
// wave pay for each other's branches (every trip round the loop then waits for some lane's memo record).  The gain is in the
// number of waves in flight, so the other 63 threads stay idle.
__global__ void __launch_bounds__(64) prf_int_walk_chunk_kernel(const uint8_t *__restrict__ buf, const prf_ilane *__restrict__ lanes,
                                                                u32 n_lanes, const u64 *__restrict__ first_last, u32 min_repeats,
                                                                u32 min_span, u32 stride, prf_icand *__restrict__ cands,
                                                                u64 *__restrict__ cand_cnt, u32 *__restrict__ lane_end,
                                                                u32 *__restrict__ first_end, prf_imemo *__restrict__ memo,
                                                                u32 *__restrict__ eps, u64 *__restrict__ counters) {
    const u32 li = blockIdx.x;
    if (li >= n_lanes || threadIdx.x != 0) return;
    walk_lane<true>(buf, lanes, li, first_last, min_repeats, min_span, stride, cands, cand_cnt, lane_end, first_end, memo, eps, counters);
}

// boundaries of each lane's chunk (an upper bound of its episodes, hence of its candidates): one workgroup per lane
__global__ void __launch_bounds__(256) prf_int_bound_kernel(const uint8_t *__restrict__ buf, const prf_ilane *__restrict__ lanes,
                                                            const u64 *__restrict__ first_last, u64 *__restrict__ bcount) {
    const u32 li = blockIdx.x;
    const prf_ilane ln = lanes[li];
    const u64 f0 = first_last[2 * ln.seq], f1 = first_last[2 * ln.seq + 1];
    if (f0 == ~0ull) return;
    const i64 n = (i64)(f1 - f0), k = ln.k;
    const uint8_t *__restrict__ s = buf + ln.seq_base + f0;
    const i64 q0 = ln.lo > 1 ? (i64)ln.lo - 1 : 1;                                  // q + 1 in [lo, hi), 1 <= q < n - k
    const i64 q1 = (i64)ln.hi - 1 < n - k ? (i64)ln.hi - 1 : n - k;
    u64 cnt = 0;
    for (i64 q = q0 + threadIdx.x; q < q1; q += blockDim.x) cnt += (s[q - 1] == s[q - 1 + k]) && (s[q] != s[q + k]);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(bcount + li, cnt);
}

__device__ __forceinline__ u64 key_hash(u64 a, u64 b) {
    u64 h = a * 0x9E3779B97F4A7C15ull ^ (b + 0x632BE59BD9B4E019ull) * 0xC2B2AE3D27D4EB4Full;
    return h ^ (h >> 31);
}

// lanes of sequence s: lane0[s] + j * n_chunks[s] + c for motif size j and chunk c; the chunks behind the first lane that ended
// hold landings the walk never reaches and are dropped
__global__ void __launch_bounds__(64) prf_int_emit_kernel(const prf_ilane *__restrict__ lanes, u32 nk, u32 n_seq,
                                                          const u32 *__restrict__ lane0, const u32 *__restrict__ n_chunks,
                                                          const u32 *__restrict__ lane_end,
                                                          const prf_icand *__restrict__ cands, const u64 *__restrict__ cand_cnt,
                                                          const u64 *__restrict__ first_last, const u64 *__restrict__ hash_off,
                                                          const u64 *__restrict__ hash_size, u64 *__restrict__ keys,
                                                          prf_ihit_dev *__restrict__ rows, u64 *__restrict__ row_cnt) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seq) return;
    const u64 head = first_last[2 * s] == ~0ull ? 0 : first_last[2 * s];
    u64 *__restrict__ tab = keys + 2 * hash_off[s];
    const u64 hmask = hash_size[s] - 1;  // a power of two, at least twice the candidates of the sequence
    const u32 nc = n_chunks[s];
    for (u32 j = 0; j < nk; j++) {
        bool have_prev = false, have_last = false;
        u64 prev_end = 0;
        prf_icand last{};
        bool ended = false;
        for (u32 ch = 0; ch < nc && !ended; ch++) {
            const u32 li = lane0[s] + j * nc + ch;
            const prf_ilane ln = lanes[li];
            const u64 cnt = cand_cnt[li];
            const i64 k = ln.k;
            ended = lane_end[li] != 0;
            for (u64 i = 0; i < cnt; i++) {
                const prf_icand c = cands[ln.cand_off + i];
                // a candidate equal to the one before it can never change the result
                if (have_last && c.start == last.start && c.end == last.end && c.mask == last.mask) continue;
                last = c;
                have_last = true;
                if (c.homo) continue;
                if (have_prev && (i64)(c.end - prev_end) < k) continue;
                u64 slot = key_hash(c.start, c.end) & hmask;
                bool seen = false;
                for (;;) {
                    const u64 e = tab[2 * slot + 1];
                    if (e == 0) break;  // empty (every end is >= 1)
                    if (e == c.end && tab[2 * slot] == c.start) {
                        seen = true;
                        break;
                    }
                    slot = (slot + 1) & hmask;
                }
                if (seen) continue;
                tab[2 * slot] = c.start;
                tab[2 * slot + 1] = c.end;
                const u64 at = atomicAdd(row_cnt, 1ull);
                rows[at] = prf_ihit_dev{c.start + head, c.end + head, (u32)k, s, c.mask};
                prev_end = c.end;
                have_prev = true;
            }
        }
    }
}

// first / one-past-last position that is not N of every sequence (upper-cased bytes), one thread per chunk:
// chunks[3c .. 3c+2] = (sequence, first position, one past the last position), the first position a multiple of 8
__global__ void prf_int_trim_kernel(const uint8_t *__restrict__ buf, const u64 *__restrict__ seq_base, const u64 *__restrict__ chunks,
                                    u32 n_chunks, u64 *__restrict__ first_last) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const u64 seq = chunks[3 * c], b = chunks[3 * c + 1], e = chunks[3 * c + 2];
    const uint8_t *__restrict__ s = buf + seq_base[seq];  // 16-byte aligned
    u64 lo = ~0ull, hi = 0;
    u64 p = b;
    for (; p + 8 <= e; p += 8) {
        const u64 w = *reinterpret_cast<const u64 *>(s + p) ^ 0x4E4E4E4E4E4E4E4Eull;  // a zero byte is an N
        if (w == 0) continue;
        u64 nz = w;  // bit 8i set <=> byte i is not N
        nz |= nz >> 4;
        nz |= nz >> 2;
        nz |= nz >> 1;
        nz &= 0x0101010101010101ull;
        if (lo == ~0ull) lo = p + (u64)(__builtin_ctzll(nz) >> 3);
        hi = p + (u64)((63 - __builtin_clzll(nz)) >> 3) + 1;
    }
    for (; p < e; p++) {
        if (s[p] != 'N') {
            if (lo == ~0ull) lo = p;
            hi = p + 1;
        }
    }
    if (lo != ~0ull) {
        atomicMin(first_last + 2 * seq, lo);
        atomicMax(first_last + 2 * seq + 1, hi);
    }
}

__global__ void prf_int_key_kernel(const prf_ihit_dev *__restrict__ rows, u64 n, const u32 *__restrict__ idx, int field,
                                   u64 *__restrict__ key, u32 *__restrict__ idx_out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 j = idx ? idx[i] : (u32)i;
    const prf_ihit_dev r = rows[j];
    key[i] = field == 0 ? r.end : field == 1 ? r.start : (u64)r.contig;
    if (!idx) idx_out[i] = (u32)i;
}

__global__ void prf_int_gather_kernel(const prf_ihit_dev *__restrict__ rows, u64 n, const u32 *__restrict__ idx,
                                      prf_ihit_dev *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rows[idx[i]];
}

}  // namespace

hipError_t prf_launch_int_trim(hipStream_t st, const uint8_t *buf, const u64 *seq_base, const u64 *chunks, u32 n_chunks,
                               u64 *first_last) {
    if (!n_chunks) return hipSuccess;
    hipLaunchKernelGGL(prf_int_trim_kernel, dim3((n_chunks + 255) / 256), dim3(256), 0, st, buf, seq_base, chunks, n_chunks, first_last);
    return hipGetLastError();
}

hipError_t prf_launch_int_walk(hipStream_t st, const prf_int_walk_args &a) {
    const prf_int_lanes &l = a.l;
    if (!l.n_lanes) return hipSuccess;
    if (a.first_end)
        hipLaunchKernelGGL(prf_int_walk_chunk_kernel, dim3(l.n_lanes), dim3(64), 0, st, a.buf, l.lanes, l.n_lanes, l.first_last,
                           a.min_repeats, a.min_span, a.stride, l.cands, l.cand_cnt, l.lane_end, a.first_end, a.memo, a.eps,
                           a.counters);
    else
        hipLaunchKernelGGL(prf_int_walk_kernel, dim3((l.n_lanes + 63) / 64), dim3(64), 0, st, a.buf, l.lanes, l.n_lanes, l.first_last,
                           a.min_repeats, a.min_span, a.stride, l.cands, l.cand_cnt, l.lane_end, a.memo, a.eps, a.counters);
    return hipGetLastError();
}

hipError_t prf_launch_int_bound(hipStream_t st, const uint8_t *buf, const prf_ilane *lanes, u32 n_lanes, const u64 *first_last,
                                u64 *bcount) {
    if (!n_lanes) return hipSuccess;
    hipLaunchKernelGGL(prf_int_bound_kernel, dim3(n_lanes), dim3(256), 0, st, buf, lanes, first_last, bcount);
    return hipGetLastError();
}

hipError_t prf_launch_int_emit(hipStream_t st, const prf_int_emit_args &a) {
    const prf_int_lanes &l = a.l;
    if (!a.n_seq) return hipSuccess;
    hipLaunchKernelGGL(prf_int_emit_kernel, dim3((a.n_seq + 63) / 64), dim3(64), 0, st, l.lanes, a.nk, a.n_seq, a.lane0, a.n_chunks,
                       l.lane_end, l.cands, l.cand_cnt, l.first_last, a.hash_off, a.hash_size, a.keys, a.rows, a.row_cnt);
    return hipGetLastError();
}

size_t prf_int_sort_scratch_bytes(u64 n) {
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (u64 *)nullptr, (u64 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (int)n, 0, 64);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    return 2 * up(n * 8) + 2 * up(n * 4) + up(t) + 256;
}

// rows[0..n) -> out[0..n) sorted by (contig, start, end): three stable radix passes over row indices, then a gather.
// scratch: prf_int_sort_scratch_bytes(n) bytes of device memory.
hipError_t prf_int_sort_rows(hipStream_t st, const prf_ihit_dev *rows, u64 n, prf_ihit_dev *out, void *scratch) {
    if (n == 0) return hipSuccess;
    if (n > 0x7fffffffull) return hipErrorInvalidValue;
    const int ni = (int)n;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    char *p = (char *)scratch;
    u64 *key_a = (u64 *)p;
    u64 *key_b = (u64 *)(p + up(n * 8));
    u32 *idx_a = (u32 *)(p + 2 * up(n * 8));
    u32 *idx_b = (u32 *)(p + 2 * up(n * 8) + up(n * 4));
    void *tmp = p + 2 * up(n * 8) + 2 * up(n * 4);
    size_t tmp_bytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, key_a, key_b, idx_a, idx_b, ni, 0, 64, st);
    if (e != hipSuccess) return e;
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(prf_int_key_kernel, dim3(nb), dim3(256), 0, st, rows, n, (const u32 *)nullptr, 0, key_a, idx_a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t b = tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(tmp, b, key_a, key_b, idx_a, idx_b, ni, 0, 64, st)) != hipSuccess) return e;  // end
    hipLaunchKernelGGL(prf_int_key_kernel, dim3(nb), dim3(256), 0, st, rows, n, idx_b, 1, key_a, (u32 *)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    b = tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(tmp, b, key_a, key_b, idx_b, idx_a, ni, 0, 64, st)) != hipSuccess) return e;  // start
    hipLaunchKernelGGL(prf_int_key_kernel, dim3(nb), dim3(256), 0, st, rows, n, idx_a, 2, key_a, (u32 *)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    b = tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(tmp, b, key_a, key_b, idx_a, idx_b, ni, 0, 32, st)) != hipSuccess) return e;  // contig
    hipLaunchKernelGGL(prf_int_gather_kernel, dim3(nb), dim3(256), 0, st, rows, n, idx_b, out);
    return hipGetLastError();
}
