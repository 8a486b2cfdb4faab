// interrupted.cpp -- the host path of the interrupted repeats (prf_scan_interrupted*; kernels: scan_interrupted.hip).
//
// Every entry point is prf_scan_interrupted_by_k: a budget of varying phases per motif size.  The older ones hand
// it the same budget for every motif size and keep their refusal of 0.
// Whole sequences, one call, in stages that each hand a named struct to the next (interrupted_scan runs them):
//   check_args       the refusals, parameters first
//   stage_sequences  placement, upload, upper-casing (+ the first byte that is not a letter), N-trimming -> first_last
//   lay_out_lanes    the lanes in (sequence, k, chunk) order from the trimmed lengths, their memo tables     (host only)
//   size_walk_room   candidate and episode room per lane: its boundary count, or len / 4 with one lane per (sequence, k)
//   walk             the walk kernel, run again with the exact counts if a candidate list was too small
//   drop_unreached   the chunks behind the first lane of a (sequence, k) that ended                          (host only)
//   size_hashes      one hash of emitted (start, end) per sequence, from the candidate counts                (host only)
//   emit_and_sort    emission, sort, the rows to the host
// The host-only stages take and return host vectors, make no HIP call and see no context: tests/interrupted_chunks_model.py
// restates their arithmetic (n_chunks, lane_count, the drop rule).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "prf_ctx.h"

namespace {

struct int_params {
    u32 kmin, kmax, min_repeats, min_span, memo_stride;
    u64 memo_slots;
    // 0: one lane per (sequence, k), one lane per thread (prf_scan_interrupted_ex).  Otherwise the landings of each (sequence, k)
    // are cut into chunks of `chunk` positions, one lane per wave.
    u64 chunk;
    // the budget of varying phases per motif size: by_k[j] for k = kmin + j (the caller's array, read during the call only), or
    // `uniform` for every k where an older entry point gave one number (by_k == NULL, uniform_call)
    const u32 *by_k;
    u32 uniform;
    bool uniform_call;
    u32 nk() const { return kmax - kmin + 1; }
    u32 max_int(u32 j) const { return uniform_call ? uniform : by_k[j]; }
};

// the timing events of one call, each recorded once
struct int_events {
    hipEvent_t begin, walk_begin, walk_end, emit_begin, end;
};

// words of the call's counter block on the device
enum { CTR_BADPOS = 0, CTR_WALK = 1 /* steps, memo lookups, memo hits, recorded episodes */, CTR_ROWS = 5, CTR_N = 8 };

struct staged_seqs {
    std::vector<u64> base, len;   // per sequence: its byte offset in d_buf (16-byte aligned, 16 readable bytes behind it), its length
    std::vector<u64> first_last;  // per sequence: first / one-past-last position that is not N (first == ~0: nothing but N)
    u64 positions = 0;
    u32 launches = 0;
    dev_array<uint8_t> d_buf;     // the sequences, upper-cased, 'N' between them
    dev_array<u64> d_first_last, d_ctr;
};

struct lane_layout {
    std::vector<u32> lane0, nch;   // per sequence: its first lane, its chunks; lane of (i, j, ch) = lane0[i] + j * nch[i] + ch
    std::vector<prf_ilane> lanes;  // (the candidate and episode lists are placed by the stages that size them)
    u64 memo_total = 0;
};

struct walk_room {
    std::vector<u64> cand_cap;  // per lane
    u32 launches = 0;
    dev_array<prf_ilane> d_lanes;
    dev_array<u32> d_eps;
};

struct walk_result {
    std::vector<u64> cnt;       // per lane: candidates found
    std::vector<u32> lane_end;  // per lane: the walk ended in it
    u64 counters[4] = {};       // the CTR_WALK words of the last attempt
    float ms = 0;               // the walk kernel of the last attempt
    u32 launches = 0;
    prf_int_lanes dev{};        // what the emission reads
    dev_array<prf_icand> d_cands;
    dev_array<u64> d_cnt;
    dev_array<u32> d_end, d_first_end;
    dev_array<prf_imemo> d_memo;
};

struct hash_layout {
    std::vector<u64> off, size;  // per sequence, in slots
    u64 total = 0, cand_sum = 0;
};

struct free_rows {
    void operator()(prf_ihit *p) const { free(p); }
};
struct emit_result {
    u64 n_rows = 0;
    std::unique_ptr<prf_ihit, free_rows> rows;  // malloc'ed, sorted by (contig, start, end); none if n_rows == 0 or nobody asked
    float ms = 0;                // from just before the emission to after the sort
    u32 launches = 0;
};

template <class T>
int to_device(hipStream_t st, const std::vector<T> &h, T *d) {
    if (!h.empty()) HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return PRF_OK;
}
template <class T>
int to_host(hipStream_t st, const T *d, std::vector<T> *h) {
    if (!h->empty()) HIPCHK(hipMemcpyAsync(h->data(), d, h->size() * sizeof(T), hipMemcpyDeviceToHost, st));
    return PRF_OK;
}

int interrupted_check(const int_params &p) {
    int rc = check_params(p.kmin, p.kmax, p.min_repeats, p.min_span, 0);
    if (rc) return rc;
    if (p.uniform_call && p.uniform < 1)
        return fail(PRF_EINVAL, "max_interruptions is %u: prf_scan_interrupted serves max_interruptions >= 1 (0 is prf_scan's perfect path)",
                    p.uniform);
    if (!p.uniform_call && !p.by_k) return fail(PRF_EINVAL, "prf_scan_interrupted_by_k: NULL max_interruptions_by_k");
    if (p.min_repeats < 2)
        return fail(PRF_EUNSUPPORTED, "prf_scan_interrupted: min_repeats == 1 is not supported with interruptions (min_repeats >= 2)");
    if (p.kmax > 64) return fail(PRF_EUNSUPPORTED, "prf_scan_interrupted: max_motif_size %u > 64 (the phase set is one 64-bit mask)", p.kmax);
    if (p.memo_stride & (p.memo_stride - 1u))
        return fail(PRF_EINVAL, "prf_scan_interrupted: memo_stride %u is not a power of two", p.memo_stride);
    if (p.chunk && p.chunk < PRF_INT_CHUNK_MIN)
        return fail(PRF_EINVAL, "prf_scan_interrupted_chunked: chunk %llu is below the minimum of %u positions (0 = one lane per motif size)",
                    (unsigned long long)p.chunk, (unsigned)PRF_INT_CHUNK_MIN);
    return PRF_OK;
}

// The order is part of the interface: the parameters are judged before the context is looked at
int check_args(const prf_ctx *c, const prf_contig *contigs, int n_contigs, const int_params &p) {
    const int rc = interrupted_check(p);
    if (rc) return rc;
    if (!c) return fail(PRF_EINVAL, "prf_scan_interrupted: NULL context");
    if (n_contigs < 0 || (n_contigs && !contigs)) return fail(PRF_EINVAL, "prf_scan_interrupted: bad contig array");
    for (int i = 0; i < n_contigs; i++) {
        if (contigs[i].len && !contigs[i].ascii) return fail(PRF_EINVAL, "prf_scan_interrupted: NULL sequence");
        if (contigs[i].len >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "prf_scan_interrupted: input too large (2^40 positions)");
    }
    if (const int busy = refuse_in_flight(c, "prf_scan_interrupted")) return busy;
    if ((u64)n_contigs * p.nk() > 0x7fffffffull) return fail(PRF_EUNSUPPORTED, "prf_scan_interrupted: too many (sequence, motif size) lanes");
    return PRF_OK;
}

int stage_sequences(prf_ctx *c, const int_events &ev, const prf_contig *contigs, u32 n_seq, staged_seqs *s) {
    hipStream_t st = c->stream;
    std::vector<u64> pieces;  // the trim kernel's work: (sequence, first position, one past the last) per 4096 positions
    u64 total = 0;
    for (u32 i = 0; i < n_seq; i++) {
        const u64 len = contigs[i].len;
        s->base.push_back(total);
        s->len.push_back(len);
        total += (len + 16 + 15) & ~15ull;
        s->positions += len;
        for (u64 b = 0; b < len; b += 4096) pieces.insert(pieces.end(), {(u64)i, b, std::min<u64>(len, b + 4096)});
        s->first_last.insert(s->first_last.end(), {~0ull, 0ull});
    }
    dev_array<u64> d_base, d_pieces;
    int rc;
    if ((rc = s->d_buf.alloc(total + 16)) || (rc = d_base.alloc(n_seq)) || (rc = d_pieces.alloc(pieces.size())) ||
        (rc = s->d_first_last.alloc(2 * (size_t)n_seq)) || (rc = s->d_ctr.alloc(CTR_N)))
        return rc;
    HIPCHK(hipMemsetAsync(s->d_buf.p, 'N', total + 16, st));  // the gaps are letters: the symbol check passes over them
    for (u32 i = 0; i < n_seq; i++)
        if (contigs[i].len) HIPCHK(hipMemcpyAsync(s->d_buf.p + s->base[i], contigs[i].ascii, contigs[i].len, hipMemcpyHostToDevice, st));
    if ((rc = to_device(st, s->base, d_base.p)) || (rc = to_device(st, pieces, d_pieces.p)) ||
        (rc = to_device(st, s->first_last, s->d_first_last.p)))
        return rc;
    HIPCHK(hipMemsetAsync(s->d_ctr.p, 0, CTR_N * 8, st));
    HIPCHK(hipMemsetAsync(s->d_ctr.p + CTR_BADPOS, 0xFF, 8, st));  // first byte that is not a letter
    HIPCHK(hipEventRecord(ev.begin, st));
    if (total) HIPCHK(prf_launch_lit_upper(st, s->d_buf.p, total, s->d_ctr.p + CTR_BADPOS));
    HIPCHK(prf_launch_int_trim(st, s->d_buf.p, d_base.p, d_pieces.p, (u32)(pieces.size() / 3), s->d_first_last.p));
    s->launches = 2;
    u64 bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, s->d_ctr.p + CTR_BADPOS, 8, hipMemcpyDeviceToHost, st));
    if ((rc = to_host(st, s->d_first_last.p, &s->first_last))) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if (bad != ~0ull) {
        const u32 ci = (u32)(std::upper_bound(s->base.begin(), s->base.end(), bad) - s->base.begin()) - 1;
        return fail(PRF_ESYMBOL, "unsupported symbol at contig %u position %llu: only letters are accepted (A, C, G, T, N and -- as "
                    "ordinary symbols, like the reference -- any other letter, in either case)", ci, (unsigned long long)(bad - s->base[ci]));
    }
    return PRF_OK;
}

// lanes in (sequence, k, chunk) order; the chunks cut the trimmed sequence
int lay_out_lanes(const std::vector<u64> &base, const std::vector<u64> &len, const std::vector<u64> &first_last, const int_params &p,
                  lane_layout *lay) {
    const u32 n_seq = (u32)len.size(), nk = p.nk();
    u64 n_lanes = 0;
    for (u32 i = 0; i < n_seq; i++) {
        const u64 n_trim = first_last[2 * i] == ~0ull ? 0 : first_last[2 * i + 1] - first_last[2 * i];
        const u64 nc = p.chunk ? std::max<u64>(1, (n_trim + p.chunk - 1) / p.chunk) : 1;
        if (n_lanes + nc * nk > 0x7fffffffull) return fail(PRF_EUNSUPPORTED, "prf_scan_interrupted: too many (sequence, motif size, chunk) lanes");
        lay->lane0.push_back((u32)n_lanes);
        lay->nch.push_back((u32)nc);
        n_lanes += nc * nk;
    }
    lay->lanes.reserve(n_lanes);
    for (u32 i = 0; i < n_seq; i++) {
        const u64 reach = p.chunk ? std::min<u64>(len[i], p.chunk) : len[i];
        for (u32 j = 0; j < nk; j++)
            for (u32 ch = 0; ch < lay->nch[i]; ch++) {
                prf_ilane ln{};
                ln.seq = i;
                ln.k = p.kmin + j;
                ln.seq_base = base[i];
                ln.chunk = ch;
                ln.kslot = i * nk + j;
                ln.max_int = p.max_int(j);
                ln.lo = (u64)ch * p.chunk;
                ln.hi = p.chunk ? (u64)(ch + 1) * p.chunk : (u64)INT64_MAX;
                ln.memo_slots = p.memo_stride ? std::min<u64>(p.memo_slots, reach / p.memo_stride + 1) : 0;
                ln.memo_off = lay->memo_total;
                lay->memo_total += ln.memo_slots;
                lay->lanes.push_back(ln);
            }
    }
    return PRF_OK;
}

int size_walk_room(prf_ctx *c, const staged_seqs &s, const int_params &p, lane_layout *lay, walk_room *room) {
    hipStream_t st = c->stream;
    std::vector<prf_ilane> &lanes = lay->lanes;
    const u32 n_lanes = (u32)lanes.size();
    room->cand_cap.resize(n_lanes);
    int rc;
    if ((rc = room->d_lanes.alloc(n_lanes))) return rc;
    if (p.chunk) {
        // every episode of a lane lands on a boundary of its chunk (the first lane's first one on position 0) and lists at most
        // one candidate: counting the boundaries sizes both arrays so that the walk runs once
        dev_array<u64> d_bcount;
        if ((rc = d_bcount.alloc(n_lanes)) || (rc = to_device(st, lanes, room->d_lanes.p))) return rc;
        if (n_lanes) HIPCHK(hipMemsetAsync(d_bcount.p, 0, 8 * (size_t)n_lanes, st));
        HIPCHK(prf_launch_int_bound(st, s.d_buf.p, room->d_lanes.p, n_lanes, s.d_first_last.p, d_bcount.p));
        room->launches = 1;
        if ((rc = to_host(st, d_bcount.p, &room->cand_cap))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        for (u64 &cap : room->cand_cap) cap += 1;
    } else {
        // about one candidate per five positions on random sequence (every episode that jumps back ends in one): room for one per
        // four, so that the walk usually runs once
        for (u32 li = 0; li < n_lanes; li++) room->cand_cap[li] = s.len[lanes[li].seq] / 4 + 16;
    }
    u64 ep_total = 0;
    for (u32 li = 0; li < n_lanes; li++) {
        prf_ilane &ln = lanes[li];
        // episodes land at strictly increasing positions: at most len of them; past ep_cap they are not recorded
        ln.ep_cap = !ln.memo_slots ? 0 : p.chunk ? room->cand_cap[li] : s.len[ln.seq] / 4 + 64;
        ln.ep_off = ep_total;
        ep_total += ln.ep_cap;
    }
    return room->d_eps.alloc(ep_total);
}

int walk(prf_ctx *c, const int_events &ev, const staged_seqs &s, const int_params &p, lane_layout *lay, walk_room *room, walk_result *w) {
    hipStream_t st = c->stream;
    std::vector<prf_ilane> &lanes = lay->lanes;
    const u32 n_lanes = (u32)lanes.size();
    const size_t n_kslots = s.len.size() * p.nk();
    w->cnt.resize(n_lanes);
    w->lane_end.resize(n_lanes);
    int rc;
    if ((rc = w->d_cnt.alloc(n_lanes)) || (rc = w->d_end.alloc(n_lanes)) || (rc = w->d_first_end.alloc(n_kslots)) ||
        (rc = w->d_memo.alloc(lay->memo_total)))
        return rc;
    for (int attempt = 0;; attempt++) {
        u64 cand_total = 0;
        for (u32 li = 0; li < n_lanes; li++) {
            lanes[li].cand_off = cand_total;
            lanes[li].cand_cap = room->cand_cap[li];
            cand_total += room->cand_cap[li];
        }
        if ((rc = w->d_cands.alloc(cand_total)) || (rc = to_device(st, lanes, room->d_lanes.p))) return rc;
        if (lay->memo_total) HIPCHK(hipMemsetAsync(w->d_memo.p, 0xFF, lay->memo_total * sizeof(prf_imemo), st));  // no state has pos ~0
        if (n_kslots) HIPCHK(hipMemsetAsync(w->d_first_end.p, 0xFF, 4 * n_kslots, st));
        HIPCHK(hipMemsetAsync(s.d_ctr.p + CTR_WALK, 0, (CTR_N - CTR_WALK) * 8, st));
        w->dev = prf_int_lanes{room->d_lanes.p, n_lanes, s.d_first_last.p, w->d_cands.p, w->d_cnt.p, w->d_end.p};
        prf_int_walk_args a{};
        a.l = w->dev;
        a.buf = s.d_buf.p;
        a.min_repeats = p.min_repeats; a.min_span = p.min_span; a.stride = p.memo_stride;
        a.first_end = p.chunk ? w->d_first_end.p : nullptr;
        a.memo = w->d_memo.p;
        a.eps = room->d_eps.p;
        a.counters = s.d_ctr.p + CTR_WALK;
        HIPCHK(hipEventRecord(ev.walk_begin, st));
        HIPCHK(prf_launch_int_walk(st, a));
        HIPCHK(hipEventRecord(ev.walk_end, st));
        w->launches++;
        if ((rc = to_host(st, w->d_cnt.p, &w->cnt)) || (rc = to_host(st, w->d_end.p, &w->lane_end))) return rc;
        HIPCHK(hipMemcpyAsync(w->counters, s.d_ctr.p + CTR_WALK, sizeof w->counters, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool over = false;
        for (u32 li = 0; li < n_lanes; li++) {
            if (w->cnt[li] > (u64)0x3fffffff) return fail(PRF_EUNSUPPORTED, "prf_scan_interrupted: more than 2^30 candidates on one lane");
            if (w->cnt[li] > room->cand_cap[li]) { over = true; room->cand_cap[li] = w->cnt[li]; }
        }
        if (!over) break;
        if (attempt >= 1) return fail(PRF_EHIP, "prf_scan_interrupted: the candidate counts changed between two runs");
    }
    HIPCHK(hipEventElapsedTime(&w->ms, ev.walk_begin, ev.walk_end));
    return PRF_OK;
}

// the chunks behind the first lane of a (sequence, k) that ended start on landings the walk never reaches: their candidates
// do not count
int drop_unreached(const lane_layout &lay, const int_params &p, const std::vector<u32> &lane_end, std::vector<u64> *cnt, u64 *dropped) {
    *dropped = 0;
    for (u32 i = 0; i < lay.nch.size(); i++)
        for (u32 j = 0; j < p.nk(); j++) {
            const u32 nch = lay.nch[i], l0 = lay.lane0[i] + j * nch;
            u32 e = 0;
            while (e < nch && !lane_end[l0 + e]) e++;
            if (e == nch) return fail(PRF_EHIP, "prf_scan_interrupted: no lane of contig %u, motif size %u reached the end", i, p.kmin + j);
            for (u32 ch = e + 1; ch < nch; ch++) (*cnt)[l0 + ch] = 0;
            *dropped += nch - 1 - e;
        }
    return PRF_OK;
}

// a power of two of slots, at least twice the candidates of the sequence
hash_layout size_hashes(const lane_layout &lay, u32 nk, const std::vector<u64> &cnt) {
    hash_layout h;
    for (u32 i = 0; i < lay.nch.size(); i++) {
        u64 cs = 0;
        for (u32 l = 0; l < nk * lay.nch[i]; l++) cs += cnt[(size_t)lay.lane0[i] + l];
        h.cand_sum += cs;
        u64 sz = 16;
        while (sz < 2 * cs) sz <<= 1;
        h.off.push_back(h.total);
        h.size.push_back(sz);
        h.total += sz;
    }
    return h;
}

// one emission lane per sequence; want_rows: copy the sorted rows to the host
int emit_and_sort(prf_ctx *c, const int_events &ev, const staged_seqs &s, const lane_layout &lay, const walk_result &w, const hash_layout &h,
                  u32 nk, bool want_rows, emit_result *r) {
    hipStream_t st = c->stream;
    dev_array<u32> d_lane0, d_nch;
    dev_array<u64> d_hoff, d_hsize, d_keys;
    dev_array<prf_ihit_dev> d_rows, d_sorted;
    dev_array<char> d_scratch;
    int rc;
    if ((rc = d_lane0.alloc(lay.lane0.size())) || (rc = d_nch.alloc(lay.nch.size())) || (rc = d_hoff.alloc(h.off.size())) ||
        (rc = d_hsize.alloc(h.size.size())) || (rc = d_keys.alloc(2 * h.total)) || (rc = d_rows.alloc(h.cand_sum)) ||
        (rc = d_sorted.alloc(h.cand_sum)) || (rc = d_scratch.alloc(prf_int_sort_scratch_bytes(h.cand_sum))))
        return rc;
    if ((rc = to_device(st, lay.lane0, d_lane0.p)) || (rc = to_device(st, lay.nch, d_nch.p)) || (rc = to_device(st, h.off, d_hoff.p)) ||
        (rc = to_device(st, h.size, d_hsize.p)))
        return rc;
    if (h.total) HIPCHK(hipMemsetAsync(d_keys.p, 0, h.total * 16, st));
    HIPCHK(hipMemsetAsync(s.d_ctr.p + CTR_ROWS, 0, 8, st));
    prf_int_emit_args a{};
    a.l = w.dev;
    a.nk = nk; a.n_seq = (u32)lay.nch.size();
    a.lane0 = d_lane0.p; a.n_chunks = d_nch.p;
    a.hash_off = d_hoff.p; a.hash_size = d_hsize.p;
    a.keys = d_keys.p;
    a.rows = d_rows.p;
    a.row_cnt = s.d_ctr.p + CTR_ROWS;
    HIPCHK(hipEventRecord(ev.emit_begin, st));
    HIPCHK(prf_launch_int_emit(st, a));
    r->launches = 1;
    HIPCHK(hipMemcpyAsync(&r->n_rows, s.d_ctr.p + CTR_ROWS, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (r->n_rows > h.cand_sum)
        return fail(PRF_EHIP, "prf_scan_interrupted: emission returned %llu rows for %llu candidates", (unsigned long long)r->n_rows,
                    (unsigned long long)h.cand_sum);
    HIPCHK(prf_int_sort_rows(st, d_rows.p, r->n_rows, d_sorted.p, d_scratch.p));
    if (r->n_rows) r->launches += 11;
    HIPCHK(hipEventRecord(ev.end, st));
    static_assert(sizeof(prf_ihit) == sizeof(prf_ihit_dev), "row layouts must agree");
    if (want_rows && r->n_rows) {
        r->rows.reset((prf_ihit *)malloc(r->n_rows * sizeof(prf_ihit)));
        if (!r->rows) return fail(PRF_ENOMEM, "prf_scan_interrupted: cannot allocate %llu rows", (unsigned long long)r->n_rows);
        HIPCHK(hipMemcpyAsync(r->rows.get(), d_sorted.p, r->n_rows * sizeof(prf_ihit), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&r->ms, ev.emit_begin, ev.end));
    return PRF_OK;
}

// counters_out (may be NULL): n_counters words of steps, memo lookups, memo hits, recorded episodes, lanes, dropped lanes
int interrupted_scan(prf_ctx *c, const prf_contig *contigs, int n_contigs, const int_params &p, prf_ihits *out, prf_scan_stats *stats,
                     uint64_t *counters_out, u32 n_counters) {
    if (out) { out->rows = nullptr; out->n = 0; }
    int rc = check_args(c, contigs, n_contigs, p);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->dev));
    const int_events ev{c->ev[0], c->ev[1], c->ev[2], c->ev[3], c->ev[4]};
    staged_seqs seqs;
    lane_layout lay;
    walk_room room;
    walk_result w;
    u64 dropped = 0;
    if ((rc = stage_sequences(c, ev, contigs, (u32)n_contigs, &seqs)) ||
        (rc = lay_out_lanes(seqs.base, seqs.len, seqs.first_last, p, &lay)) ||
        (rc = size_walk_room(c, seqs, p, &lay, &room)) ||
        (rc = walk(c, ev, seqs, p, &lay, &room, &w)) ||
        (rc = drop_unreached(lay, p, w.lane_end, &w.cnt, &dropped)))
        return rc;
    const hash_layout h = size_hashes(lay, p.nk(), w.cnt);
    emit_result e;
    if ((rc = emit_and_sort(c, ev, seqs, lay, w, h, p.nk(), out != nullptr, &e))) return rc;
    float all_ms = 0;
    HIPCHK(hipEventElapsedTime(&all_ms, ev.begin, ev.end));
    c->last.nhits = 0;  // the rows of this lane are handed over on the host only
    c->last.rows = nullptr;
    if (out) { out->n = e.rows ? e.n_rows : 0; out->rows = e.rows.release(); }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = all_ms;
        stats->phase1_ms = w.ms;
        stats->phase2_ms = e.ms;
        stats->positions = seqs.positions;
        stats->packed_bytes = seqs.positions;  // this lane reads the bytes themselves
        stats->n_candidates = h.cand_sum;
        stats->n_hits = e.n_rows;
        stats->n_launches = seqs.launches + room.launches + w.launches + e.launches;
        stats->path = 3;
        stats->sorted_on_device = 1;
    }
    const u64 six[6] = {w.counters[0], w.counters[1], w.counters[2], w.counters[3], lay.lanes.size(), dropped};
    if (counters_out) memcpy(counters_out, six, n_counters * sizeof(u64));
    return PRF_OK;
}

}  // namespace

extern "C" {

int prf_scan_interrupted_ex(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                            uint32_t min_span, uint32_t max_interruptions, uint32_t memo_stride, uint64_t memo_slots, prf_ihits *out,
                            prf_scan_stats *stats, uint64_t *counters) {
    return guarded("prf_scan_interrupted", [&] {
        const int_params p{kmin, kmax, min_repeats, min_span, memo_stride, memo_slots, 0, nullptr, max_interruptions, true};
        return interrupted_scan(c, contigs, n_contigs, p, out, stats, counters, 4);
    });
}

int prf_scan_interrupted_chunked(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                                 uint32_t min_span, uint32_t max_interruptions, uint32_t memo_stride, uint64_t memo_slots, uint64_t chunk,
                                 prf_ihits *out, prf_scan_stats *stats, uint64_t *counters) {
    return guarded("prf_scan_interrupted_chunked", [&] {
        const int_params p{kmin, kmax, min_repeats, min_span, memo_stride, memo_slots, chunk, nullptr, max_interruptions, true};
        return interrupted_scan(c, contigs, n_contigs, p, out, stats, counters, 6);
    });
}

int prf_scan_interrupted_by_k(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                              uint32_t min_span, const uint32_t *max_interruptions_by_k, uint32_t memo_stride, uint64_t memo_slots,
                              uint64_t chunk, prf_ihits *out, prf_scan_stats *stats, uint64_t *counters) {
    return guarded("prf_scan_interrupted_by_k", [&] {
        const int_params p{kmin, kmax, min_repeats, min_span, memo_stride, memo_slots, chunk, max_interruptions_by_k, 0, false};
        return interrupted_scan(c, contigs, n_contigs, p, out, stats, counters, 6);
    });
}

int prf_scan_interrupted(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmin, uint32_t kmax, uint32_t min_repeats,
                         uint32_t min_span, uint32_t max_interruptions, prf_ihits *out, prf_scan_stats *stats) {
    return prf_scan_interrupted_chunked(c, contigs, n_contigs, kmin, kmax, min_repeats, min_span, max_interruptions, PRF_MEMO_STRIDE,
                                        PRF_MEMO_SLOTS, PRF_INT_CHUNK, out, stats, nullptr);
}

void prf_free_ihits(prf_ihits *hits) {
    if (!hits) return;
    free(hits->rows);
    hits->rows = nullptr;
    hits->n = 0;
}

}  // extern "C"
