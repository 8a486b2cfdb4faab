// matrix_host.h -- the host path that the matrix products share (periodicity_host.cpp, dotplot_host.cpp, dotpair_host.cpp;
// list_host.h, the frame of the products whose output is a list with a count, includes it for matrix_clip and
// matrix_check_letters; nobody else includes it).
//
// One call = one range of one contig of a resident genome (a product of two ranges names the second one in its request and
// resolves it in check_view): judge the arguments (before the context or the genome is looked at),
// take the contig's planes, clip `end`, size and zero the output on the device, launch between two events, copy the output to the
// caller.  Nothing of the scans' state is touched: no selection is read, no row sink written, the rows of the last scan stay
// where they are.  The order of the refusals is part of the interface (tests/test_periodicity_cpu.py, tests/test_dotplot_cpu.py).
//
// A product is its request R:
//   static constexpr u32 path                      prf_scan_stats.path
//   u64 begin, end;  bool bits() const             the range; words of bits (no zeroing) or 32-bit counts
//   struct room { u64 n; u64 total() const; ... }  the positions the call covers (the stats' positions), the entries of the output
//   int check(name) const                          what can be said without a genome
//   int check_room(name, seq_len, room *) const    what needs the length of the sequence
//   int check_view(name, genome, view, room *) const   what needs the genome; may note in the room what check_room needs from it
//   void publish(room) const                       the sizes, to the caller's size pointers
//   u32 load_kmax() const                          the kmax_hint a one-shot call loads its sequence with
//   int launch(stream, view, room, d_out, u32 *launches) const
#pragma once
#include <cctype>

#include "prf_ctx.h"

// `end` clipped to the sequence; *n = the positions of the range
static int matrix_clip(const char *name, u64 begin, u64 end, u64 seq_len, u64 *n) {
    if (end > seq_len) end = seq_len;
    *n = begin < end ? end - begin : 0;
    if (*n >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "%s: range too large (2^40 positions)", name);
    return PRF_OK;
}

// An output of a x b entries against the caller's room and the limit per call.  `a_what` is what the text calls a, `advice` ends
// the limit's text.
static int matrix_check_output(const char *name, bool bits, u64 capacity, u64 a, const char *a_what, u64 b, const char *advice) {
    const unsigned long long total = a * b, limit = PRF_PERIOD_BITS_MAX_WORDS;
    const char *entries = bits ? "words" : "counts";
    if (total > capacity)
        return fail(PRF_EINVAL, "%s: the destination holds %llu %s, the output has %llu (%llu%s x %llu)", name,
                    (unsigned long long)capacity, entries, total, (unsigned long long)a, a_what, (unsigned long long)b);
    if (total > limit)
        return fail(PRF_EUNSUPPORTED, "%s: an output of %llu %s is above the limit of %llu per call%s", name, total, entries, limit, advice);
    return PRF_OK;
}

// what the packer would refuse, found on the host
static int matrix_check_letters(const char *name, const prf_contig *seq) {
    for (u64 i = 0; i < seq->len; i++)
        if (!isalpha(seq->ascii[i]) || seq->ascii[i] > 127)
            return fail(PRF_ESYMBOL, "%s: unsupported symbol at position %llu: only letters can be packed", name, (unsigned long long)i);
    return PRF_OK;
}

template <class R>
static int matrix_run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const R &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    typename R::room o;
    if ((rc = r.check_view(name, g, v, &o))) return rc;
    if ((rc = r.check_room(name, v.len, &o))) return rc;
    if ((rc = refuse_in_flight(c, name))) return rc;
    HIPCHK(hipSetDevice(c->dev));
    r.publish(o);
    const size_t bytes = (size_t)o.total() * (r.bits() ? sizeof(u64) : sizeof(u32));
    float ms = 0;
    u32 launches = 0;
    if (bytes) {
        dev_array<unsigned char> d_out;
        if ((rc = d_out.alloc(bytes))) return rc;
        if (!r.bits()) HIPCHK(hipMemsetAsync(d_out.p, 0, bytes, c->stream));
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        if ((rc = r.launch(c->stream, v, o, d_out.p, &launches))) return rc;
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(r.dst, d_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    }
    lane_stats(stats, R::path, ms, o.n, (o.n + 3) / 4, launches);
    return PRF_OK;
}

template <class R>
static int matrix_on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const R &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = r.check(name);
        return rc ? rc : matrix_run(name, c, g, contig, r, stats);
    });
}

// load + call + free; everything that can be refused from the arguments and the bytes is refused before the context is looked at
template <class R>
static int matrix_one_shot(const char *name, prf_ctx *c, const prf_contig *seq, const R &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        typename R::room o;
        if ((rc = r.check_room(name, seq->len, &o))) return rc;
        if ((rc = matrix_check_letters(name, seq))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, r.load_kmax(), &g))) return rc;
        rc = matrix_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}
