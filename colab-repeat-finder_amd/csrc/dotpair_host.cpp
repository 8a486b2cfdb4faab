// dotpair_host.cpp -- the part of the host path that the dot plot of two ranges owns (prf_dotpair_bits / prf_dotpair_counts, their
// _ex and one-shot forms; kernel: dotplot_pair.hip).  The path itself is matrix_host.h: its contig is A's (the rows),
// the request names B's (the columns) and takes that view from the same genome in check_view.  One call = one window of the
// na x nb matrix; the window's rows are cut into launches as dotplot_host.cpp cuts them.
// NOTE: check_room's window clipping and output sizing and launch's cut into launches are repeated in dotplot_host.cpp (dot_request):
// a change to either belongs in both.
#include "matrix_host.h"

namespace {

struct pair_request {
    static constexpr u32 path = 6;
    u64 begin, end;     // A's range, on the contig the path is called with
    u32 b_contig;
    u64 b_begin, b_end;
    u32 strand;
    u64 row0, row1, col0, col1;
    u32 t;
    bool counts;        // the entry point: cells per block (counts) or the cells themselves (bits)
    u64 block;
    void *dst;
    u64 capacity;       // entries (counts) or words (bits) dst holds
    uint64_t *n_out0;   // bits: words per row; counts: block rows
    uint64_t *n_out1;   // counts: block columns
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS, divided by the filter's cost
    struct room {
        u64 b_base, b_len;               // B's contig: its first global position and its length
        u64 n, na, nb;                   // n = na + nb, the positions of the two clipped ranges
        u64 row0, row1, col0, col1;      // the clipped window
        u64 out_rows, out_cols;          // of the output: rows x words, or block rows x block columns
        u64 total() const { return out_rows * out_cols; }
    };
    bool bits() const { return !counts; }
    u32 load_kmax() const { return 64; }
    void publish(const room &o) const {
        *n_out0 = bits() ? o.out_cols : o.out_rows;
        if (n_out1) *n_out1 = o.out_cols;
    }

    int check(const char *name) const {
        if (counts && (block < 64 || block % 64 || block > 32768))
            return fail(PRF_EINVAL, "%s: block is %llu. It must be a multiple of 64, at least 64 and at most 32768.", name, (unsigned long long)block);
        if (begin > end) return fail(PRF_EINVAL, "%s: a_begin %llu is behind a_end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (b_begin > b_end)
            return fail(PRF_EINVAL, "%s: b_begin %llu is behind b_end %llu", name, (unsigned long long)b_begin, (unsigned long long)b_end);
        if (row0 > row1) return fail(PRF_EINVAL, "%s: row0 %llu is behind row1 %llu", name, (unsigned long long)row0, (unsigned long long)row1);
        if (col0 > col1) return fail(PRF_EINVAL, "%s: col0 %llu is behind col1 %llu", name, (unsigned long long)col0, (unsigned long long)col1);
        if (strand > 1) return fail(PRF_EINVAL, "%s: strand is %u. It must be 0 (plus) or 1 (minus).", name, strand);
        if (t > PRF_DOT_MAX_RUN)
            return fail(PRF_EUNSUPPORTED, "%s: min_diagonal_run %u is above %u (PRF_DOT_MAX_RUN)", name, t, PRF_DOT_MAX_RUN);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        if (!n_out0 || (counts && !n_out1)) return fail(PRF_EINVAL, "%s: NULL size pointer", name);
        return PRF_OK;
    }

    // B's contig, of the same genome (and so of the same context and the same planes) as A's
    int check_view(const char *, const prf_genome *g, const prf_contig_view &, room *o) const {
        prf_contig_view vb;
        const int rc = prf_genome_contig_view(g, b_contig, &vb);
        if (rc) return rc;
        o->b_base = vb.base;
        o->b_len = vb.len;
        return PRF_OK;
    }

    // o->b_len is set: by check_view, or by the one-shot form from its second sequence
    int check_room(const char *name, u64 a_len, room *o) const {
        int rc = matrix_clip(name, begin, end, a_len, &o->na);
        if (!rc) rc = matrix_clip(name, b_begin, b_end, o->b_len, &o->nb);
        if (rc) return rc;
        o->n = o->na + o->nb;
        o->row1 = row1 < o->na ? row1 : o->na;
        o->row0 = row0 < o->row1 ? row0 : o->row1;
        o->col1 = col1 < o->nb ? col1 : o->nb;
        o->col0 = col0 < o->col1 ? col0 : o->col1;
        const u64 rows = o->row1 - o->row0, cols = o->col1 - o->col0;
        const u64 unit = bits() ? 64 : block;
        o->out_rows = bits() ? rows : (rows + unit - 1) / unit;
        o->out_cols = (cols + unit - 1) / unit;
        rc = matrix_check_output(name, bits(), capacity, o->out_rows, "", o->out_cols,
                                 bits() ? " (PRF_PERIOD_BITS_MAX_WORDS): ask for counts, or for a smaller window"
                                        : " (PRF_PERIOD_BITS_MAX_WORDS): ask for a larger block or a smaller window");
        if (rc) return rc;
        if (rows && cols > PRF_DOT_MAX_CELLS / rows)
            return fail(PRF_EUNSUPPORTED, "%s: a window of %llu x %llu cells is above the limit of 2^42 per call (PRF_DOT_MAX_CELLS)", name,
                        (unsigned long long)rows, (unsigned long long)cols);
        return PRF_OK;
    }

    int launch(hipStream_t stream, const prf_contig_view &v, const room &o, void *d_out, u32 *launches) const {
        prf_dotpair_args a{};
        a.pl = v.planes;
        a.a_g_begin = v.base + begin;
        a.na = o.na;
        a.b_g_begin = o.b_base + b_begin;
        a.nb = o.nb;
        a.strand = strand;
        a.row0 = o.row0;
        a.col0 = o.col0;
        a.col1 = o.col1;
        a.words_per_row = (o.col1 - o.col0 + 63) / 64;
        a.m = t > 2 ? t - 1 : 1;
        a.wpb = bits() ? 1u : (u32)(block / 64);
        a.n_block_cols = o.out_cols;
        a.bits = bits() ? (u64 *)d_out : nullptr;
        a.counts = bits() ? nullptr : (u32 *)d_out;
        u32 tile_rows, span_words, halo;
        prf_dotplot_shape_for(t, &tile_rows, &span_words, &halo);
        // rows per launch, as dot_request::launch (dotplot_host.cpp) cuts them: whole tiles, at most launch_cells cells and 2^30
        // workgroups, at least one tile; the default shrinks with the filter's cost
        const u64 cost = a.m > 2 ? ((u64)a.m * a.m + 3) / 4 : 1;
        const u64 cells = launch_cells ? launch_cells : PRF_DOT_LAUNCH_CELLS / cost;
        const u64 cols = o.col1 - o.col0;
        const u64 n_spans = (a.words_per_row + span_words - 1) / span_words;
        u64 tiles = cells / cols / tile_rows;
        if (tiles > (1ull << 30) / n_spans) tiles = (1ull << 30) / n_spans;
        if (tiles < 1) tiles = 1;
        for (u64 lr = o.row0; lr < o.row1; lr += tiles * tile_rows) {
            a.lrow0 = lr;
            a.lrow1 = o.row1 - lr > tiles * tile_rows ? lr + tiles * tile_rows : o.row1;
            HIPCHK(prf_launch_dotpair(stream, a, bits()));
            ++*launches;
        }
        return PRF_OK;
    }
};

// matrix_one_shot for two sequences: they become contigs 0 (A) and 1 (B) of a genome that lives for the call.  Everything that can
// be refused from the arguments and the bytes is refused before the context is looked at.
int pair_one_shot(const char *name, prf_ctx *c, const prf_contig *seq_a, const prf_contig *seq_b, const pair_request &r, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = r.check(name);
        if (rc) return rc;
        for (const prf_contig *seq : {seq_a, seq_b})
            if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        pair_request::room o{};
        o.b_len = seq_b->len;
        if ((rc = r.check_room(name, seq_a->len, &o))) return rc;
        if ((rc = matrix_check_letters(name, seq_a)) || (rc = matrix_check_letters(name, seq_b))) return rc;
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        const prf_contig both[2] = {*seq_a, *seq_b};
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, both, 2, r.load_kmax(), &g))) return rc;
        rc = matrix_run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_dotpair_bits_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                        uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                        uint32_t t, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row, prf_scan_stats *stats,
                        uint64_t launch_cells) {
    return matrix_on_genome("prf_dotpair_bits", c, g, a_contig,
                            pair_request{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, t, false, 0, dst,
                                         capacity_words, words_per_row, nullptr, launch_cells},
                            stats);
}

int prf_dotpair_counts_ex(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                          uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                          uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols,
                          prf_scan_stats *stats, uint64_t launch_cells) {
    return matrix_on_genome("prf_dotpair_counts", c, g, a_contig,
                            pair_request{a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, t, true, block, dst,
                                         capacity, n_block_rows, n_block_cols, launch_cells},
                            stats);
}

int prf_dotpair_bits(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                     uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                     uint32_t t, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row, prf_scan_stats *stats) {
    return prf_dotpair_bits_ex(c, g, a_contig, a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, t, dst,
                               capacity_words, words_per_row, stats, 0);
}

int prf_dotpair_counts(prf_ctx *c, const prf_genome *g, uint32_t a_contig, uint64_t a_begin, uint64_t a_end, uint32_t b_contig,
                       uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                       uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols,
                       prf_scan_stats *stats) {
    return prf_dotpair_counts_ex(c, g, a_contig, a_begin, a_end, b_contig, b_begin, b_end, strand, row0, row1, col0, col1, t, block, dst,
                                 capacity, n_block_rows, n_block_cols, stats, 0);
}

int prf_dotpair_bits_seq(prf_ctx *c, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b, uint64_t b_begin,
                         uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1, uint32_t t,
                         uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row, prf_scan_stats *stats) {
    return pair_one_shot("prf_dotpair_bits_seq", c, seq_a, seq_b,
                         pair_request{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, t, false, 0, dst, capacity_words,
                                      words_per_row, nullptr, 0},
                         stats);
}

int prf_dotpair_counts_seq(prf_ctx *c, const prf_contig *seq_a, uint64_t a_begin, uint64_t a_end, const prf_contig *seq_b,
                           uint64_t b_begin, uint64_t b_end, uint32_t strand, uint64_t row0, uint64_t row1, uint64_t col0, uint64_t col1,
                           uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity, uint64_t *n_block_rows, uint64_t *n_block_cols,
                           prf_scan_stats *stats) {
    return pair_one_shot("prf_dotpair_counts_seq", c, seq_a, seq_b,
                         pair_request{a_begin, a_end, 1, b_begin, b_end, strand, row0, row1, col0, col1, t, true, block, dst, capacity,
                                      n_block_rows, n_block_cols, 0},
                         stats);
}

}  // extern "C"
