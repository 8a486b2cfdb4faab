// dotplot_host.cpp -- the exact dot plot's part of the host path (prf_dotplot_bits / prf_dotplot_counts, their _ex and one-shot
// forms; kernel: dotplot.hip).  The path itself is matrix_host.h.  One call = one window of the n x n matrix of a
// range: the window's rows are cut into launches of at most launch_cells cells (whole tiles of rows; by default fewer cells the
// larger the threshold, as the filter's cost per cell grows).
// NOTE: check_room's window clipping and output sizing and launch's cut into launches are repeated in dotpair_host.cpp (pair_request):
// a change to either belongs in both.
#include "matrix_host.h"

namespace {

struct dot_request {
    static constexpr u32 path = 5;
    u64 begin, end, row0, row1, col0, col1;
    u32 t;
    bool counts;        // the entry point: cells per block (counts) or the cells themselves (bits)
    u64 block;
    void *dst;
    u64 capacity;       // entries (counts) or words (bits) dst holds
    uint64_t *n_out0;   // bits: words per row; counts: block rows
    uint64_t *n_out1;   // counts: block columns
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS, divided by the filter's cost
    struct room {
        u64 n, row0, row1, col0, col1;   // the clipped range and window
        u64 out_rows, out_cols;          // of the output: rows x words, or block rows x block columns
        u64 total() const { return out_rows * out_cols; }
    };
    bool bits() const { return !counts; }
    u32 load_kmax() const { return 64; }
    int check_view(const char *, const prf_genome *, const prf_contig_view &, room *) const { return PRF_OK; }
    void publish(const room &o) const {
        *n_out0 = bits() ? o.out_cols : o.out_rows;
        if (n_out1) *n_out1 = o.out_cols;
    }

    int check(const char *name) const {
        if (counts && (block < 64 || block % 64 || block > 32768))
            return fail(PRF_EINVAL, "%s: block is %llu. It must be a multiple of 64, at least 64 and at most 32768.", name, (unsigned long long)block);
        if (begin > end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)begin, (unsigned long long)end);
        if (row0 > row1) return fail(PRF_EINVAL, "%s: row0 %llu is behind row1 %llu", name, (unsigned long long)row0, (unsigned long long)row1);
        if (col0 > col1) return fail(PRF_EINVAL, "%s: col0 %llu is behind col1 %llu", name, (unsigned long long)col0, (unsigned long long)col1);
        if (t > PRF_DOT_MAX_RUN)
            return fail(PRF_EUNSUPPORTED, "%s: min_diagonal_run %u is above %u (PRF_DOT_MAX_RUN)", name, t, PRF_DOT_MAX_RUN);
        if (!dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
        if (!n_out0 || (counts && !n_out1)) return fail(PRF_EINVAL, "%s: NULL size pointer", name);
        return PRF_OK;
    }

    int check_room(const char *name, u64 seq_len, room *o) const {
        int rc = matrix_clip(name, begin, end, seq_len, &o->n);
        if (rc) return rc;
        o->row1 = row1 < o->n ? row1 : o->n;
        o->row0 = row0 < o->row1 ? row0 : o->row1;
        o->col1 = col1 < o->n ? col1 : o->n;
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
        prf_dotplot_args a{};
        a.pl = v.planes;
        a.g_begin = v.base + begin;
        a.n = o.n;
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
        // rows per launch: whole tiles, at most launch_cells cells and 2^30 workgroups, at least one tile.  The filter costs m^2
        // steps per cell and direction above m = 2, so the default shrinks with it: a launch stays a few ms long.
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
            HIPCHK(prf_launch_dotplot(stream, a, bits()));
            ++*launches;
        }
        return PRF_OK;
    }
};

}  // namespace

extern "C" {

int prf_dotplot_bits_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                        uint64_t col0, uint64_t col1, uint32_t t, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row,
                        prf_scan_stats *stats, uint64_t launch_cells) {
    return matrix_on_genome("prf_dotplot_bits", c, g, contig,
                            dot_request{begin, end, row0, row1, col0, col1, t, false, 0, dst, capacity_words, words_per_row, nullptr, launch_cells},
                            stats);
}

int prf_dotplot_counts_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                          uint64_t col0, uint64_t col1, uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity,
                          uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats, uint64_t launch_cells) {
    return matrix_on_genome("prf_dotplot_counts", c, g, contig,
                            dot_request{begin, end, row0, row1, col0, col1, t, true, block, dst, capacity, n_block_rows, n_block_cols, launch_cells},
                            stats);
}

int prf_dotplot_bits(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                     uint64_t col0, uint64_t col1, uint32_t t, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row,
                     prf_scan_stats *stats) {
    return prf_dotplot_bits_ex(c, g, contig, begin, end, row0, row1, col0, col1, t, dst, capacity_words, words_per_row, stats, 0);
}

int prf_dotplot_counts(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                       uint64_t col0, uint64_t col1, uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity,
                       uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats) {
    return prf_dotplot_counts_ex(c, g, contig, begin, end, row0, row1, col0, col1, t, block, dst, capacity, n_block_rows, n_block_cols,
                                 stats, 0);
}

int prf_dotplot_bits_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1, uint64_t col0,
                         uint64_t col1, uint32_t t, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row,
                         prf_scan_stats *stats) {
    return matrix_one_shot("prf_dotplot_bits_seq", c, seq,
                           dot_request{begin, end, row0, row1, col0, col1, t, false, 0, dst, capacity_words, words_per_row, nullptr, 0}, stats);
}

int prf_dotplot_counts_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1, uint64_t col0,
                           uint64_t col1, uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity, uint64_t *n_block_rows,
                           uint64_t *n_block_cols, prf_scan_stats *stats) {
    return matrix_one_shot("prf_dotplot_counts_seq", c, seq,
                           dot_request{begin, end, row0, row1, col0, col1, t, true, block, dst, capacity, n_block_rows, n_block_cols, 0}, stats);
}

int prf_dotplot_shape(uint32_t t, uint32_t *tile_rows, uint32_t *span_words, uint32_t *halo_rows) {
    if (!tile_rows || !span_words || !halo_rows) return fail(PRF_EINVAL, "prf_dotplot_shape: NULL pointer");
    if (t > PRF_DOT_MAX_RUN) return fail(PRF_EUNSUPPORTED, "prf_dotplot_shape: min_diagonal_run %u is above %u (PRF_DOT_MAX_RUN)", t, PRF_DOT_MAX_RUN);
    prf_dotplot_shape_for(t, tile_rows, span_words, halo_rows);
    return PRF_OK;
}

}  // extern "C"
