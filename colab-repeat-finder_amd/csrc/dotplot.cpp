// dotplot.cpp -- the host path of the exact dot plot (prf_dotplot_bits / prf_dotplot_counts, their _ex and one-shot forms;
// kernel: dotplot.hip).
//
// One call = one window of the n x n matrix of one range of one contig of a resident genome: judge the arguments (before the
// context or the genome is looked at), take the contig's planes, clip `end` and the window, size and zero the output on the
// device, cut the window's rows into launches of at most launch_cells cells (whole tiles of rows; by default fewer cells the
// larger the threshold, as the filter's cost per cell grows) between two events, copy the output to the caller.  Nothing of
// the scans' state is touched: no selection is read, no row sink written, the rows of the last scan stay where they are.
#include <cctype>
#include <cstring>

#include "prf_ctx.h"

namespace {

struct dot_request {
    u64 begin, end, row0, row1, col0, col1;
    u32 t;
    u64 block;          // 0: the cells themselves (bits)
    void *dst;
    u64 capacity;       // entries (counts) or words (bits) dst holds
    uint64_t *n_out0;   // bits: words per row; counts: block rows
    uint64_t *n_out1;   // counts: block columns
    u64 launch_cells;   // 0: PRF_DOT_LAUNCH_CELLS, divided by the filter's cost
    bool bits() const { return block == 0; }
};

struct dot_room {
    u64 n, row0, row1, col0, col1;   // the clipped range and window
    u64 out_rows, out_cols;          // of the output: rows x words, or block rows x block columns
    u64 total() const { return out_rows * out_cols; }
};

// what can be said without a genome; `name` is the entry point
int check_request(const char *name, const dot_request &r, bool counts) {
    if (counts && (r.block < 64 || r.block % 64 || r.block > 32768))
        return fail(PRF_EINVAL, "%s: block is %llu. It must be a multiple of 64, at least 64 and at most 32768.", name, (unsigned long long)r.block);
    if (r.begin > r.end) return fail(PRF_EINVAL, "%s: begin %llu is behind end %llu", name, (unsigned long long)r.begin, (unsigned long long)r.end);
    if (r.row0 > r.row1) return fail(PRF_EINVAL, "%s: row0 %llu is behind row1 %llu", name, (unsigned long long)r.row0, (unsigned long long)r.row1);
    if (r.col0 > r.col1) return fail(PRF_EINVAL, "%s: col0 %llu is behind col1 %llu", name, (unsigned long long)r.col0, (unsigned long long)r.col1);
    if (r.t > PRF_DOT_MAX_RUN)
        return fail(PRF_EUNSUPPORTED, "%s: min_diagonal_run %u is above %u (PRF_DOT_MAX_RUN)", name, r.t, PRF_DOT_MAX_RUN);
    if (!r.dst) return fail(PRF_EINVAL, "%s: NULL destination", name);
    if (!r.n_out0 || (counts && !r.n_out1)) return fail(PRF_EINVAL, "%s: NULL size pointer", name);
    return PRF_OK;
}

// what needs the length of the sequence
int check_room(const char *name, const dot_request &r, u64 seq_len, dot_room *o) {
    const u64 end = r.end < seq_len ? r.end : seq_len;
    o->n = r.begin < end ? end - r.begin : 0;
    if (o->n >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "%s: range too large (2^40 positions)", name);
    o->row1 = r.row1 < o->n ? r.row1 : o->n;
    o->row0 = r.row0 < o->row1 ? r.row0 : o->row1;
    o->col1 = r.col1 < o->n ? r.col1 : o->n;
    o->col0 = r.col0 < o->col1 ? r.col0 : o->col1;
    const u64 rows = o->row1 - o->row0, cols = o->col1 - o->col0;
    const u64 unit = r.bits() ? 64 : r.block;
    o->out_rows = r.bits() ? rows : (rows + unit - 1) / unit;
    o->out_cols = (cols + unit - 1) / unit;
    if (o->total() > r.capacity)
        return fail(PRF_EINVAL, "%s: the destination holds %llu %s, the output has %llu (%llu x %llu)", name, (unsigned long long)r.capacity,
                    r.bits() ? "words" : "counts", (unsigned long long)o->total(), (unsigned long long)o->out_rows,
                    (unsigned long long)o->out_cols);
    if (o->total() > PRF_PERIOD_BITS_MAX_WORDS)
        return fail(PRF_EUNSUPPORTED, "%s: an output of %llu %s is above the limit of %llu per call (PRF_PERIOD_BITS_MAX_WORDS): ask for %s",
                    name, (unsigned long long)o->total(), r.bits() ? "words" : "counts", (unsigned long long)PRF_PERIOD_BITS_MAX_WORDS,
                    r.bits() ? "counts, or for a smaller window" : "a larger block or a smaller window");
    if (rows && cols > PRF_DOT_MAX_CELLS / rows)
        return fail(PRF_EUNSUPPORTED, "%s: a window of %llu x %llu cells is above the limit of 2^42 per call (PRF_DOT_MAX_CELLS)", name,
                    (unsigned long long)rows, (unsigned long long)cols);
    return PRF_OK;
}

int run(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const dot_request &r, prf_scan_stats *stats) {
    if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
    prf_contig_view v;
    int rc = prf_genome_contig_view(g, contig, &v);
    if (rc) return rc;
    if (v.ctx != c) return fail(PRF_EINVAL, "%s: the genome belongs to another context", name);
    dot_room o;
    if ((rc = check_room(name, r, v.len, &o))) return rc;
    if (c->slot[0].seq || c->slot[1].seq) return fail(PRF_EINVAL, "%s: pipelined scans are in flight on this context", name);
    HIPCHK(hipSetDevice(c->dev));
    *r.n_out0 = r.bits() ? o.out_cols : o.out_rows;
    if (r.n_out1) *r.n_out1 = o.out_cols;
    const u64 total = o.total();
    const size_t bytes = (size_t)total * (r.bits() ? sizeof(u64) : sizeof(u32));
    float ms = 0;
    u32 launches = 0;
    if (total) {
        dev_array<unsigned char> d_out;
        if ((rc = d_out.alloc(bytes))) return rc;
        prf_dotplot_args a{};
        a.pl = v.planes;
        a.g_begin = v.base + r.begin;
        a.n = o.n;
        a.row0 = o.row0;
        a.col0 = o.col0;
        a.col1 = o.col1;
        a.words_per_row = (o.col1 - o.col0 + 63) / 64;
        a.m = r.t > 2 ? r.t - 1 : 1;
        a.wpb = r.bits() ? 1u : (u32)(r.block / 64);
        a.n_block_cols = o.out_cols;
        a.bits = r.bits() ? (u64 *)d_out.p : nullptr;
        a.counts = r.bits() ? nullptr : (u32 *)d_out.p;
        u32 tile_rows, span_words, halo;
        prf_dotplot_shape_for(r.t, &tile_rows, &span_words, &halo);
        // rows per launch: whole tiles, at most launch_cells cells and 2^30 workgroups, at least one tile.  The filter costs m^2
        // steps per cell and direction above m = 2, so the default shrinks with it: a launch stays a few ms long.
        const u64 cost = a.m > 2 ? ((u64)a.m * a.m + 3) / 4 : 1;
        const u64 cells = r.launch_cells ? r.launch_cells : PRF_DOT_LAUNCH_CELLS / cost;
        const u64 cols = o.col1 - o.col0;
        const u64 n_spans = (a.words_per_row + span_words - 1) / span_words;
        u64 tiles = cells / cols / tile_rows;
        if (tiles > (1ull << 30) / n_spans) tiles = (1ull << 30) / n_spans;
        if (tiles < 1) tiles = 1;
        if (!r.bits()) HIPCHK(hipMemsetAsync(d_out.p, 0, bytes, c->stream));
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        for (u64 lr = o.row0; lr < o.row1; lr += tiles * tile_rows) {
            a.lrow0 = lr;
            a.lrow1 = o.row1 - lr > tiles * tile_rows ? lr + tiles * tile_rows : o.row1;
            HIPCHK(prf_launch_dotplot(c->stream, a, r.bits()));
            launches++;
        }
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipMemcpyAsync(r.dst, d_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->phase1_ms = ms;
        stats->positions = o.n;
        stats->packed_bytes = (o.n + 3) / 4;
        stats->n_launches = launches;
        stats->path = 5;
    }
    return PRF_OK;
}

int on_genome(const char *name, prf_ctx *c, const prf_genome *g, u32 contig, const dot_request &r, bool counts, prf_scan_stats *stats) {
    return guarded(name, [&] {
        const int rc = check_request(name, r, counts);
        return rc ? rc : run(name, c, g, contig, r, stats);
    });
}

// load + call + free; everything that can be refused from the arguments and the bytes is refused before the context is looked at
int one_shot(const char *name, prf_ctx *c, const prf_contig *seq, const dot_request &r, bool counts, prf_scan_stats *stats) {
    return guarded(name, [&] {
        int rc = check_request(name, r, counts);
        if (rc) return rc;
        if (!seq || (seq->len && !seq->ascii)) return fail(PRF_EINVAL, "%s: NULL sequence", name);
        dot_room o;
        if ((rc = check_room(name, r, seq->len, &o))) return rc;
        for (u64 i = 0; i < seq->len; i++)
            if (!isalpha(seq->ascii[i]) || seq->ascii[i] > 127)
                return fail(PRF_ESYMBOL, "%s: unsupported symbol at position %llu: only letters can be packed", name, (unsigned long long)i);
        if (!c) return fail(PRF_EINVAL, "%s: NULL context", name);
        prf_genome *g = nullptr;
        if ((rc = prf_genome_load(c, seq, 1, 64, &g))) return rc;
        rc = run(name, c, g, 0, r, stats);
        prf_genome_free(g);
        return rc;
    });
}

}  // namespace

extern "C" {

int prf_dotplot_bits_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                        uint64_t col0, uint64_t col1, uint32_t t, uint64_t *dst, uint64_t capacity_words, uint64_t *words_per_row,
                        prf_scan_stats *stats, uint64_t launch_cells) {
    return on_genome("prf_dotplot_bits", c, g, contig,
                     dot_request{begin, end, row0, row1, col0, col1, t, 0, dst, capacity_words, words_per_row, nullptr, launch_cells}, false, stats);
}

int prf_dotplot_counts_ex(prf_ctx *c, const prf_genome *g, uint32_t contig, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1,
                          uint64_t col0, uint64_t col1, uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity,
                          uint64_t *n_block_rows, uint64_t *n_block_cols, prf_scan_stats *stats, uint64_t launch_cells) {
    return on_genome("prf_dotplot_counts", c, g, contig,
                     dot_request{begin, end, row0, row1, col0, col1, t, block, dst, capacity, n_block_rows, n_block_cols, launch_cells}, true, stats);
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
    return one_shot("prf_dotplot_bits_seq", c, seq,
                    dot_request{begin, end, row0, row1, col0, col1, t, 0, dst, capacity_words, words_per_row, nullptr, 0}, false, stats);
}

int prf_dotplot_counts_seq(prf_ctx *c, const prf_contig *seq, uint64_t begin, uint64_t end, uint64_t row0, uint64_t row1, uint64_t col0,
                           uint64_t col1, uint32_t t, uint64_t block, uint32_t *dst, uint64_t capacity, uint64_t *n_block_rows,
                           uint64_t *n_block_cols, prf_scan_stats *stats) {
    return one_shot("prf_dotplot_counts_seq", c, seq,
                    dot_request{begin, end, row0, row1, col0, col1, t, block, dst, capacity, n_block_rows, n_block_cols, 0}, true, stats);
}

int prf_dotplot_shape(uint32_t t, uint32_t *tile_rows, uint32_t *span_words, uint32_t *halo_rows) {
    if (!tile_rows || !span_words || !halo_rows) return fail(PRF_EINVAL, "prf_dotplot_shape: NULL pointer");
    if (t > PRF_DOT_MAX_RUN) return fail(PRF_EUNSUPPORTED, "prf_dotplot_shape: min_diagonal_run %u is above %u (PRF_DOT_MAX_RUN)", t, PRF_DOT_MAX_RUN);
    prf_dotplot_shape_for(t, tile_rows, span_words, halo_rows);
    return PRF_OK;
}

}  // extern "C"
