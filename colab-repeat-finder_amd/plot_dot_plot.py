"""Plot the dot plot of a DNA sequence (reference plot_dot_plot.py), computed on the GPU: pixel (i, j) is dark if positions i and
j hold the same base and the pixel lies on a diagonal or anti-diagonal run of dark pixels of at least --filter-threshold - 1.

The reference's arguments, for sequences of at most 5,000 positions (one pixel per cell):
    plot_dot_plot.py CAGCAGCAGCAGTTTCTGCTGCTG -o dots.png
    plot_dot_plot.py -R genome.fa chr22:1000-3000 regions.bed -p 50 -d plots --show-filtered-pixels
Beyond the reference: --block B turns the plot into a density image -- one pixel per block of B x B cells, grey = kept cells /
cells of the block -- which has no such limit, and --tsv writes the counts:
    plot_dot_plot.py -R genome.fa chr22:20000000-21000000 --block 1024 --tsv density.tsv -o density.png
Also beyond it: --versus X plots the inputs (rows) against another sequence or interval X (columns), a rectangular image, and
--strand - compares with the complement of the columns' bases, so that an inverted repeat shows as an anti-diagonal; --strand both
draws the cells that only the minus strand keeps in a second colour:
    plot_dot_plot.py -R genome.fa chr22:1000-3000 --versus chr21:5000-6500 --strand both -o pair.png
And --runs-tsv lists what the picture shows as coordinates: every maximal diagonal or anti-diagonal run of matching cells of at
least --min-run cells, one line each.  With --runs-tsv and no -o no image is drawn, and no limit on the length applies:
    plot_dot_plot.py -R genome.fa chr22:20000000-21000000 --versus chr22:30000000-31000000 --strand both --runs-tsv runs.tsv --min-run 40
--chains-tsv lists repeats with mismatches: exact runs of at least --min-seed cells on one diagonal or anti-diagonal, joined across
at most --max-gap cells, with their matching cells, joined runs and identity:
    plot_dot_plot.py -R genome.fa chr22:20000000-21000000 --versus chr22:30000000-31000000 --strand both --chains-tsv chains.tsv --min-seed 12 --max-gap 8 --min-chain 100 --min-identity 0.9
--groups-tsv lists repeats with mismatches AND indels: those chains, joined across junctions of at most --max-shift diagonals:
    plot_dot_plot.py -R genome.fa chr22:20000000-21000000 --versus chr22:30000000-31000000 --strand both --groups-tsv groups.tsv --min-seed 12 --max-gap 8 --max-shift 4 --min-group 200 --min-identity 0.85
"""
import argparse
import gzip
import os
import sys

import numpy as np

MAX_MATRIX_POSITIONS = 5_000   # one pixel per cell up to here (the limit of perfect_repeat_finder.py -p); above it: --block


def parse_interval(interval_string):
    """"chr1:12345-54321" -> (chrom, start, end); the chromosome name may itself hold colons."""
    try:
        chrom, _, span = interval_string.rpartition(":")
        start, end = (int(v) for v in span.split("-"))
    except Exception as e:
        raise ValueError(f"Unable to parse interval: '{interval_string}': {e}")
    return chrom, start, end


def _context(context):
    if context is not None:
        return context
    import prf_native
    return prf_native.default_context()


MINUS_ONLY = 3                 # the value of a cell that only the minus strand keeps (--strand both)


def dot_plot_matrix(sequence, min_diagonal_run=3, set_noise_to=0, context=None, versus=None, strand="+"):
    """numpy uint8[n, n]: 1 where the reference's generate_matrix + filter_out_noise(min_diagonal_run) leave a 1, set_noise_to
    where they put set_noise_to, 0 elsewhere -- from the GPU: one call at min_diagonal_run, and one more without a filter if
    the filtered-out cells are wanted.
    versus: the sequence of the columns (None: `sequence` itself), which makes the matrix uint8[len(sequence), len(versus)].
    strand "-": a cell compares a row's base with the complement of the column's base; "both": one call per strand, cells that
    only the minus strand keeps are MINUS_ONLY, filtered-out cells are those that neither strand keeps."""
    import prf_native
    ctx = _context(context)
    columns = sequence if versus is None else versus

    def cells(t):
        if versus is None and strand == "+":
            return prf_native.unpack_bits(ctx.dotplot_bits(sequence, t), len(columns))
        per_strand = [prf_native.unpack_bits(ctx.dotpair_bits(sequence, columns, s, t), len(columns)) for s in "+-" if strand in (s, "both")]
        return per_strand[0] if len(per_strand) == 1 else per_strand[0] | (per_strand[1] << 1)      # bit 0: plus, bit 1: minus

    kept = cells(min_diagonal_run)
    out = np.where(kept == 2, MINUS_ONLY, kept & 1).astype(np.uint8) if strand == "both" else kept
    if not set_noise_to or min_diagonal_run <= 2:
        return out
    raw = cells(0)
    return (out + set_noise_to * ((raw != 0) & (kept == 0))).astype(np.uint8)


def generate_matrix(sequence, context=None):
    """The square list of lists with entry (i, j) == 1 if sequence[i] == sequence[j] (compared in upper case), else 0."""
    return dot_plot_matrix("".join(sequence), 0, context=context).tolist()


def is_noise(matrix, i, j, min_diagonal_run=3):
    """True unless (i, j) lies on a stretch of cells > 0 along one of the two diagonals that is long enough: the cell counts in
    both directions of a diagonal, so a stretch of L cells passes if L + 1 >= min_diagonal_run."""
    size = len(matrix)

    def reach(di, dj):
        steps, a, b = 0, i, j
        while 0 <= a < size and 0 <= b < size and matrix[a][b] > 0:
            a, b, steps = a + di, b + dj, steps + 1
        return steps

    if not (0 <= i < size and 0 <= j < size and matrix[i][j] > 0):
        return True
    return all(reach(1, dj) + reach(-1, -dj) < min_diagonal_run for dj in (1, -1))


def _long_enough(cells, m):
    """bool matrix: the cell is set and lies on a run of at least m set cells along (+1, +1)."""
    n_rows, n_cols = cells.shape
    total = np.zeros(cells.shape, dtype=np.int32)
    for sign in (1, -1):
        alive = cells.copy()
        total += alive
        for v in range(1, m):
            moved = np.zeros_like(cells)
            if v < n_rows and v < n_cols:
                if sign > 0:
                    moved[:-v, :-v] = cells[v:, v:]
                else:
                    moved[v:, v:] = cells[:-v, :-v]
            alive &= moved
            if not alive.any():
                break
            total += alive
    return cells & (total - 1 >= m)


def filter_out_noise(matrix, min_diagonal_run=3, set_noise_to=0):
    """Filters a 0/1 matrix (list of lists or numpy array) in place as the reference does: a cell > 0 that is_noise() becomes
    set_noise_to.  The reference's row-major in-place loop leaves exactly the cells whose diagonal or anti-diagonal stretch in
    the UNFILTERED matrix has L + 1 >= min_diagonal_run; that closed form is computed here with numpy."""
    cells = np.asarray(matrix) > 0
    if cells.size == 0 or min_diagonal_run <= 2:
        return
    m = min_diagonal_run - 1
    kept = _long_enough(cells, m) | _long_enough(cells[:, ::-1], m)[:, ::-1]
    noise = cells & ~kept
    if isinstance(matrix, np.ndarray):
        matrix[noise] = set_noise_to
        return
    for i in np.flatnonzero(noise.any(axis=1)).tolist():
        row = matrix[i]
        for j in np.flatnonzero(noise[i]).tolist():
            row[j] = set_noise_to


# cell values 0 (empty), 1 (kept), 2 (filtered out, --show-filtered-pixels), 3 (kept on the minus strand only, --strand both)
PALETTE = ("white", "black", "red", "royalblue")


def _draw(image, save_path, show, figure_size, **imshow):
    """One image without ticks, with a thin grey frame, cropped to the axes when saved: figure_size inches along its longer
    side, the other side in proportion (a square for a square matrix)."""
    import matplotlib
    if not show:
        matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    n_rows, n_cols = np.shape(image) if np.ndim(image) == 2 else (0, 0)
    longer = max(n_rows, n_cols, 1)
    fig, ax = plt.subplots(figsize=(figure_size * max(n_cols, 1) / longer, figure_size * max(n_rows, 1) / longer) if n_rows != n_cols
                           else (figure_size, figure_size))
    if n_rows and n_cols:
        ax.imshow(image, interpolation="nearest", **imshow)
    ax.tick_params(left=False, bottom=False, labelleft=False, labelbottom=False)
    for side in ("left", "right", "top", "bottom"):
        ax.spines[side].set(color="#CCCCCC", linewidth=0.5)
    if show:
        plt.show()
    if save_path:
        fig.savefig(save_path, bbox_inches="tight", pad_inches=0)
    plt.close(fig)


def plot_dot_plot(matrix, save_path=None, show=False, figure_size=None):
    """Draw the matrix as an image, square for a square matrix: 0 white, 1 black, 2 (filtered-out cells) red, 3 (cells of the
    minus strand only) blue.  figure_size (inches, the longer side) defaults to the reference's 5 * len(matrix) / 150."""
    from matplotlib.colors import ListedColormap
    size = max(np.shape(matrix)) if np.ndim(matrix) == 2 else len(matrix)
    top = int(np.max(matrix)) if np.size(matrix) else 0
    _draw(matrix, save_path, show, max(5 * size / 150, 0.2) if figure_size is None else figure_size,
          cmap=ListedColormap(list(PALETTE[:top + 1])), vmin=0, vmax=top)


def plot_density(counts, block, n, save_path=None, show=False, figure_size=None, n_cols=None):
    """Draw block counts (dotplot_counts of an n x n matrix, or dotpair_counts of an n x n_cols one) as a grey image: kept cells /
    cells of the (clipped) block."""
    edges = [np.minimum(block, length - block * np.arange(blocks)).astype(np.float64)
             for length, blocks in zip((n, n if n_cols is None else n_cols), counts.shape)]
    density = counts / np.outer(*edges)
    _draw(density, save_path, show, min(max(5 * max(counts.shape) / 150, 2.0), 40.0) if figure_size is None else figure_size,
          cmap="gray_r", vmin=0.0, vmax=1.0)


def density_lines(name, begin, n, block, counts, col_begin=None, n_cols=None):
    """The --tsv lines: name, row start, row end, column start, column end, kept cells; one line per block with a kept cell.
    col_begin, n_cols: where the columns begin and how many they are, if not as the rows (--versus)."""
    col_begin, n_cols = begin if col_begin is None else col_begin, n if n_cols is None else n_cols
    for r, c in zip(*(v.tolist() for v in counts.nonzero())):
        yield (f"{name}\t{begin + r * block}\t{begin + min(n, (r + 1) * block)}\t{col_begin + c * block}\t"
               f"{col_begin + min(n_cols, (c + 1) * block)}\t{int(counts[r, c])}\n")


def run_lines(name, begin, x_name, x_begin, strand, runs):
    """The --runs-tsv lines of a list of runs (fields row, col, len, dir): name, a_start, a_end, X's name, b_start, b_end, strand,
    direction, length -- genomic coordinates, ends exclusive, the columns' in forward coordinates on both strands: an anti run
    (row + s, col - s) covers columns col - len + 1 .. col."""
    for row, col, length, direction in zip(*(runs[f].tolist() for f in ("row", "col", "len", "dir"))):
        b_start = x_begin + (col if direction == 1 else col - length + 1)
        yield (f"{name}\t{begin + row}\t{begin + row + length}\t{x_name}\t{b_start}\t{b_start + length}\t{strand}\t"
               f"{'main' if direction == 1 else 'anti'}\t{length}\n")


def list_runs(ctx, seq, min_len, directions="both", versus=None, strand="+"):
    """[(strand, runs)] of seq against versus, or against itself (then without the trivial diagonal and with one run of each
    mirror pair: prf_native.unique_runs), one entry per strand of "+", "-" or "both"."""
    import prf_native
    out = []
    for s in "+-":
        if strand in (s, "both"):
            runs = ctx.dotpair_runs(seq, seq if versus is None else versus, s, directions, min_len)
            out.append((s, prf_native.unique_runs(runs, s) if versus is None else runs))
    return out


def chain_lines(name, begin, x_name, x_begin, strand, chains):
    """The --chains-tsv lines of a list of chains (fields row, col, len, matches, dir, seeds): the columns of run_lines, then the
    matching cells, the seeds and the identity matches / len to four decimals."""
    lines = run_lines(name, begin, x_name, x_begin, strand, chains)
    for line, matches, seeds, length in zip(lines, *(chains[f].tolist() for f in ("matches", "seeds", "len"))):
        yield f"{line[:-1]}\t{matches}\t{seeds}\t{matches / length:.4f}\n"


def list_chains(ctx, seq, min_seed, max_gap, min_len=0, min_identity=None, directions="both", versus=None, strand="+"):
    """[(strand, chains)] of seq against versus, or against itself (then through prf_native.unique_chains), one entry per strand of
    "+", "-" or "both"; min_identity filters here, on matches / len."""
    import prf_native
    out = []
    for s in "+-":
        if strand in (s, "both"):
            chains = ctx.dotpair_chains(seq, seq if versus is None else versus, s, directions, min_seed, max_gap, min_len)
            if versus is None:
                chains = prf_native.unique_chains(chains, s)
            if min_identity is not None:
                chains = chains[prf_native.chain_identity(chains) >= min_identity]
            out.append((s, chains))
    return out


def group_lines(name, begin, x_name, x_begin, strand, groups):
    """The --groups-tsv lines of a list of groups (prf_native.join_chains): name, a_start, a_end, X's name, b_start, b_end (ends
    exclusive, forward coordinates on both strands), strand, direction, the rows and the columns spanned, the matching cells, the
    chains, the seeds, the inserted or deleted bases (the sum of |shift|), the cells of the junctions' gaps, 1 if the group begins
    outside the rectangle's window (0 otherwise) and the identity matches / max(span_a, span_b) to four decimals."""
    import prf_native
    fields = ("row", "col", "end_row", "end_col", "dir", "span_a", "span_b", "matches", "chains", "seeds", "indel", "gap_cells", "open")
    identity = prf_native.group_identity(groups).tolist()
    for (row, col, end_row, end_col, direction, span_a, span_b, matches, chains, seeds, indel, gap_cells, is_open), share in zip(
            zip(*(groups[f].tolist() for f in fields)), identity):
        yield (f"{name}\t{begin + row}\t{begin + end_row + 1}\t{x_name}\t{x_begin + min(col, end_col)}\t{x_begin + max(col, end_col) + 1}\t"
               f"{strand}\t{'main' if direction == 1 else 'anti'}\t{span_a}\t{span_b}\t{matches}\t{chains}\t{seeds}\t{indel}\t{gap_cells}\t"
               f"{int(is_open)}\t{share:.4f}\n")


def list_groups(ctx, seq, min_seed, max_gap, max_shift, min_group=0, min_identity=None, directions="both", versus=None, strand="+"):
    """[(strand, groups)] of seq against versus, or against itself (then BOTH mirror images are listed: the tie-break on the sign
    of the shift is not mirror-symmetric), one entry per strand of "+", "-" or "both": the chains at min_len = 0 and the links of
    the whole rectangle, folded by prf_native.join_chains; min_group (on the longer span) and min_identity filter here."""
    import prf_native
    out = []
    columns = seq if versus is None else versus
    for s in "+-":
        if strand in (s, "both"):
            chains = ctx.dotpair_chains(seq, columns, s, directions, min_seed, max_gap, 0)
            links = ctx.dotpair_links(seq, columns, s, directions, min_seed, max_gap, max_shift)
            groups = prf_native.join_chains(chains, links, len(columns))
            if min_group:
                groups = groups[np.maximum(groups["span_a"], groups["span_b"]) >= min_group]
            if min_identity is not None:
                groups = groups[prf_native.group_identity(groups) >= min_identity]
            out.append((s, groups))
    return out


def no_image(args):
    """--runs-tsv, --chains-tsv or --groups-tsv without -o: the list is all that is asked for."""
    return (args.runs_tsv is not None or args.chains_tsv is not None or args.groups_tsv is not None) and args.output_path is None


def build_parser():
    """The reference's options and positionals (names as there, so that its command lines run unchanged), plus --block / --tsv."""
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-w", "--image-size", type=float, help="side of the square image, in inches (default: 5/150 inch per cell)")
    p.add_argument("-d", "--output-dir", default=".", help="directory the images go to; created if missing")
    p.add_argument("-o", "--output-path", help="file name of the image when there is exactly one input (default: dot_plot.png)")
    p.add_argument("-t", "--filter-threshold", type=int, default=3,
                   help="min_diagonal_run of the noise filter, 0 to 64: a cell stays if its diagonal or anti-diagonal run has "
                        "at least this many cells minus one; 2 or less keeps every cell")
    p.add_argument("-p", "--padding", type=int, default=0, help="widen every interval by this many positions on both sides")
    p.add_argument("--show-filtered-pixels", action="store_true", help="draw the cells the filter removed in red")
    p.add_argument("--show-plot", action="store_true", help="open each image in a window as well")
    p.add_argument("-R", "--reference-fasta", help="FASTA file that intervals and BED lines refer to")
    p.add_argument("-v", "--verbose", action="store_true", help="report every sequence as it is plotted")
    p.add_argument("--block", type=int, help="Plot the density instead: one pixel per block of this many x this many cells (a "
                                             "multiple of 64, at most 32768). Needed above 5,000 positions.")
    p.add_argument("--tsv", help="With --block: also write the block counts as a table. With --versus the name and the row "
                                 "coordinates are the input's, the column coordinates are X's.")
    p.add_argument("--versus", metavar="X", help="Plot every input (the rows) against X (the columns) instead of against itself: a "
                                                 "literal ACGT sequence, or an interval chrom:start_0based-end with -R.")
    p.add_argument("--strand", choices=["+", "-", "both"], default="+",
                   help="-: compare each row's base with the complement of the column's base, so that an inverted repeat is an "
                        "anti-diagonal; both: draw the cells that only the minus strand keeps in a second colour (one pixel per "
                        "cell only: with --block, plot one strand at a time)")
    p.add_argument("--runs-tsv", metavar="PATH",
                   help="Write the maximal diagonal and anti-diagonal runs of matching cells as a table: name, a_start, a_end, X's "
                        "name, b_start, b_end (ends exclusive, forward coordinates on both strands), strand, direction, length. "
                        "Needs --min-run. Without --versus each repeat is listed once and the trivial diagonal not at all. "
                        "Without -o no image is drawn, and sequences above 5,000 positions need no --block.")
    p.add_argument("--min-run", type=int, metavar="L", help="With --runs-tsv: the cells a run must have to be listed.")
    p.add_argument("--run-directions", choices=["main", "anti", "both"], default="both",
                   help="With --runs-tsv, --chains-tsv or --groups-tsv: list diagonal runs, anti-diagonal runs or both (default).")
    p.add_argument("--chains-tsv", metavar="PATH",
                   help="Write the diagonal repeats with mismatches as a table: exact runs of at least --min-seed cells on one "
                        "diagonal or anti-diagonal, joined wherever at most --max-gap cells lie between two of them. The columns of "
                        "--runs-tsv (the length is the chain's span), then the matching cells, the joined runs and the identity "
                        "(matches / span, four decimals). Needs --min-seed and --max-gap. Without --versus each repeat is listed "
                        "once; without -o no image is drawn, and sequences above 5,000 positions need no --block.")
    p.add_argument("--min-seed", type=int, metavar="S",
                   help="With --chains-tsv or --groups-tsv: the cells an exact run must have to be joined or listed.")
    p.add_argument("--max-gap", type=int, metavar="G",
                   help="With --chains-tsv or --groups-tsv: the most cells between two joined runs, 0 to 4096.")
    p.add_argument("--min-chain", type=int, metavar="L", help="With --chains-tsv: the cells a chain must span to be listed (default: no limit).")
    p.add_argument("--min-identity", type=float, metavar="F",
                   help="With --chains-tsv or --groups-tsv: list the chains (groups) with matches / span of at least this, 0 to 1.")
    p.add_argument("--groups-tsv", metavar="PATH",
                   help="Write the repeats with mismatches and indels as a table: the chains of --chains-tsv at --min-seed and "
                        "--max-gap, joined across junctions to a chain that starts 1 to --max-shift diagonals away, on the whole "
                        "rectangle of the two ranges. One line per group: name, a_start, a_end, X's name, b_start, b_end, strand, "
                        "direction, rows spanned, columns spanned, matching cells, chains, seeds, inserted or deleted bases, cells "
                        "of the junctions' gaps, 0 (1: the group begins outside the rectangle) and the identity matches / longer "
                        "span. Needs --min-seed, --max-gap and --max-shift. Without --versus BOTH mirror images of a repeat are "
                        "written (the tie-break between an insertion and a deletion is not mirror-symmetric) and the trivial "
                        "diagonal too; without -o no image is drawn, and sequences above 5,000 positions need no --block.")
    p.add_argument("--max-shift", type=int, metavar="D", help="With --groups-tsv: the most diagonals between two joined chains, 1 to 32.")
    p.add_argument("--min-group", type=int, metavar="L",
                   help="With --groups-tsv: the rows or columns a group must span to be listed (default: no limit).")
    p.add_argument("input_sequence_or_intervals_or_bed_files", nargs="+",
                   help="any mix of literal ACGT sequences, intervals chrom:start_0based-end, and BED files")
    return p


def _fetch(parser, fasta_path, cache, chrom, start, end):
    """(name in the file, sequence[start:end] in upper case): the name as given, or with / without a "chr" prefix."""
    import prf_native
    bare = chrom.replace("chr", "")
    for name in (chrom, f"chr{bare}", bare):
        if name not in cache:
            entries = prf_native.Fasta(fasta_path, only=name)
            cache[name] = entries[name].seq if name in entries else None
        if cache[name] is not None:
            return name, cache[name][start:end].upper()
    parser.error(f"Error: {chrom} not found in {fasta_path}")


def resolve_inputs(args, parser):
    """[(name, begin, sequence, output file name)] after the checks that need no GPU; prints what the reference prints."""
    if not 0 <= args.filter_threshold <= 64:
        parser.error(f"--filter-threshold is set to {args.filter_threshold}. It must be between 0 and 64.")
    if args.block is not None and (args.block < 64 or args.block % 64 or args.block > 32768):
        parser.error(f"--block is set to {args.block}. It must be a multiple of 64, at least 64 and at most 32768.")
    if args.tsv and args.block is None:
        parser.error("--tsv writes the block counts: give --block too")
    if args.block is not None and args.strand == "both":
        parser.error("--strand both colours single cells: with --block, plot one strand at a time (--strand + and --strand -)")
    if args.runs_tsv is not None and args.min_run is None:
        parser.error("--runs-tsv lists the runs of at least --min-run cells: give --min-run too")
    if args.min_run is not None and (args.runs_tsv is None or args.min_run < 1):
        parser.error(f"--min-run is set to {args.min_run}. It goes with --runs-tsv and must be at least 1.")
    if args.chains_tsv is not None and (args.min_seed is None or args.max_gap is None):
        parser.error("--chains-tsv joins runs of at least --min-seed cells across at most --max-gap cells: give --min-seed and --max-gap too")
    if args.groups_tsv is not None and (args.min_seed is None or args.max_gap is None or args.max_shift is None):
        parser.error("--groups-tsv joins the chains of --min-seed and --max-gap across at most --max-shift diagonals: give --min-seed, "
                     "--max-gap and --max-shift too")
    for option, value in (("--min-seed", args.min_seed), ("--max-gap", args.max_gap), ("--min-identity", args.min_identity)):
        if value is not None and args.chains_tsv is None and args.groups_tsv is None:
            parser.error(f"{option} goes with --chains-tsv or --groups-tsv")
    if args.min_chain is not None and args.chains_tsv is None:
        parser.error("--min-chain goes with --chains-tsv")
    for option, value in (("--max-shift", args.max_shift), ("--min-group", args.min_group)):
        if value is not None and args.groups_tsv is None:
            parser.error(f"{option} goes with --groups-tsv")
    if args.max_shift is not None and not 1 <= args.max_shift <= 32:
        parser.error(f"--max-shift is set to {args.max_shift}. It must be between 1 and 32.")
    if args.min_group is not None and args.min_group < 0:
        parser.error(f"--min-group is set to {args.min_group}. It must be at least 0.")
    if args.min_seed is not None and args.min_seed < 1:
        parser.error(f"--min-seed is set to {args.min_seed}. It must be at least 1.")
    if args.max_gap is not None and not 0 <= args.max_gap <= 4096:
        parser.error(f"--max-gap is set to {args.max_gap}. It must be between 0 and 4096.")
    if args.min_chain is not None and args.min_chain < 0:
        parser.error(f"--min-chain is set to {args.min_chain}. It must be at least 0.")
    if args.min_identity is not None and not 0 <= args.min_identity <= 1:
        parser.error(f"--min-identity is set to {args.min_identity}. It must be between 0 and 1.")
    inputs = args.input_sequence_or_intervals_or_bed_files
    out, n_intervals, cache = [], 0, {}
    for i, text in enumerate(inputs):
        if not set(text) - set("ACGT"):                               # a literal nucleotide sequence
            name = (args.output_path or "dot_plot.png") if len(inputs) == 1 else f"dot_plot_{i + 1:03d}_of_{len(inputs)}.{len(text)}bp_sequence.png"
            out.append(("sequence", 0, text, os.path.join(args.output_dir, name)))
            continue
        if "bed" not in text and not (":" in text and "-" in text):
            parser.error(f"Error: {text} is not a valid nucleotide sequence, BED file path, or interval")
        if not args.reference_fasta:
            parser.error("Error: --reference-fasta is required when the input is a BED file or interval")
        intervals = []
        if "bed" in text:
            if not os.path.isfile(text):
                parser.error(f"Error: {text} file not found")
            with (gzip.open if text.endswith("gz") else open)(text, "rt") as bed_file:
                for line_i, line in enumerate(bed_file):
                    fields = line.strip().split("\t")
                    if len(fields) < 3:
                        parser.error(f"Error: {text} line #{line_i + 1} is invalid: '{line.strip()}'")
                    intervals.append((fields[0], int(fields[1]), int(fields[2])))
        else:
            try:
                intervals.append(parse_interval(text))
            except ValueError as e:
                parser.error(f"Error: {e}")
        for k, (chrom, start, end) in enumerate(intervals):
            start, end = max(0, start - args.padding), end + args.padding     # (the reference lets a padded start go negative)
            name, seq = _fetch(parser, args.reference_fasta, cache, chrom, start, end)
            out.append((name, start, seq, os.path.join(
                args.output_dir, f"dot_plot_{k + 1:03d}_of_{len(intervals)}.{name}_{start}-{end}.{len(seq)}bp_sequence.png")))
        n_intervals += len(intervals)
    if n_intervals:                                                    # (the reference prints this line always, and crashes
        print(f"Loaded {n_intervals:,d} interval(s) from {args.reference_fasta}")   # on it when there were only literals)
    for name, _begin, seq, _path in out:
        if args.block is None and len(seq) > MAX_MATRIX_POSITIONS and not no_image(args):
            parser.error(f"The input sequence is too long for one pixel per cell ({len(seq):,d} bp > {MAX_MATRIX_POSITIONS:,d}). "
                         f"Use --block B (a multiple of 64) to plot the density instead.")
        if not seq.isalpha() and seq:
            parser.error(f"Error: the sequence of {name} holds characters that are not letters")
    if (args.tsv or args.runs_tsv or args.chains_tsv or args.groups_tsv) and len(out) > 1:
        parser.error(f"{'--tsv' if args.tsv else '--runs-tsv' if args.runs_tsv else '--chains-tsv' if args.chains_tsv else '--groups-tsv'} "
                     "takes one input sequence")
    return out


def resolve_versus(args, parser):
    """None, or (name, begin, sequence) of --versus: a literal sequence or an interval of --reference-fasta, widened by --padding
    like the inputs and under the same limit without --block."""
    text = args.versus
    if text is None:
        return None
    if not set(text) - set("ACGT"):
        name, begin, seq = "sequence", 0, text
    else:
        if not (":" in text and "-" in text):
            parser.error(f"Error: --versus {text} is not a valid nucleotide sequence or interval")
        if not args.reference_fasta:
            parser.error("Error: --reference-fasta is required when --versus is an interval")
        try:
            chrom, start, end = parse_interval(text)
        except ValueError as e:
            parser.error(f"Error: {e}")
        begin, end = max(0, start - args.padding), end + args.padding
        name, seq = _fetch(parser, args.reference_fasta, {}, chrom, begin, end)
    if args.block is None and len(seq) > MAX_MATRIX_POSITIONS and not no_image(args):
        parser.error(f"The --versus sequence is too long for one pixel per cell ({len(seq):,d} bp > {MAX_MATRIX_POSITIONS:,d}). "
                     f"Use --block B (a multiple of 64) to plot the density instead.")
    if not seq.isalpha() and seq:
        parser.error(f"Error: the sequence of {name} holds characters that are not letters")
    return name, begin, seq


def density_counts(ctx, seq, block, min_diagonal_run, versus=None, strand="+"):
    """uint32 block counts of seq against itself, or against versus, on one strand: the self plot's call where it serves."""
    if versus is None and strand == "+":
        return ctx.dotplot_counts(seq, block, min_diagonal_run)
    return ctx.dotpair_counts(seq, seq if versus is None else versus, block, strand, min_diagonal_run)


def main(argv=None, context=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    todo = resolve_inputs(args, parser)
    versus = resolve_versus(args, parser)
    os.makedirs(args.output_dir, exist_ok=True)
    for i, (name, begin, seq, path) in enumerate(todo):
        if args.verbose:
            print(f"[{i + 1}/{len(todo)}] {name}: {len(seq):,d} positions")
        columns = seq if versus is None else versus[2]
        if args.runs_tsv:
            x_name, x_begin = (name, begin) if versus is None else versus[:2]
            listed = list_runs(_context(context), seq, args.min_run, args.run_directions, None if versus is None else columns, args.strand)
            with open(args.runs_tsv, "wt") as f:
                for strand, runs in listed:
                    f.writelines(run_lines(name, begin, x_name, x_begin, strand, runs))
            print(f"Wrote {args.runs_tsv} ({sum(len(runs) for _, runs in listed):,d} runs)")
        if args.chains_tsv:
            x_name, x_begin = (name, begin) if versus is None else versus[:2]
            listed = list_chains(_context(context), seq, args.min_seed, args.max_gap, args.min_chain or 0, args.min_identity,
                                 args.run_directions, None if versus is None else columns, args.strand)
            with open(args.chains_tsv, "wt") as f:
                for strand, chains in listed:
                    f.writelines(chain_lines(name, begin, x_name, x_begin, strand, chains))
            print(f"Wrote {args.chains_tsv} ({sum(len(chains) for _, chains in listed):,d} chains)")
        if args.groups_tsv:
            x_name, x_begin = (name, begin) if versus is None else versus[:2]
            listed = list_groups(_context(context), seq, args.min_seed, args.max_gap, args.max_shift, args.min_group or 0, args.min_identity,
                                 args.run_directions, None if versus is None else columns, args.strand)
            with open(args.groups_tsv, "wt") as f:
                for strand, groups in listed:
                    f.writelines(group_lines(name, begin, x_name, x_begin, strand, groups))
            print(f"Wrote {args.groups_tsv} ({sum(len(groups) for _, groups in listed):,d} groups)")
        if no_image(args):
            continue
        if args.block is None:
            matrix = dot_plot_matrix(seq, args.filter_threshold, 2 if args.show_filtered_pixels else 0, context=context,
                                     versus=None if versus is None else columns, strand=args.strand)
            plot_dot_plot(matrix, save_path=path, show=args.show_plot, figure_size=args.image_size)
        else:
            counts = density_counts(_context(context), seq, args.block, args.filter_threshold, None if versus is None else columns,
                                    args.strand)
            plot_density(counts, args.block, len(seq), save_path=path, show=args.show_plot, figure_size=args.image_size,
                         n_cols=len(columns))
            if args.tsv:
                with open(args.tsv, "wt") as f:
                    f.writelines(density_lines(name, begin, len(seq), args.block, counts, begin if versus is None else versus[1],
                                               len(columns)))
                print(f"Wrote {args.tsv}")
        if args.verbose or len(todo) == 1:
            print(f"Wrote {path} ({len(seq):,d} positions)")
    if not no_image(args):
        print(f"{len(todo):,d} dot plot(s) written to {os.path.abspath(args.output_dir)}")


if __name__ == "__main__":
    sys.exit(main())
