"""Plot the periodicity matrix for a given input sequence (reference plot_periodicity_matrix.py), computed on the GPU.

The reference's arguments, for a sequence of at most 5,000 positions:
    plot_periodicity_matrix.py CAGCAGCAGCAGTTT --max-motif-size 10 -o matrix.png
Beyond the reference: the input may be a FASTA file with -i chrom:start-end, and --window W turns the matrix into the
periodicity profile -- for every period k and every window of W positions, the number of positions that match their k-th
neighbour -- which has no size limit (a chromosome takes well under a second on the device):
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --window 65536 --tsv profile.tsv
"""
import argparse
import os
import re
import sys

MAX_MATRIX_POSITIONS = 5_000   # the limit the reference puts on what it plots (perfect_repeat_finder.py:176)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("input_sequence", help="The input sequence, or a FASTA file path (then with --interval).")
    p.add_argument("--min-motif-size", default=1, type=int, help="The minimum motif size in base pairs.")
    p.add_argument("--max-motif-size", default=50, type=int, help="The maximum motif size in base pairs.")
    p.add_argument("-o", "--output-path", default="periodicity_matrix.png", help="The output path for the periodicity matrix.")
    p.add_argument("-i", "--interval", help="FASTA input: only consider sequence from this interval (chrom:start_0based-end).")
    p.add_argument("--window", type=int, help="Plot the periodicity profile instead: matches per period and window of this many "
                                              "positions (a multiple of 64). Needed above 5,000 positions.")
    p.add_argument("--tsv", help="With --window: also write the profile as a table: chrom, start, end, k, matches; one line per "
                                 "(window, k) with at least one match.")
    return p


def resolve_input(args, parser):
    """(name, sequence text of the whole record or literal, begin, end) after the checks that need no GPU."""
    if args.min_motif_size < 1:
        parser.error(f"--min-motif-size is set to {args.min_motif_size}. It must be at least 1.")
    if args.max_motif_size < args.min_motif_size:
        parser.error(f"--max-motif-size is set to {args.max_motif_size}. It must be at least --min-motif-size.")
    if args.window is not None and (args.window < 64 or args.window % 64):
        parser.error(f"--window is set to {args.window}. It must be a multiple of 64, at least 64.")
    if args.tsv and args.window is None:
        parser.error("--tsv writes the windowed profile: give --window too")
    if os.path.isfile(args.input_sequence):
        if not args.interval:
            parser.error("A FASTA input needs --interval chrom:start_0based-end")
        parts = re.split("[:-]", args.interval)          # as perfect_repeat_finder.py -i (reference :119)
        if len(parts) != 3:
            parser.error("Invalid --interval format. Must be chrom:start_0based-end")
        chrom, begin, end = parts[0], int(parts[1]), int(parts[2])
        import prf_native
        entries = prf_native.Fasta(args.input_sequence, only=chrom)     # prf_fasta_open_contig: by seeking if there is a .fai
        if chrom not in entries:
            parser.error(f"Chromosome {chrom} not found in the input FASTA file")
        seq = entries[chrom].seq
        end = min(end, len(seq))
        if begin > end:
            parser.error(f"--interval {args.interval}: the start lies behind the end ({end})")
    else:
        if args.interval:
            parser.error("The --interval option is only supported for FASTA files.")
        if not args.input_sequence.isalpha():
            parser.error(f"Invalid input: {args.input_sequence}. This should be a FASTA file path or a string of letters.")
        chrom, seq, begin, end = "sequence", args.input_sequence, 0, len(args.input_sequence)
    if args.window is None and end - begin > MAX_MATRIX_POSITIONS:
        parser.error(f"The input sequence is too long for the full matrix ({end - begin:,d} bp > {MAX_MATRIX_POSITIONS:,d}). "
                     f"Use --window W (a multiple of 64) to plot the periodicity profile instead.")
    return chrom, seq, begin, end


def profile_lines(chrom, begin, end, window, min_motif_size, counts):
    """The --tsv lines of a profile: counts[k - min_motif_size][w] matches of period k in window w of [begin, end)."""
    for w in range(counts.shape[1]):
        start = begin + w * window
        stop = min(start + window, end)
        for r in counts[:, w].nonzero()[0].tolist():
            yield f"{chrom}\t{start}\t{stop}\t{min_motif_size + r}\t{int(counts[r, w])}\n"


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    chrom, seq, begin, end = resolve_input(args, parser)
    from utils.plot_utils import get_period_matrix, plot_periodicity_matrix
    if args.window is None:
        matrix = get_period_matrix(args.min_motif_size, args.max_motif_size, seq[begin:end])
        plot_periodicity_matrix(matrix, args.output_path)
        return
    import prf_native
    ctx = prf_native.default_context()
    genome = ctx.load([seq.encode("ascii", "replace")], args.max_motif_size)
    try:
        counts = genome.period_counts(0, args.min_motif_size, args.max_motif_size, args.window, begin, end)
    finally:
        genome.free()
    if args.tsv:
        with open(args.tsv, "wt") as out:
            out.writelines(profile_lines(chrom, begin, end, args.window, args.min_motif_size, counts))
        print(f"Wrote {args.tsv}")
    n = end - begin
    rows = [[0.0] * counts.shape[1] for _ in range(args.min_motif_size - 1)] + (counts / float(args.window)).tolist()
    # the reference's denominator (utils/plot_utils.py:46): width - period + 1
    fractions = [0.0] * (args.min_motif_size - 1) + [
        float(total) / max(1, n - k + 1) for k, total in zip(range(args.min_motif_size, args.max_motif_size + 1), counts.sum(axis=1))]
    plot_periodicity_matrix(rows, args.output_path, fractions=fractions, extent=(begin, end),
                            value_label=f"Matches per window of {args.window:,d} / window")


if __name__ == "__main__":
    sys.exit(main())
