"""Plot the periodicity matrix for a given input sequence (reference plot_periodicity_matrix.py), computed on the GPU.

The reference's arguments, for a sequence of at most 5,000 positions:
    plot_periodicity_matrix.py CAGCAGCAGCAGTTT --max-motif-size 10 -o matrix.png
Beyond the reference: the input may be a FASTA file with -i chrom:start-end, and --window W turns the matrix into the
periodicity profile -- for every period k and every window of W positions, the number of positions that match their k-th
neighbour -- which has no size limit (a chromosome takes well under a second on the device):
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --window 65536 --tsv profile.tsv
--chains-tsv lists the DIVERGED TANDEM REPEATS of the input instead: on every period line, exact runs of at least --min-seed
positions joined across at most --max-gap mismatching ones; it needs neither --window nor an image:
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --chains-tsv repeats.tsv --min-seed 12 --max-gap 8
With --consensus the list also says WHAT each repeat is: its consensus motif (the majority letter of every column), the identity
against that motif, the motif's own smallest period and the catalogue key (least rotation of the motif or its reverse complement):
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --chains-tsv repeats.tsv --min-seed 12 --max-gap 8 --consensus
--groups-tsv lists the GAPPED tandem repeats: those chains joined across indels of at most --max-shift bases (the junctions
between neighbouring period lines), one line per repeat with substitutions and indels:
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --groups-tsv vntr.tsv --min-seed 12 --max-gap 8 --max-shift 4
With --group-consensus that list says WHAT each gapped repeat is as well: the consensus motif of its largest piece (the stretch
over which isolated indels decide the column of every base), counted over segments with a phase:
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --groups-tsv vntr.tsv --min-seed 12 --max-gap 8 --max-shift 4 --group-consensus
With --align on top of either, the list says HOW FAR each repeat is from its motif: substitutions, insertions and deletions of
the best alignment of the whole repeat to the endless repetition of the motif, the aligned identity and the aligned copies:
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --groups-tsv vntr.tsv --min-seed 12 --max-gap 8 --max-shift 4 --group-consensus --align
--align-path adds the alignment itself as a CIGAR, --refine R re-estimates each motif from its aligned copies and aligns again,
--copies-tsv lists where each copy begins and ends and what it differs in:
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --groups-tsv vntr.tsv --min-seed 12 --max-gap 8 --max-shift 4 --group-consensus --align --align-path --refine 2 --copies-tsv copies.tsv
--extend F gives every repeat SCORED BOUNDARIES: the best local alignment of the repeat padded by F positions on both sides against
the endless repetition of its motif, under --weights match,mismatch,indel (TRF's 2,7,7 by default); --min-score filters by it:
    plot_periodicity_matrix.py genome.fa -i chr22:0-50818468 --max-motif-size 1000 --groups-tsv vntr.tsv --min-seed 12 --max-gap 8 --max-shift 4 --group-consensus --extend 50 --min-score 50
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
    p.add_argument("--chains-tsv", help="List the diverged tandem repeats instead of plotting: one line per repeat with chrom, "
                                        "start, end, k, copies, identity, matches, seeds and the first k bases. Needs --min-seed "
                                        "and --max-gap; no image is written.")
    p.add_argument("--groups-tsv", help="List the gapped tandem repeats instead of plotting: the chains of --chains-tsv joined across "
                                        "indels, one line per repeat with chrom, start, end, period, copies, identity, indel, "
                                        "chains, seeds and the first `period` bases. Needs --min-seed, --max-gap and --max-shift; "
                                        "no image is written.")
    p.add_argument("--max-shift", type=int, help="With --groups-tsv: period lines a junction may reach: the longest indel (1 .. 32).")
    p.add_argument("--min-group", type=int, default=0, help="With --groups-tsv: keep repeats that cover at least this many positions "
                                                            "(end - start).")
    p.add_argument("--keep-covered", action="store_true", help="With --groups-tsv: keep the repeats that one of a smaller period "
                                                               "covers (the images at multiples of a period among them).")
    p.add_argument("--min-seed", type=int, help="With --chains-tsv: positions an exact run must match its k-th neighbour to count.")
    p.add_argument("--max-gap", type=int, help="With --chains-tsv: mismatching positions two runs are joined across (0 .. 4096).")
    p.add_argument("--min-chain", type=int, default=0, help="With --chains-tsv: keep repeats of at least this many cells "
                                                            "(end - start - k).")
    p.add_argument("--min-identity", type=float, default=0.0, help="With --chains-tsv or --groups-tsv: keep repeats of at least this identity.")
    p.add_argument("--keep-multiples", action="store_true", help="With --chains-tsv: keep the images of a repeat at multiples of "
                                                                 "its period.")
    p.add_argument("--n-matches", action="store_true", help="With --chains-tsv or --groups-tsv: N matches N, as in the matrix (default: N never "
                                                            "matches, as in the scans).")
    p.add_argument("--chain-window", type=int, default=1 << 22, help="With --chains-tsv or --groups-tsv: start positions per call.")
    p.add_argument("--consensus", action="store_true", help="With --chains-tsv: append four columns per repeat: the consensus motif "
                                                            "(majority letter per column), the identity against it, the motif's "
                                                            "primitive period and its canonical form (least rotation of the motif "
                                                            "or its reverse complement).")
    p.add_argument("--min-consensus-identity", type=float, help="With --consensus: keep repeats of at least this identity against "
                                                                "their consensus motif.")
    p.add_argument("--group-consensus", action="store_true", help="With --groups-tsv: append six columns per repeat: the consensus "
                                                                  "motif of its largest piece, the identity against it, the "
                                                                  "motif's primitive period, its canonical form, the number of "
                                                                  "pieces the repeat was cut into and the share of the repeat "
                                                                  "that the chosen piece covers.")
    p.add_argument("--min-group-consensus-identity", type=float, help="With --group-consensus: keep repeats of at least this "
                                                                      "identity against their consensus motif.")
    p.add_argument("--align", action="store_true", help="With --consensus or --group-consensus: append six columns per repeat: "
                   "edits, substitutions, insertions and deletions of the best alignment of the repeat to the endless repetition of "
                   "its consensus motif (unit costs, free at both ends of the motif), the aligned identity (matches / (positions + "
                   "deletions)) and the aligned copies (motif letters the alignment runs over / period).  A '.' in all six: a "
                   "repeat above a limit of one alignment.")
    p.add_argument("--min-aligned-identity", type=float, help="With --align: keep repeats of at least this aligned identity.")
    p.add_argument("--align-path", action="store_true", help="With --align: append a column `cigar`: the alignment itself as run "
                   "lengths of = (match), X (substitution), I (inserted base) and D (deleted motif letter).")
    p.add_argument("--refine", type=int, default=0, metavar="R", help="With --align: re-estimate every motif from its aligned "
                   "copies and align again, R rounds at most; the reported motif, its canonical form and the columns of --align are "
                   "those of the last round, and a column `refined` says in how many rounds the motif changed.")
    p.add_argument("--copies-tsv", help="With --align: also write one line per aligned copy of every listed repeat: chrom, start, "
                                        "end and period of the repeat, the copy's number, start and end, its substitutions, "
                                        "insertions and deletions.")
    p.add_argument("--extend", type=int, metavar="F", help="With --consensus or --group-consensus: append three columns per repeat: "
                   "ext_start, ext_end and score of the best local alignment of the repeat padded by F positions on both sides "
                   "against the endless repetition of its motif; of equal scores the alignment that ends first and begins last.  A "
                   "'.' in all three: a repeat above a limit of one alignment.  A score of 0: nothing matches, and the interval is "
                   "the repeat's own.")
    p.add_argument("--weights", metavar="M,X,G", help="With --extend: the score is M * matches - X * substitutions - G * (insertions "
                   "+ deletions); each 1 .. 16 (default: 2,7,7).")
    p.add_argument("--min-score", type=int, metavar="S", help="With --extend: keep repeats of at least this score.")
    return p


def parse_weights(text, parser):
    """(match, mismatch, indel) of --weights M,X,G."""
    if text is None:
        return 2, 7, 7
    if not re.fullmatch(r"\d+,\d+,\d+", text):
        parser.error(f"--weights is set to {text!r}. It must be three numbers match,mismatch,indel, such as 2,7,7.")
    weights = tuple(int(w) for w in text.split(","))
    for name, w in zip(("match", "mismatch", "indel"), weights):
        if not 1 <= w <= 16:
            parser.error(f"--weights: {name} is set to {w}. It must be 1 .. 16.")
    return weights


def check_chain_args(args, parser):
    """The checks of the --chains-tsv and --groups-tsv arguments, which need no GPU."""
    if args.consensus and args.groups_tsv:
        parser.error("--consensus goes with --chains-tsv: the columns of a gapped repeat drift at an indel, and its consensus needs "
                     "the phase of every chain")
    if args.consensus and not args.chains_tsv:
        parser.error("--consensus belongs to --chains-tsv")
    if args.min_consensus_identity is not None:
        if not args.consensus:
            parser.error("--min-consensus-identity belongs to --consensus")
        if not 0.0 <= args.min_consensus_identity <= 1.0:
            parser.error(f"--min-consensus-identity is set to {args.min_consensus_identity}. It must be 0 .. 1.")
    if args.group_consensus and not args.groups_tsv:
        parser.error("--group-consensus belongs to --groups-tsv")
    if args.min_group_consensus_identity is not None:
        if not args.group_consensus:
            parser.error("--min-group-consensus-identity belongs to --group-consensus")
        if not 0.0 <= args.min_group_consensus_identity <= 1.0:
            parser.error(f"--min-group-consensus-identity is set to {args.min_group_consensus_identity}. It must be 0 .. 1.")
    if args.align and not (args.consensus or args.group_consensus):
        parser.error("--align needs the motifs of --consensus (with --chains-tsv) or --group-consensus (with --groups-tsv)")
    if args.min_aligned_identity is not None:
        if not args.align:
            parser.error("--min-aligned-identity belongs to --align")
        if not 0.0 <= args.min_aligned_identity <= 1.0:
            parser.error(f"--min-aligned-identity is set to {args.min_aligned_identity}. It must be 0 .. 1.")
    if not args.align:
        for name in ("align_path", "refine", "copies_tsv"):
            if getattr(args, name):
                parser.error(f"--{name.replace('_', '-')} belongs to --align")
    if not 0 <= args.refine <= 100:
        parser.error(f"--refine is set to {args.refine}. It must be 0 .. 100.")
    if args.extend is None:
        for name in ("weights", "min_score"):
            if getattr(args, name) is not None:
                parser.error(f"--{name.replace('_', '-')} belongs to --extend")
    else:
        if not (args.consensus or args.group_consensus):
            parser.error("--extend needs the motifs of --consensus (with --chains-tsv) or --group-consensus (with --groups-tsv)")
        if args.extend < 0:
            parser.error(f"--extend is set to {args.extend}. It must be at least 0.")
        args.weights = parse_weights(args.weights, parser)
    if not args.groups_tsv:
        if args.max_shift is not None:
            parser.error("--max-shift belongs to --groups-tsv")
        if args.min_group:
            parser.error("--min-group belongs to --groups-tsv")
        if args.keep_covered:
            parser.error("--keep-covered belongs to --groups-tsv")
    if not args.chains_tsv and not args.groups_tsv:
        for name in ("min_seed", "max_gap"):
            if getattr(args, name) is not None:
                parser.error(f"--{name.replace('_', '-')} belongs to --chains-tsv or --groups-tsv")
        return
    if args.groups_tsv:
        if args.chains_tsv:
            parser.error("--groups-tsv and --chains-tsv are two lists: ask for one of them per call")
        if args.min_seed is None or args.max_gap is None or args.max_shift is None:
            parser.error("--groups-tsv needs --min-seed, --max-gap and --max-shift")
        if not 1 <= args.max_shift <= 32:
            parser.error(f"--max-shift is set to {args.max_shift}. It must be 1 .. 32.")
        if args.min_group < 0:
            parser.error(f"--min-group is set to {args.min_group}. It must be at least 0.")
        if args.min_chain:
            parser.error("--min-chain goes with --chains-tsv: a group needs every chain (use --min-group)")
        if args.keep_multiples:
            parser.error("--keep-multiples goes with --chains-tsv (use --keep-covered)")
    elif args.min_seed is None or args.max_gap is None:
        parser.error("--chains-tsv needs --min-seed and --max-gap")
    if args.min_seed < 1:
        parser.error(f"--min-seed is set to {args.min_seed}. It must be at least 1.")
    if not 0 <= args.max_gap <= 4096:
        parser.error(f"--max-gap is set to {args.max_gap}. It must be 0 .. 4096.")
    if args.min_chain < 0:
        parser.error(f"--min-chain is set to {args.min_chain}. It must be at least 0.")
    if not 0.0 <= args.min_identity <= 1.0:
        parser.error(f"--min-identity is set to {args.min_identity}. It must be 0 .. 1.")
    if args.chain_window < 1:
        parser.error(f"--chain-window is set to {args.chain_window}. It must be at least 1.")
    if args.window is not None or args.tsv:
        parser.error("--chains-tsv and --groups-tsv list repeats; --window and --tsv belong to the profile")


def resolve_input(args, parser):
    """(name, sequence text of the whole record or literal, begin, end) after the checks that need no GPU."""
    if args.min_motif_size < 1:
        parser.error(f"--min-motif-size is set to {args.min_motif_size}. It must be at least 1.")
    if args.max_motif_size < args.min_motif_size:
        parser.error(f"--max-motif-size is set to {args.max_motif_size}. It must be at least --min-motif-size.")
    if args.window is not None and (args.window < 64 or args.window % 64):
        parser.error(f"--window is set to {args.window}. It must be a multiple of 64, at least 64.")
    check_chain_args(args, parser)
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
    if args.window is None and not args.chains_tsv and not args.groups_tsv and end - begin > MAX_MATRIX_POSITIONS:
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


def chain_lines(chrom, begin, seq, rows):
    """The --chains-tsv lines of the rows of prf_native.tandem_rows, whose positions are relative to begin."""
    for start, stop, k, copies, identity, matches, seeds in rows.tolist():
        yield (f"{chrom}\t{begin + start}\t{begin + stop}\t{k}\t{copies:.3f}\t{identity:.4f}\t{matches}\t{seeds}\t"
               f"{seq[begin + start:begin + start + k].upper()}\n")


def consensus_batches(ks, max_rows, max_letters):
    """(first, one past last) of the batches of rows that one period_consensus call takes: at most max_rows rows and max_letters
    letters (the sum of k) each.  A single row above max_letters is a batch of its own, for the library to refuse."""
    first, letters = 0, 0
    for at, k in enumerate(ks):
        if at > first and (at - first >= max_rows or letters + k > max_letters):
            yield first, at
            first, letters = at, 0
        letters += k
    if len(ks) > first:
        yield first, len(ks)


def consensus_of(genome, begin, end, rows):
    """(rows of prf_native.consensus_rows, motifs) of the rows of tandem_rows, sent in batches that respect both limits."""
    import numpy as np
    import prf_native
    cons, motifs = [np.zeros(0, dtype=prf_native.CONSENSUS_DTYPE)], []
    for a, b in consensus_batches(rows["k"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS):
        part, text = genome.period_consensus(0, begin, end, rows[a:b])
        cons.append(part)
        motifs += text
    return prf_native.consensus_rows(rows, np.concatenate(cons), motifs), motifs


def consensus_columns(rows, motifs):
    """The four columns --consensus appends to a --chains-tsv line, per row of prf_native.consensus_rows."""
    import prf_native
    for identity, primitive, motif in zip(rows["consensus_identity"].tolist(), rows["primitive"].tolist(), motifs):
        yield f"\t{motif}\t{identity:.4f}\t{primitive}\t{prf_native.canonical_motif(motif)}\n"


def aligned_of(genome, begin, end, rows, motifs):
    """(rows of prf_native.alignment_rows, which of them were aligned) of rows with the fields start, end and k or period against
    one motif each: every row within the limits of one alignment (and with a motif), sent in batches that respect the limits of
    one call; the others stay 0."""
    import numpy as np
    import prf_native
    table = np.zeros(len(rows), dtype=prf_native.REPEAT_DTYPE)
    table["start"], table["end"], table["k"] = rows["start"], rows["end"], [len(m) for m in motifs]
    fits = (table["k"] >= 1) & (table["k"] <= prf_native.ALIGN_MAX_K) & (table["end"] - table["start"] <= prf_native.ALIGN_MAX_LEN)
    sent = np.flatnonzero(fits)
    parts = [np.zeros(0, dtype=prf_native.ALIGNMENT_DTYPE)]
    for a, b in consensus_batches(table["k"][sent].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS):
        parts.append(genome.motif_align(0, begin, end, table[sent[a:b]], [motifs[at] for at in sent[a:b].tolist()]))
    got = np.zeros(len(rows), dtype=prf_native.ALIGNMENT_DTYPE)
    got["consumed"] = table["end"] - table["start"]             # a row that was not sent: no edits, and never shown
    got[sent] = np.concatenate(parts)
    return prf_native.alignment_rows(rows, got), fits


def align_columns(rows, fits):
    """The six columns --align appends to a line, per row of prf_native.alignment_rows."""
    for ok, edits, subs, ins, dele, identity, copies in zip(fits.tolist(), *(rows[f].tolist() for f in (
            "edits", "subs", "ins", "del", "aligned_identity", "aligned_copies"))):
        yield f"\t{edits}\t{subs}\t{ins}\t{dele}\t{identity:.4f}\t{copies:.2f}\n" if ok else "\t.\t.\t.\t.\t.\t.\n"


def with_alignments(args, lines, aligned, fits, detail=None):
    """The lines with the columns of --align (and, from `detail`, of --align-path and --refine), without those
    --min-aligned-identity drops (a row above a limit among them)."""
    lines = [line[:-1] + more for line, more in zip(lines, align_columns(aligned, fits))]
    if detail is not None:
        lines = [line[:-1] + more for line, more in zip(lines, path_columns(args, detail, fits))]
    if args.min_aligned_identity is not None:
        keep = (fits & (aligned["aligned_identity"] >= args.min_aligned_identity)).tolist()
        lines = [line for line, kept in zip(lines, keep) if kept]
    return lines


def extended_of(genome, begin, end, rows, motifs, flank, weights):
    """(rows of prf_native.local_rows, which of them were sent) of rows with the fields start and end against one motif each: the
    window of every row within the limits of one alignment (and with a motif) is the row padded by `flank`
    (prf_native.flank_repeats), sent in batches that respect the limits of one call; the others keep their interval and score 0."""
    import numpy as np
    import prf_native
    table = np.zeros(len(rows), dtype=prf_native.REPEAT_DTYPE)
    table["start"], table["end"], table["k"] = rows["start"], rows["end"], [len(m) for m in motifs]
    windows, fits = prf_native.flank_repeats(table, flank, end - begin)
    sent = np.flatnonzero(fits)
    local = np.zeros(len(rows), dtype=prf_native.LOCAL_ALIGNMENT_DTYPE)
    for a, b in consensus_batches(table["k"][sent].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS):
        local[sent[a:b]] = genome.motif_align_local(0, begin, end, windows[sent[a:b]], [motifs[at] for at in sent[a:b].tolist()], *weights)
    return prf_native.local_rows(table, windows, local), fits


def with_extensions(args, begin, lines, extended, fits):
    """The lines with the three columns of --extend, in the file's coordinates, without those --min-score drops (a row above a
    limit among them)."""
    more = [f"\t{begin + first}\t{begin + last}\t{score}\n" if ok else "\t.\t.\t.\n"
            for ok, first, last, score in zip(fits.tolist(), *(extended[f].tolist() for f in ("local_start", "local_end", "score")))]
    lines = [line[:-1] + tail for line, tail in zip(lines, more)]
    if args.min_score is not None:
        keep = (fits & (extended["score"] >= args.min_score)).tolist()
        lines = [line for line, kept in zip(lines, keep) if kept]
    return lines


def aligned_kept(args, aligned, fits):
    """Which rows with_alignments keeps."""
    import numpy as np
    if args.min_aligned_identity is None:
        return np.ones(len(fits), dtype=bool)
    return fits & (aligned["aligned_identity"] >= args.min_aligned_identity)


def wants_paths(args):
    return bool(args.align_path or args.refine or args.copies_tsv)


def aligned_paths_of(genome, begin, end, rows, motifs, rounds):
    """aligned_of with the paths (--align-path, --refine, --copies-tsv): (rows of prf_native.alignment_rows, which of them were
    aligned, detail) with detail = the motifs of the last round, per row the rounds of --refine that changed its motif, and the
    row's path (None: not aligned).  Batches respect the limits of one call, the positions of one call's path among them."""
    import numpy as np
    import prf_native
    table = np.zeros(len(rows), dtype=prf_native.REPEAT_DTYPE)
    table["start"], table["end"], table["k"] = rows["start"], rows["end"], [len(m) for m in motifs]
    fits = (table["k"] >= 1) & (table["k"] <= prf_native.ALIGN_MAX_K) & (table["end"] - table["start"] <= prf_native.ALIGN_MAX_LEN)
    sent = np.flatnonzero(fits)
    got = np.zeros(len(rows), dtype=prf_native.ALIGNMENT_DTYPE)
    got["consumed"] = table["end"] - table["start"]             # a row that was not sent: no edits, and never shown
    detail = {"motifs": list(motifs), "refined": np.zeros(len(rows), dtype=np.uint32), "paths": [None] * len(rows),
              "k": table["k"].tolist(), "start": table["start"].tolist()}
    lengths = (table["end"] - table["start"])[sent].tolist()
    for a, b in piece_batches(table["k"][sent].tolist(), lengths, prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS,
                              prf_native.ALIGNPATH_MAX_POSITIONS):
        which = sent[a:b]
        part, names = table[which], [motifs[at] for at in which.tolist()]
        if rounds:
            names, _, changed = prf_native.refine_motifs(genome, 0, begin, end, part, names, rounds)
            detail["refined"][which] = changed
        got[which], paths = genome.motif_align_path(0, begin, end, part, names)
        for at, name, path in zip(which.tolist(), names, paths):
            detail["motifs"][at], detail["paths"][at] = name, path
    return prf_native.alignment_rows(rows, got), fits, detail


def take_detail(detail, keep):
    """The detail of the rows whose `keep` is set."""
    import numpy as np
    keep = np.asarray(keep, dtype=bool)
    return {name: (value[keep] if isinstance(value, np.ndarray) else [v for v, kept in zip(value, keep.tolist()) if kept])
            for name, value in detail.items()}


def path_columns(args, detail, fits):
    """The columns --align-path (cigar) and --refine (refined) append to a line; '.' for a row above a limit."""
    import prf_native
    for ok, path, k, refined in zip(fits.tolist(), detail["paths"], detail["k"], detail["refined"].tolist()):
        more = ""
        if args.align_path:
            more += "\t" + (prf_native.path_cigar(path, k) if ok else ".")
        if args.refine:
            more += f"\t{refined}" if ok else "\t."
        yield more + "\n"


def write_copies(args, chrom, begin, aligned, fits, detail):
    """--copies-tsv: one line per aligned copy of the rows that are listed."""
    import prf_native
    keep = fits if args.min_aligned_identity is None else fits & (aligned["aligned_identity"] >= args.min_aligned_identity)
    n_lines = 0
    with open(args.copies_tsv, "wt") as out:
        for ok, path, k, start, end in zip(keep.tolist(), detail["paths"], detail["k"], detail["start"], aligned["end"].tolist()):
            if not ok:
                continue
            for copy, first, last, subs, ins, dels in prf_native.path_copies(path, start, k).tolist():
                out.write(f"{chrom}\t{begin + start}\t{begin + end}\t{k}\t{copy}\t{begin + first}\t{begin + last}\t{subs}\t{ins}\t{dels}\n")
                n_lines += 1
    print(f"Wrote {args.copies_tsv}: {n_lines} copies")


def list_chains(args, chrom, seq, begin, end, context=None):
    """--chains-tsv: the interval in windows of --chain-window start positions, the lists concatenated; with --consensus the
    consensus of every repeat that is left, from the same resident genome."""
    import numpy as np
    import prf_native
    ctx = context if context is not None else prf_native.default_context()
    genome = ctx.load([seq.encode("ascii", "replace")], 64)
    try:
        parts = [genome.period_chains(0, begin, end, args.min_motif_size, args.max_motif_size, args.min_seed, args.max_gap,
                                      args.min_chain, args.n_matches, (at, min(at + args.chain_window, end - begin)))
                 for at in range(0, end - begin, args.chain_window)]
        chains = np.concatenate(parts) if parts else np.zeros(0, dtype=prf_native.PCHAIN_DTYPE)
        rows = prf_native.tandem_rows(chains, drop_multiples=not args.keep_multiples)
        rows = rows[rows["identity"] >= args.min_identity]
        if args.consensus:
            named, motifs = consensus_of(genome, begin, end, rows)
            detail = None
            if args.align and wants_paths(args):
                aligned, fits, detail = aligned_paths_of(genome, begin, end, rows, motifs, args.refine)
                motifs = detail["motifs"]                           # of the last round of --refine
            elif args.align:
                aligned, fits = aligned_of(genome, begin, end, rows, motifs)
            if args.extend is not None:
                extended, extends = extended_of(genome, begin, end, rows, motifs, args.extend, args.weights)
    finally:
        genome.free()
    lines = list(chain_lines(chrom, begin, seq, rows))
    if args.consensus:
        lines = [line[:-1] + more for line, more in zip(lines, consensus_columns(named, motifs))]
        if args.min_consensus_identity is not None:
            keep = (named["consensus_identity"] >= args.min_consensus_identity).tolist()
            lines = [line for line, kept in zip(lines, keep) if kept]
            if args.align:
                aligned, fits = aligned[np.array(keep, dtype=bool)], fits[np.array(keep, dtype=bool)]
                detail = take_detail(detail, keep) if detail is not None else None
            if args.extend is not None:
                extended, extends = extended[np.array(keep, dtype=bool)], extends[np.array(keep, dtype=bool)]
        if args.align:
            lines = with_alignments(args, lines, aligned, fits, detail)
            if args.copies_tsv:
                write_copies(args, chrom, begin, aligned, fits, detail)
            if args.extend is not None:
                extended, extends = extended[aligned_kept(args, aligned, fits)], extends[aligned_kept(args, aligned, fits)]
        if args.extend is not None:
            lines = with_extensions(args, begin, lines, extended, extends)
    with open(args.chains_tsv, "wt") as out:
        out.writelines(lines)
    print(f"Wrote {args.chains_tsv}: {len(lines)} repeats")


def group_lines(chrom, begin, seq, rows):
    """The --groups-tsv lines of the rows of prf_native.tandem_groups, whose positions are relative to begin."""
    for start, stop, period, copies, identity, indel, chains, seeds in rows.tolist():
        yield (f"{chrom}\t{begin + start}\t{begin + stop}\t{period}\t{copies:.3f}\t{identity:.4f}\t{indel}\t{chains}\t{seeds}\t"
               f"{seq[begin + start:begin + start + period].upper()}\n")


def piece_batches(ks, segments, max_rows, max_letters, max_segments):
    """(first, one past last) of the batches of pieces that one phased_consensus call takes: at most max_rows rows, max_letters
    letters (the sum of k) and max_segments segments each; segments[i] is the number of segments of piece i.  A single piece
    above a limit is a batch of its own, for the library to refuse."""
    first, letters, n_segments = 0, 0, 0
    for at, (k, n) in enumerate(zip(ks, segments)):
        if at > first and (at - first >= max_rows or letters + k > max_letters or n_segments + n > max_segments):
            yield first, at
            first, letters, n_segments = at, 0, 0
        letters, n_segments = letters + k, n_segments + n
    if len(ks) > first:
        yield first, len(ks)


def group_consensus_of(genome, begin, end, joined, keep, chains, links):
    """(rows of prf_native.group_consensus_rows, motifs) of all groups of joined = join_period_chains(chains, links,
    with_paths=True); only the pieces of the groups whose `keep` is set are counted, in batches that respect the limits of one call, the others stay empty."""
    import numpy as np
    import prf_native
    groups = joined[0]
    pieces, segments = prf_native.group_segments(chains, links, joined)
    wanted = keep[pieces["group"].astype(np.int64)] if len(pieces) else np.zeros(0, dtype=bool)
    new_row = np.cumsum(wanted) - 1                                              # of a wanted piece among the wanted ones
    pieces = pieces[wanted]
    segments = segments[wanted[segments["row"].astype(np.int64)]] if len(segments) else segments
    segments["row"] = new_row[segments["row"].astype(np.int64)] if len(segments) else segments["row"]
    cons, motifs = [np.zeros(0, dtype=prf_native.CONSENSUS_DTYPE)], []
    seg0 = np.concatenate([[0], np.cumsum(pieces["segments"].astype(np.int64))])    # a piece's segments are consecutive
    for a, b in piece_batches(pieces["k"].tolist(), pieces["segments"].tolist(), prf_native.CONSENSUS_MAX_ROWS,
                              prf_native.CONSENSUS_MAX_LETTERS, prf_native.PHASED_MAX_SEGMENTS):
        part = segments[seg0[a]:seg0[b]].copy()
        part["row"] -= a
        rows, text = genome.phased_consensus(0, begin, end, pieces["k"][a:b], part)
        cons.append(rows)
        motifs += text
    return prf_native.group_consensus_rows(groups, pieces, np.concatenate(cons), motifs)


def group_consensus_columns(rows, motifs):
    """The six columns --group-consensus appends to a --groups-tsv line, per row of prf_native.group_consensus_rows."""
    import prf_native
    for identity, primitive, pieces, covered, motif in zip(rows["consensus_identity"].tolist(), rows["primitive"].tolist(),
                                                           rows["pieces"].tolist(), rows["covered"].tolist(), motifs):
        yield f"\t{motif}\t{identity:.4f}\t{primitive}\t{prf_native.canonical_motif(motif)}\t{pieces}\t{covered:.4f}\n"


def list_groups(args, chrom, seq, begin, end, context=None):
    """--groups-tsv: the interval in windows of --chain-window start positions; per window the chains (min_len 0) and the links,
    which add up over the windows; then the join, the filters and one line per group; with --group-consensus the consensus of
    every repeat that is left, from the same resident genome."""
    import numpy as np
    import prf_native
    ctx = context if context is not None else prf_native.default_context()
    genome = ctx.load([seq.encode("ascii", "replace")], 64)
    chains, links = [], []
    try:
        for at in range(0, end - begin, args.chain_window):
            window = (at, min(at + args.chain_window, end - begin))
            chains.append(genome.period_chains(0, begin, end, args.min_motif_size, args.max_motif_size, args.min_seed, args.max_gap, 0,
                                               args.n_matches, window))
            links.append(genome.period_links(0, begin, end, args.min_motif_size, args.max_motif_size, args.min_seed, args.max_gap,
                                             args.max_shift, args.n_matches, window))
        chains = np.concatenate(chains) if chains else np.zeros(0, dtype=prf_native.PCHAIN_DTYPE)
        links = np.concatenate(links) if links else np.zeros(0, dtype=prf_native.PLINK_DTYPE)
        joined = prf_native.join_period_chains(chains, links, with_paths=True)
        groups = joined[0]
        rows, kept = prf_native.tandem_groups(groups, drop_covered=not args.keep_covered, with_index=True)
        passed = (rows["end"] - rows["start"] >= args.min_group) & (rows["identity"] >= args.min_identity)
        rows, kept = rows[passed], kept[passed]
        if args.group_consensus:
            keep = np.zeros(len(groups), dtype=bool)
            keep[kept] = True
            named, motifs = group_consensus_of(genome, begin, end, joined, keep, chains, links)
            named, motifs = named[kept], [motifs[at] for at in kept.tolist()]
            detail = None
            if args.align and wants_paths(args):                # the whole [start, end) of a group against the motif of its chosen piece
                aligned, fits, detail = aligned_paths_of(genome, begin, end, rows, motifs, args.refine)
                motifs = detail["motifs"]                           # of the last round of --refine
            elif args.align:
                aligned, fits = aligned_of(genome, begin, end, rows, motifs)
            if args.extend is not None:                         # the group's [start, end) plus the flank against the motif of its chosen piece
                extended, extends = extended_of(genome, begin, end, rows, motifs, args.extend, args.weights)
    finally:
        genome.free()
    lines = list(group_lines(chrom, begin, seq, rows))
    if args.group_consensus:
        lines = [line[:-1] + more for line, more in zip(lines, group_consensus_columns(named, motifs))]
        if args.min_group_consensus_identity is not None:
            passed = (named["consensus_identity"] >= args.min_group_consensus_identity).tolist()
            lines = [line for line, ok in zip(lines, passed) if ok]
            if args.align:
                aligned, fits = aligned[np.array(passed, dtype=bool)], fits[np.array(passed, dtype=bool)]
                detail = take_detail(detail, passed) if detail is not None else None
            if args.extend is not None:
                extended, extends = extended[np.array(passed, dtype=bool)], extends[np.array(passed, dtype=bool)]
        if args.align:
            lines = with_alignments(args, lines, aligned, fits, detail)
            if args.copies_tsv:
                write_copies(args, chrom, begin, aligned, fits, detail)
            if args.extend is not None:
                extended, extends = extended[aligned_kept(args, aligned, fits)], extends[aligned_kept(args, aligned, fits)]
        if args.extend is not None:
            lines = with_extensions(args, begin, lines, extended, extends)
    with open(args.groups_tsv, "wt") as out:
        out.writelines(lines)
    print(f"Wrote {args.groups_tsv}: {len(lines)} repeats")


def main(argv=None, context=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    chrom, seq, begin, end = resolve_input(args, parser)
    if args.chains_tsv:
        return list_chains(args, chrom, seq, begin, end, context)
    if args.groups_tsv:
        return list_groups(args, chrom, seq, begin, end, context)
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
