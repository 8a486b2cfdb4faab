"""The reference's plotting helpers (reference utils/plot_utils.py), with the periodicity matrix computed on the GPU.

shift_string_by is the string helper the reference's tests import (:6-9).  get_period_matrix (:12-25) takes its set cells from
libprf (prf_period_bits: cell (k, i) = seq[i] == seq[i + k], N == N included) and colours them on the host; the two plot
functions (:29-77) are written from the reference's behaviour and import matplotlib only when they are called.  The dot plot
(reference plot_dot_plot.py) stays out of scope."""
import hashlib
import zlib


def shift_string_by(string, shift):
    """Rotate `string` to the right by `shift` characters ("AGTTT", 2 -> "TTAGT")."""
    n = len(string)
    if n == 0:
        return string
    cut = (n - shift % n) % n
    return string[cut:] + string[:cut]


def motif_value(motif):
    """A nonzero number that depends on the motif text alone.  The reference takes abs(hash(...)) of Python's salted 64-bit hash
    (:22), which differs from run to run.  Its commented-out line (:74) suggests adler32, but adler32 gives different short
    texts over four letters the same value (two sums of bytes), and which cells share a value is what the matrix shows: a 64-bit
    digest instead."""
    return int.from_bytes(hashlib.blake2b(motif.encode("utf-8"), digest_size=8).digest(), "little") + 1


def period_classes(seq, bits, min_motif_size=1):
    """The values of the set cells of a periodicity matrix.  bits: uint64[nk, ceil(len(seq) / 64)] as Genome.period_bits
    returns it for k = min_motif_size .. min_motif_size + nk - 1 (bit j of word w of row r: cell (min_motif_size + r, 64 w + j)).
    Returns nk rows of len(seq) ints: 0 where the cell is not set, else motif_value of the text the reference hashes (:22):
    seq[i:i+k] rotated right by i % k, which stays the same along a run of one motif."""
    import numpy as np
    n = len(seq)
    bits = np.ascontiguousarray(bits, dtype="<u8")
    rows = []
    for r in range(bits.shape[0]):
        k = min_motif_size + r
        cells = np.unpackbits(bits[r].view(np.uint8), bitorder="little")[:n]
        row = [0] * n
        seen = {}
        for i in np.flatnonzero(cells).tolist():
            text = shift_string_by(seq[i:i + k], i % k)
            value = seen.get(text)
            if value is None:
                value = seen[text] = motif_value(text)
            row[i] = value
        rows.append(row)
    return rows


def get_period_matrix(min_motif_size, max_motif_size, input_sequence, context=None):
    """The reference's periodicity matrix (:12-25): max_motif_size rows (after its clamps) of len(input_sequence) ints, row
    k - 1 for period k; cell (k, i) is nonzero iff seq[i] == seq[i + k], and two cells of a row share a value iff the reference
    gives them the same hash.  The sequence is upper-cased, as everywhere in this package.  The set cells come from the GPU
    (Context.period_bits); context: a prf_native.Context, default the process-wide one."""
    import prf_native
    seq = input_sequence.upper()
    min_motif_size = max(min_motif_size, 1)
    max_motif_size = min(max_motif_size, len(seq) // 2)
    matrix = [[0] * len(seq) for _ in range(min(min_motif_size - 1, max_motif_size))]
    if max_motif_size >= min_motif_size:
        ctx = context or prf_native.default_context()
        bits = ctx.period_bits(seq, min_motif_size, max_motif_size)
        matrix += period_classes(seq, bits, min_motif_size)
    return matrix


def _pyplot():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def plot_periodicity_matrix(periodicity_matrix, output_path, fractions=None, extent=None, value_label=None):
    """Two panels as in the reference (:29-53): the matrix above (one colour per value, pale grey for 0), the fraction of
    matches per period below, with its denominator width - period + 1.
    For a windowed profile (plot_periodicity_matrix.py --window) the caller passes a matrix of floats (counts / window), the
    fractions over the whole range, and extent = (first position, last position) for the x axis; the upper panel is then a
    continuous colour scale labelled value_label."""
    plt = _pyplot()
    from matplotlib.colors import ListedColormap
    matrix_width = len(periodicity_matrix[0]) if periodicity_matrix else 0
    fig, (ax1, ax2) = plt.subplots(nrows=2, figsize=(10, 8))
    if periodicity_matrix and matrix_width:
        if fractions is None:
            cmap = ListedColormap(["#F3F3F3"] + list(plt.get_cmap("Pastel2", 12).colors))
            # the reference hands matshow the raw hashes; small class numbers give the same picture with stable colours
            shown = [[0 if v == 0 else 1 + v % 12 for v in row] for row in periodicity_matrix]
            ax1.matshow(shown, aspect="auto", cmap=cmap, vmin=0, vmax=12)
        else:
            box = None if extent is None else (extent[0], extent[1], len(periodicity_matrix) + 0.5, 0.5)
            image = ax1.matshow(periodicity_matrix, aspect="auto", cmap="viridis", vmin=0, vmax=1, extent=box)
            fig.colorbar(image, ax=ax1, label=value_label or "Fraction of matches per window")
    ax1.set_xlabel("Input sequence position")
    ax1.set_ylabel("Period")

    if fractions is None:
        scores = [sum(1 for v in row if v > 0) for row in periodicity_matrix]
        fractions = [score / (matrix_width - (i + 1) + 1) for i, score in enumerate(scores)]
    periods = list(range(1, len(fractions) + 1))
    ax2.bar(periods, fractions)
    if len(periods) <= 60:
        ax2.set_xticks(periods)
    ax2.set_ylabel("Fraction of matches")
    ax2.set_xlabel("Period")

    plt.savefig(output_path)
    plt.close(fig)
    print(f"Wrote {output_path}")


def plot_results(input_sequence, output_intervals, max_motif_size, output_path):
    """Plot the repeats detected in input_sequence (reference :56-77): row len(motif) - 1 is painted from start_0based to end
    inclusive (the reference's range(start, end + 1); clipped to the sequence, where the reference raises IndexError for a repeat
    that reaches the last position) with a colour chosen by the motif text -- zlib.adler32(motif) % 10 + 1, the deterministic
    form of the reference's hash(motif) % 10 + 1."""
    plt = _pyplot()
    plt.rcParams["figure.figsize"] = [16.5, 5]
    plt.rcParams["font.size"] = 12
    n = len(input_sequence)
    matrix = [[0] * n for _ in range(max_motif_size)]
    for start_0based, end, motif in output_intervals:
        row = len(motif) - 1
        if not 0 <= row < max_motif_size:
            continue
        value = zlib.adler32(motif.encode("utf-8")) % 10 + 1
        for i in range(start_0based, min(end + 1, n)):
            matrix[row][i] = value
    plot_periodicity_matrix(matrix, output_path)
