"""CPU: the exact dot plot of two ranges on either strand (prf_dotpair_bits / prf_dotpair_counts, plot_dot_plot.py
--versus / --strand).  The numpy model (tests/dotpair_model.py) equals the reference's filter on every case of
tests/golden/dotpair.jsonl.gz and keeps the identities of DESIGN 12.4; the refusals of the new entry points are decided before the
context is looked at (NULL context, no GPU needed), in the documented order.  The command line's checks and the plot function run
on the host as well."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import dotpair_model as P
import dotplot_model as D
from conftest import ROOT, load_jsonl_gz


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("dotpair.jsonl.gz")


def test_the_fixture_is_what_the_tool_promises(golden):
    assert 130 <= len(golden) <= 170
    sizes = {(len(c["a"]), len(c["b"])) for c in golden}
    for side in (0, 1):
        assert {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193} <= {s[side] for s in sizes}
    assert max(max(s) for s in sizes) <= 200
    assert any(na < nb for na, nb in sizes) and any(na > nb for na, nb in sizes)
    assert any(na == 0 and nb > 0 for na, nb in sizes) and any(nb == 0 and na > 0 for na, nb in sizes)
    assert {c["t"] for c in golden} == {0, 1, 2, 3, 4, 5, 8, 16, 63, 64} and {c["strand"] for c in golden} == {"+", "-"}
    letters = set("".join(c["a"] + c["b"] for c in golden))
    assert set("ACGTNRYKMSWBVDH") <= letters
    assert all(c["a"] == c["a"].upper() and c["b"] == c["b"].upper() and len(c["kept"]) == len(c["a"]) for c in golden)
    for kind in ("shared", "revcomp", "reversed", "complemented"):
        assert sum(c["tag"].startswith(kind + "-") and P.fixture_cells(c).any() for c in golden) >= 4, kind
    # N == N is a match on both strands
    c = next(c for c in golden if c["tag"].startswith("all-n") and len(c["a"]) >= 64 and len(c["b"]) >= 65)
    assert P.fixture_cells(c).all()
    # a reverse-complemented piece is an anti-diagonal of the minus matrix: some kept cell has no main-diagonal neighbour
    c = next(c for c in golden if c["tag"].startswith("revcomp-") and not c["tag"].startswith("revcomp-other") and c["t"] >= 3
             and P.fixture_cells(c).any())
    cells, raw = P.fixture_cells(c), P.kept_cells(c["a"], c["b"], "-", 0)
    assert (cells[1:-1, 1:-1] & ~raw[:-2, :-2] & ~raw[2:, 2:]).any()


def test_model_equals_the_reference(golden):
    bad = [c["tag"] for c in golden if not np.array_equal(P.kept_cells(c["a"], c["b"], c["strand"], c["t"]), P.fixture_cells(c))]
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_model_windows_equal_the_whole_rectangle(golden):
    rng = random.Random(5)
    for c in golden[::5]:
        na, nb = len(c["a"]), len(c["b"])
        whole = P.fixture_cells(c)
        r0, c0 = rng.randrange(0, na + 1), rng.randrange(0, nb + 1)
        r1, c1 = rng.randrange(r0, na + 40), rng.randrange(c0, nb + 40)
        got = P.kept_cells(c["a"], c["b"], c["strand"], c["t"], rows=(r0, r1), cols=(c0, c1))
        assert np.array_equal(got, whole[r0:r1, c0:c1]), c["tag"]
    a, b = "ACGTTGCAAC" * 30, "GTTGCAACGT" * 20 + "ACGTNNRYAC" * 9
    for strand in "+-":
        inner = P.kept_cells(a, b, strand, 4, (17, 250), (3, 280))
        assert np.array_equal(inner, P.kept_cells(a[17:250], b[3:280], strand, 4))
        assert np.array_equal(P.kept_cells(a, b, strand, 4, (17, 9_999), (3, None)), P.kept_cells(a[17:], b[3:], strand, 4))
    assert P.kept_bits(a, b, "-", 3, rows=(5, 6), cols=(64, 200)).shape == (1, 3)
    # the same range twice on the plus strand is the self plot's model
    assert np.array_equal(P.kept_cells(a, a, "+", 5, (7, 200), (7, 200), (3, 150), (0, 190)), D.kept_cells(a, 5, 7, 200, (3, 150), (0, 190)))


def test_the_model_keeps_the_identities(golden):
    """the transpose swaps the ranges; the minus strand is the plus strand of the reverse complement with the
    columns mirrored, filter included."""
    for c in golden[::3]:
        a, b, t = c["a"].encode(), c["b"].encode(), c["t"]
        for strand in "+-":
            ab = P.kept_cells(a, b, strand, t)
            assert np.array_equal(ab.T, P.kept_cells(b, a, strand, t)), (c["tag"], strand)
        assert np.array_equal(P.kept_cells(a, b, "-", t), P.kept_cells(a, P.revcomp(b), "+", t)[:, ::-1]), c["tag"]
    assert P.comp(b"ACGTRYKMBVDHNSWacgtX") == b"TGCAYRMKVBHDNSWacgtX"      # an involution on upper case; anything else stays
    assert P.comp(P.comp(bytes(range(65, 91)))) == bytes(range(65, 91))


# ---- the C ABI: refusals are decided before the context is looked at (NULL context) ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _call(lib, pn, form, seq_a=b"ACGTACGTAC", seq_b=b"ACGTACGTACGT", a=(0, 10), b=(0, 12), strand=0, rows=(0, 10), cols=(0, 12), t=3,
          block=None, capacity=4096, dst=True, sizes=True):
    buf = (ctypes.c_uint64 * 4096)()
    n0, n1, stats = ctypes.c_uint64(0), ctypes.c_uint64(0), pn.ScanStats()
    p0, p1 = (ctypes.byref(n0), ctypes.byref(n1)) if sizes else (None, None)
    window = (strand, rows[0], rows[1], cols[0], cols[1], t)
    out = buf if dst else None
    tail = (out, capacity, p0, ctypes.byref(stats)) if block is None else (block, out, capacity, p0, p1, ctypes.byref(stats))
    kind = "bits" if block is None else "counts"
    if form == "one_shot":
        arr_a, _keep_a = pn._contig_array([seq_a])
        arr_b, _keep_b = pn._contig_array([seq_b])
        return getattr(lib, f"prf_dotpair_{kind}_seq")(None, arr_a, *a, arr_b, *b, *window, *tail)
    if form == "ex":
        return getattr(lib, f"prf_dotpair_{kind}_ex")(None, None, 0, *a, 1, *b, *window, *tail, 4096)
    return getattr(lib, f"prf_dotpair_{kind}")(None, None, 0, *a, 1, *b, *window, *tail)


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_dotpair.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.DOTPAIR_EXPORTS) and len(declared) == 6
    assert not set(declared) & (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS))
    assert '#include "prf_dotpair.h"' in open(os.path.join(ROOT, "include", "prf.h")).read()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4


# each case breaks one rule and every rule behind it: the first in the documented order is the one reported
LATER = dict(rows=(5, 4), cols=(9, 2), strand=2, t=65, dst=False, sizes=False)
ORDER = [
    (dict(block=100, a=(7, 3), b=(8, 2), **LATER), "PRF_EINVAL", "block"),
    (dict(a=(7, 3), b=(8, 2), **LATER), "PRF_EINVAL", "a_begin 7"),
    (dict(b=(8, 2), **LATER), "PRF_EINVAL", "b_begin 8"),
    (dict(LATER), "PRF_EINVAL", "row0"),
    (dict(LATER, rows=(0, 10)), "PRF_EINVAL", "col0"),
    (dict(strand=2, t=65, dst=False, sizes=False), "PRF_EINVAL", "strand is 2"),
    (dict(t=65, dst=False, sizes=False), "PRF_EUNSUPPORTED", "min_diagonal_run 65"),
    (dict(dst=False, sizes=False), "PRF_EINVAL", "NULL destination"),
    (dict(sizes=False), "PRF_EINVAL", "NULL size pointer"),
    (dict(sizes=False, block=64), "PRF_EINVAL", "NULL size pointer"),
    (dict(block=0), "PRF_EINVAL", "block"),
    (dict(block=32), "PRF_EINVAL", "block"),
    (dict(block=32832), "PRF_EINVAL", "block"),
    (dict(strand=0xFFFFFFFF), "PRF_EINVAL", "strand"),
    (dict(), "PRF_EINVAL", "NULL context"),                             # valid arguments
    (dict(strand=1, t=64, block=32768), "PRF_EINVAL", "NULL context"),
    (dict(t=0, rows=(3, 3), a=(4, 4)), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_dotpair_")


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(capacity=9), "PRF_EINVAL", "destination holds 9 words"),                              # 10 rows x 1 word
    (dict(seq_a=b"A" * 200, seq_b=b"T" * 70, a=(0, 200), b=(0, 70), rows=(0, 200), cols=(0, 200), capacity=399), "PRF_EINVAL",
     "the output has 400 (200 x 2)"),                                                           # columns clipped to nb
    (dict(seq_a=b"A" * 70, seq_b=b"T" * 200, a=(0, 200), b=(0, 200), rows=(0, 200), cols=(0, 200), block=64, capacity=7), "PRF_EINVAL",
     "the output has 8 (2 x 4)"),                                                               # rows clipped to na
    (dict(seq_a=b"A" * 70, seq_b=b"T" * 200, a=(0, 200), b=(100, 200), rows=(0, 200), cols=(0, 200), block=64, capacity=4), "PRF_EINVAL",
     "NULL context"),                                                                           # 2 x 2
    (dict(a=(0, 1 << 40), b=(2, 1 << 63), rows=(0, 1 << 60), cols=(2, 1 << 63), capacity=10), "PRF_EINVAL", "NULL context"),
    (dict(rows=(20, 30), capacity=0), "PRF_EINVAL", "NULL context"),                            # an empty window needs no room
    (dict(seq_b=b"", b=(0, 0), capacity=0), "PRF_EINVAL", "NULL context"),                      # an empty side: no columns
    (dict(seq_a=b"ACGT-ACGTA"), "PRF_ESYMBOL", "position 4"),
    (dict(seq_b=b"ACGTAC1TACGT", block=64), "PRF_ESYMBOL", "position 6"),
    (dict(seq_a=b"ACGT-ACGTA", capacity=9), "PRF_EINVAL", "destination holds 9 words"),         # the room before the bytes
])
def test_refusals_that_need_the_sequences(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


def test_a_missing_sequence_is_refused():
    pn, lib = _lib()
    arr, _keep = pn._contig_array([b"ACGT"])
    buf, n0, stats = (ctypes.c_uint64 * 16)(), ctypes.c_uint64(0), pn.ScanStats()
    for first, second in ((None, arr), (arr, None)):
        rc = lib.prf_dotpair_bits_seq(None, first, 0, 4, second, 0, 4, 0, 0, 4, 0, 4, 3, buf, 16, ctypes.byref(n0), ctypes.byref(stats))
        assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()


def test_outputs_and_windows_above_the_documented_limits_are_refused():
    """2^28 entries per call (PRF_PERIOD_BITS_MAX_WORDS), 2^42 cells per call (PRF_DOT_MAX_CELLS).  The sequences are never read:
    the sizes are judged first."""
    pn, lib = _lib()
    n = 1 << 22
    arr = (pn._Contig * 1)()
    block = ctypes.create_string_buffer(16)
    arr[0].ascii, arr[0].len = ctypes.addressof(block), n
    n0, n1, stats, dst = ctypes.c_uint64(0), ctypes.c_uint64(0), pn.ScanStats(), (ctypes.c_uint64 * 1)()
    rc = lib.prf_dotpair_bits_seq(None, arr, 0, n, arr, 0, n, 1, 0, n, 0, n, 3, dst, 1 << 60, ctypes.byref(n0), ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_PERIOD_BITS_MAX_WORDS" in lib.prf_last_error().decode()     # 2^22 x 2^16 words
    rc = lib.prf_dotpair_counts_seq(None, arr, 0, n, arr, 0, n, 1, 0, n, 0, n, 3, 32768, dst, 1 << 60, ctypes.byref(n0), ctypes.byref(n1),
                                    ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()               # 2^44 cells, 2^14 counts


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g, other = pn.Genome(None, None, 2, [100, 50]), pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="block"):
        g.dotpair_counts((0, 0, None), (1, 0, None), 100)
    with pytest.raises(ValueError, match="contig 2"):
        g.dotpair_bits((0, 0, None), (2, 0, None))
    with pytest.raises(ValueError, match="strand"):
        g.dotpair_bits((0, 0, None), (1, 0, None), strand="x")
    with pytest.raises(ValueError, match="cols"):
        g.dotpair_bits((0, 0, None), (1, 0, None), cols=(5, 4))
    with pytest.raises(ValueError, match="begin"):
        g.dotpair_bits((0, 0, None), (1, 7, 3))
    with pytest.raises(ValueError, match="both be sequences or both"):
        pn._matrix(None, (g, 0), 0, None, False, dot=(3, None, None, None, 0), versus=("ACGT", 0, None, "+"))
    with pytest.raises(ValueError, match="both be sequences or both"):
        pn._matrix(None, "ACGT", 0, None, False, dot=(3, None, None, None, 0), versus=((g, 0), 0, None, "+"))
    with pytest.raises(ValueError, match="same resident genome"):
        pn._matrix(None, (g, 0), 0, None, False, dot=(3, None, None, None, 0), versus=((other, 0), 0, None, "+"))
    g._h = other._h = None


# ---- command line and plots ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_inputs(args, parser), cli.resolve_versus(args, parser), args


def test_cli_parses_versus_and_strand(tmp_path, capsys):
    import plot_dot_plot as cli
    out, versus, args = _parse(cli, ["ACGTACGT", "-o", "x.png", "-d", str(tmp_path)])
    assert versus is None and args.strand == "+" and out == [("sequence", 0, "ACGTACGT", str(tmp_path / "x.png"))]
    for argv, strand in ((["--strand", "-"], "-"), (["--strand=-"], "-"), (["--strand", "both"], "both"), (["--strand", "+"], "+")):
        assert _parse(cli, ["ACGT"] + argv)[2].strand == strand
    out, versus, _ = _parse(cli, ["ACGTACGT", "--versus", "TTGACA"])
    assert versus == ("sequence", 0, "TTGACA") and out[0][2] == "ACGTACGT"
    fa = tmp_path / "g.fa"
    chrom = "ACGTTGCAGT" * 60
    fa.write_text(">chr7 some text\n" + "\n".join(chrom[i:i + 50] for i in range(0, 600, 50)) + "\n>chrB\nacgtnry\n")
    out, versus, _ = _parse(cli, ["-R", str(fa), "chr7:10-30", "--versus", "B:1-6", "-p", "1"])
    assert out[0][:3] == ("chr7", 9, chrom[9:31]) and versus == ("chrB", 0, "ACGTNRY")
    capsys.readouterr()
    long_fa = tmp_path / "x.fa"
    long_fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    assert len(_parse(cli, ["ACGT", "-R", str(long_fa), "--versus", "chrA:0-7000", "--block", "64"])[1][2]) == 7000
    for argv, text in ((["ACGT", "--versus", "chr7:1-5"], "--reference-fasta is required"), (["ACGT", "--versus", "ACGU"], "not a valid"),
                       (["ACGT", "-R", str(fa), "--versus", "chrZ:1-5"], "not found"), (["ACGT", "--strand", "x"], "invalid choice"),
                       (["ACGT", "-R", str(fa), "--versus", "chr7:5-x"], "Unable to parse interval"),
                       (["ACGT", "-R", str(long_fa), "--versus", "chrA:0-7000"], "--block"),
                       (["ACGT", "--versus", "ACGT" * 1251], "--block"),
                       (["ACGT", "--strand", "both", "--block", "64"], "one strand at a time")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err


def test_density_lines_of_a_rectangle():
    import plot_dot_plot as cli
    counts = np.array([[3, 0, 1], [0, 5, 0]], dtype=np.uint32)
    assert list(cli.density_lines("chr1", 100, 100, 64, counts, 7, 150)) == [
        "chr1\t100\t164\t7\t71\t3\n", "chr1\t100\t164\t135\t157\t1\n", "chr1\t164\t200\t71\t135\t5\n"]


def test_plot_writes_a_rectangular_png(tmp_path):
    import plot_dot_plot as cli
    from PIL import Image
    a, b = "ACGT" * 5 + "CAG" * 10 + "TTGACCATGGTCAA", "TTGACCATGGTCAA" + "CTG" * 22 + "ACGTAC" * 8
    plus, minus = P.kept_cells(a, b, "+", 3), P.kept_cells(a, b, "-", 3)
    raw = P.kept_cells(a, b, "+", 0) | P.kept_cells(a, b, "-", 0)
    marked = np.where(plus, 1, np.where(minus, cli.MINUS_ONLY, 0)) + 2 * (raw & ~plus & ~minus)
    assert marked.shape == (64, 128) and set(np.unique(marked)) == {0, 1, 2, 3}
    out = tmp_path / "pair.png"
    cli.plot_dot_plot(marked.astype(np.uint8), save_path=str(out), figure_size=4)
    with Image.open(out) as image:
        # 4 inches at 100 dpi along the 128 columns, cropped to the axes (77 % of the figure), half as high
        assert image.format == "PNG" and 290 <= image.size[0] <= 400 and abs(image.size[0] / image.size[1] - 2.0) < 0.06
        colours = {c[:3] for _, c in image.convert("RGB").getcolors(1 << 20)}
    assert {(255, 255, 255), (0, 0, 0), (255, 0, 0), (65, 105, 225)} <= colours
    out2 = tmp_path / "tall.png"
    cli.plot_dot_plot(plus.T.astype(np.uint8).tolist(), save_path=str(out2))               # a list of lists; 5 * 128 / 150 inches high
    with Image.open(out2) as image:
        assert abs(image.size[1] / image.size[0] - 2.0) < 0.06 and 310 <= image.size[1] <= 430
    out3 = tmp_path / "density.png"
    cli.plot_density(np.array([[4096, 10, 0], [10, 36, 6]], dtype=np.uint32), 64, 70, save_path=str(out3), n_cols=134)
    with Image.open(out3) as image:
        assert image.format == "PNG" and image.size[0] > image.size[1]
