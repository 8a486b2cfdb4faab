"""CPU: the exact dot plot (prf_dotplot_bits / prf_dotplot_counts, plot_dot_plot.py).  The numpy model
(tests/dotplot_model.py) equals the reference's generate_matrix + filter_out_noise on every case of
tests/golden/dotplot.jsonl.gz, the host filter_out_noise equals the fixture and, on matrices that are no dot plots, the model;
the refusals of the new entry points are decided before the context is looked at (NULL context, no GPU needed).  The command
line's checks and the plot function run on the host as well."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import dotplot_model as D
from conftest import ROOT, load_jsonl_gz


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("dotplot.jsonl.gz")


def test_the_fixture_is_what_the_tool_promises(golden):
    assert 130 <= len(golden) <= 170
    lengths = {len(c["seq"]) for c in golden}
    assert {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193} <= lengths and max(lengths) <= 200
    assert {c["t"] for c in golden} == {0, 1, 2, 3, 4, 5, 8, 16, 63, 64}
    assert any(set(c["seq"]) == {"N"} and len(c["seq"]) > 60 for c in golden)
    assert any({"R", "Y", "K", "N"} <= set(c["seq"]) for c in golden)
    assert any(c["tag"].startswith("palindrome") for c in golden) and any(c["tag"].startswith("tandem") for c in golden)
    assert all(c["seq"] == c["seq"].upper() and len(c["kept"]) == len(c["seq"]) for c in golden)
    # N == N is a match: a case of nothing but N at a threshold that a long run passes keeps every cell
    c = next(c for c in golden if set(c["seq"]) == {"N"} and len(c["seq"]) >= 65 and c["t"] <= 64)
    assert D.fixture_cells(c).all()
    # the anti-diagonal is exercised: some kept cell has no main-diagonal neighbour
    c = next(c for c in golden if c["tag"].startswith("palindrome") and c["t"] == 3)
    cells = D.fixture_cells(c)
    raw = D.kept_cells(c["seq"], 0)
    lonely = cells[1:-1, 1:-1] & ~raw[:-2, :-2] & ~raw[2:, 2:]
    assert lonely.any()


def test_model_equals_the_reference(golden):
    bad = [c["tag"] for c in golden if not np.array_equal(D.kept_cells(c["seq"], c["t"]), D.fixture_cells(c))]
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_model_windows_equal_the_whole_matrix(golden):
    rng = random.Random(3)
    for c in golden[::7]:
        n = len(c["seq"])
        whole = D.fixture_cells(c)
        r0, c0 = rng.randrange(0, n + 1), rng.randrange(0, n + 1)
        r1, c1 = rng.randrange(r0, n + 40), rng.randrange(c0, n + 40)
        assert np.array_equal(D.kept_cells(c["seq"], c["t"], rows=(r0, r1), cols=(c0, c1)), whole[r0:r1, c0:c1]), c["tag"]
    seq = "ACGTTGCAAC" * 30
    inner = D.kept_cells(seq, 4, 17, 250)
    assert np.array_equal(inner, D.kept_cells(seq[17:250], 4))
    cells = D.kept_cells(seq, 3, rows=(5, 290), cols=(64, 200))
    assert np.array_equal(D.block_sums(cells, 64), [[cells[r:r + 64, c:c + 64].sum() for c in (0, 64, 128)] for r in range(0, 285, 64)])
    assert D.kept_bits(seq, 3, rows=(5, 6), cols=(64, 200)).shape == (1, 3)


@pytest.mark.parametrize("set_noise_to", [0, 2])
def test_host_filter_equals_the_fixture(golden, set_noise_to):
    import plot_dot_plot as cli
    bad = []
    for i, c in enumerate(golden):
        raw = D.kept_cells(c["seq"], 0).astype(np.int64)
        want = D.fixture_cells(c).astype(np.int64)
        want += set_noise_to * (raw & ~want & 1)
        matrix = raw.tolist() if i % 2 else raw.copy()            # a list of lists, as the reference's, or an array
        assert cli.filter_out_noise(matrix, c["t"], set_noise_to) is None
        if not np.array_equal(np.asarray(matrix).reshape(want.shape), want):
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_host_filter_equals_the_model_on_matrices_that_are_no_dot_plots():
    import plot_dot_plot as cli
    rng = np.random.default_rng(11)
    for k in range(50):
        n = int(rng.integers(1, 31))
        t = int(rng.choice([0, 1, 2, 3, 4, 5, 8, 31]))
        cells = (rng.random((n, n)) < rng.choice([0.3, 0.6, 0.9])).astype(np.int64)      # not symmetric, diagonal not set
        want = D.filter_matrix(cells, t)
        matrix = cells.tolist()
        cli.filter_out_noise(matrix, min_diagonal_run=t, set_noise_to=2)
        assert np.array_equal(np.asarray(matrix), want + 2 * (cells & ~want & 1)), (k, n, t)
        for i, j in ((0, 0), (n // 2, n - 1), (n - 1, n // 3)):
            assert cli.is_noise(cells.tolist(), i, j, t) == (not want[i, j]), (k, i, j)


# ---- the C ABI: refusals are decided before the context is looked at (NULL context) ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _call(lib, pn, form, seq=b"ACGTACGTAC", begin=0, end=10, rows=(0, 10), cols=(0, 10), t=3, block=None, capacity=4096, dst=True,
          sizes=True):
    buf = (ctypes.c_uint64 * 4096)()
    n0, n1, stats = ctypes.c_uint64(0), ctypes.c_uint64(0), pn.ScanStats()
    p0, p1 = (ctypes.byref(n0), ctypes.byref(n1)) if sizes else (None, None)
    window = (begin, end, rows[0], rows[1], cols[0], cols[1], t)
    out = buf if dst else None
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        if block is None:
            return lib.prf_dotplot_bits_seq(None, arr, *window, out, capacity, p0, ctypes.byref(stats))
        return lib.prf_dotplot_counts_seq(None, arr, *window, block, out, capacity, p0, p1, ctypes.byref(stats))
    if form == "ex":
        if block is None:
            return lib.prf_dotplot_bits_ex(None, None, 0, *window, out, capacity, p0, ctypes.byref(stats), 4096)
        return lib.prf_dotplot_counts_ex(None, None, 0, *window, block, out, capacity, p0, p1, ctypes.byref(stats), 4096)
    if block is None:
        return lib.prf_dotplot_bits(None, None, 0, *window, out, capacity, p0, ctypes.byref(stats))
    return lib.prf_dotplot_counts(None, None, 0, *window, block, out, capacity, p0, p1, ctypes.byref(stats))


def test_entry_points_are_declared_bound_and_exported():
    """What tests/test_abi.py checks for prf.h and prf_native.EXPORTS, for prf_dotplot.h and prf_native.DOTPLOT_EXPORTS."""
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_dotplot.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.DOTPLOT_EXPORTS) and len(declared) == 7
    assert not set(declared) & (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS))
    assert '#include "prf_dotplot.h"' in open(os.path.join(ROOT, "include", "prf.h")).read()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "prf_dotplot.h")).read()
    assert f"PRF_DOT_LAUNCH_CELLS (1ull << {pn.DOT_LAUNCH_CELLS.bit_length() - 1})" in header
    assert f"PRF_DOT_MAX_CELLS (1ull << {pn.DOT_MAX_CELLS.bit_length() - 1})" in header


REFUSALS = [
    (dict(begin=7, end=3), "PRF_EINVAL", "begin"),
    (dict(rows=(5, 4)), "PRF_EINVAL", "row0"),
    (dict(cols=(9, 2)), "PRF_EINVAL", "col0"),
    (dict(t=65), "PRF_EUNSUPPORTED", "min_diagonal_run 65"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(sizes=False), "PRF_EINVAL", "NULL size pointer"),
    (dict(block=64, dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(block=0), "PRF_EINVAL", "block"),
    (dict(block=32), "PRF_EINVAL", "block"),
    (dict(block=100), "PRF_EINVAL", "block"),
    (dict(block=32832), "PRF_EINVAL", "block"),
    (dict(), "PRF_EINVAL", "NULL context"),                             # valid arguments
    (dict(t=64, block=32768), "PRF_EINVAL", "NULL context"),
    (dict(t=0, rows=(3, 3)), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", REFUSALS)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(capacity=9), "PRF_EINVAL", "destination holds 9 words"),                              # 10 rows x 1 word
    (dict(seq=b"A" * 200, end=200, rows=(0, 200), cols=(0, 200), capacity=799), "PRF_EINVAL", "the output has 800 (200 x 4)"),
    (dict(seq=b"A" * 200, end=200, rows=(0, 200), cols=(0, 200), block=64, capacity=15), "PRF_EINVAL", "the output has 16 (4 x 4)"),
    (dict(seq=b"A" * 200, end=100, rows=(0, 200), cols=(0, 200), block=64, capacity=4), "PRF_EINVAL", "NULL context"),   # clipped: 2 x 2
    (dict(seq=b"A" * 10, end=1 << 40, rows=(0, 1 << 60), cols=(2, 1 << 63), capacity=10), "PRF_EINVAL", "NULL context"),
    (dict(seq=b"A" * 10, rows=(20, 30), cols=(0, 10), capacity=0), "PRF_EINVAL", "NULL context"),   # an empty window needs no room
    (dict(seq=b"ACGT-ACGTA"), "PRF_ESYMBOL", "position 4"),
    (dict(seq=b"ACGT1ACGTA", block=64), "PRF_ESYMBOL", "position 4"),
    (dict(seq=b"", end=0), "PRF_EINVAL", "NULL context"),
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


def test_outputs_and_windows_above_the_documented_limits_are_refused():
    """2^28 entries per call (PRF_PERIOD_BITS_MAX_WORDS), 2^42 cells per call (PRF_DOT_MAX_CELLS).  The sequence is never read:
    the sizes are judged first."""
    pn, lib = _lib()
    n = 1 << 22
    arr = (pn._Contig * 1)()
    block = ctypes.create_string_buffer(16)
    arr[0].ascii, arr[0].len = ctypes.addressof(block), n
    n0, n1, stats, dst = ctypes.c_uint64(0), ctypes.c_uint64(0), pn.ScanStats(), (ctypes.c_uint64 * 1)()
    rc = lib.prf_dotplot_bits_seq(None, arr, 0, n, 0, n, 0, n, 3, dst, 1 << 60, ctypes.byref(n0), ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_PERIOD_BITS_MAX_WORDS" in lib.prf_last_error().decode()     # 2^22 x 2^16 words
    rc = lib.prf_dotplot_counts_seq(None, arr, 0, n, 0, n, 0, n, 3, 32768, dst, 1 << 60, ctypes.byref(n0), ctypes.byref(n1),
                                    ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()               # 2^44 cells, 2^14 counts


def test_shape_function_needs_no_gpu():
    pn, _ = _lib()
    for t in (0, 2, 3, 5, 18, 19, 64):
        tile_rows, span_words, halo = pn.dotplot_shape(t)
        assert halo == max(t - 2, 0) and tile_rows == 64 and span_words in (30, 62)
        raw_rows, words = tile_rows + 2 * halo, span_words + 2
        assert words & (words - 1) == 0                                       # a power of two of words per raw row
        assert (raw_rows * words + 8 * (words + 2)) * 8 + (raw_rows + 1 + words) * 4 <= 65536          # the LDS of a workgroup, 8 planes
    with pytest.raises(pn.PrfError) as info:
        pn.dotplot_shape(65)
    assert info.value.code == pn.PRF_EUNSUPPORTED


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="block"):
        g.dotplot_counts(0, 100)
    with pytest.raises(ValueError, match="contig"):
        g.dotplot_bits(3)
    with pytest.raises(ValueError, match="rows"):
        g.dotplot_bits(0, rows=(5, 4))
    with pytest.raises(ValueError, match="min_diagonal_run"):
        g.dotplot_bits(0, -1)
    with pytest.raises(ValueError, match="begin"):
        g.dotplot_bits(0, begin=7, end=3)
    g._h = None
    bits = np.array([[0b101, 1], [0, 1 << 63]], dtype=np.uint64)
    cells = pn.unpack_bits(bits, 70)
    assert cells.shape == (2, 70) and cells.dtype == np.uint8
    assert cells[0].nonzero()[0].tolist() == [0, 2, 64] and cells[1].nonzero()[0].tolist() == []
    assert pn.unpack_bits(bits, 128)[1, 127] == 1 and pn.unpack_bits(bits[:0], 5).shape == (0, 5)


# ---- command line and plots ----

def _resolve(cli, argv):
    parser = cli.build_parser()
    return cli.resolve_inputs(parser.parse_args(argv), parser)


def test_cli_parses_literals_intervals_and_bed_files(tmp_path, capsys):
    import plot_dot_plot as cli
    assert cli.parse_interval("chr1:12345-54321") == ("chr1", 12345, 54321)
    assert cli.parse_interval("HLA:A*01:5-9") == ("HLA:A*01", 5, 9)
    with pytest.raises(ValueError, match="Unable to parse interval"):
        cli.parse_interval("chr1:5")
    # only literal sequences: the reference raises NameError at its "Loaded ..." line; here the line is left out
    out = _resolve(cli, ["ACGTACGT", "-o", "x.png", "-d", str(tmp_path)])
    assert out == [("sequence", 0, "ACGTACGT", str(tmp_path / "x.png"))] and "Loaded" not in capsys.readouterr().out
    out = _resolve(cli, ["ACGT", "GGGTT"])
    assert [os.path.basename(o[3]) for o in out] == ["dot_plot_001_of_2.4bp_sequence.png", "dot_plot_002_of_2.5bp_sequence.png"]
    fa = tmp_path / "g.fa"
    chrom = "ACGTTGCAGT" * 60
    fa.write_text(">chr7 some text\n" + "\n".join(chrom[i:i + 50] for i in range(0, 600, 50)) + "\n>chrB\nacgtn\n")
    out = _resolve(cli, ["-R", str(fa), "chr7:10-30"])
    assert out[0][:3] == ("chr7", 10, chrom[10:30]) and out[0][3].endswith("dot_plot_001_of_1.chr7_10-30.20bp_sequence.png")
    assert "Loaded 1 interval(s)" in capsys.readouterr().out
    out = _resolve(cli, ["-R", str(fa), "7:10-30", "-p", "25"])                  # the padded start is clamped to 0
    assert out[0][:3] == ("chr7", 0, chrom[0:55])
    bed = tmp_path / "regions.bed"
    bed.write_text("chr7\t100\t140\tx\nchrB\t1\t4\n")
    out = _resolve(cli, ["-p", "2", "-R", str(fa), str(bed), "ACCA"])
    assert [o[:3] for o in out] == [("chr7", 98, chrom[98:142]), ("chrB", 0, "ACGTN"), ("sequence", 0, "ACCA")]
    assert "Loaded 2 interval(s)" in capsys.readouterr().out
    for argv, text in ((["chr7:1-5"], "--reference-fasta is required"), (["ACGU"], "not a valid nucleotide sequence"),
                       (["-R", str(fa), "chrZ:1-5"], "not found"), (["-R", str(fa), str(tmp_path / "none.bed")], "file not found"),
                       (["ACGT", "-t", "65"], "between 0 and 64"), (["ACGT", "--block", "100"], "multiple of 64"),
                       (["ACGT", "--tsv", "x.tsv"], "--block"), (["ACGT", "CCC", "--block", "64", "--tsv", "x"], "one input")):
        with pytest.raises(SystemExit):
            _resolve(cli, argv)
        assert text in capsys.readouterr().err


def test_cli_requires_block_above_5000_positions(tmp_path, capsys):
    import plot_dot_plot as cli
    with pytest.raises(SystemExit):
        _resolve(cli, ["ACGT" * 1251])
    assert "--block" in capsys.readouterr().err
    assert len(_resolve(cli, ["ACGT" * 1250])[0][2]) == 5000
    assert len(_resolve(cli, ["ACGT" * 1251, "--block", "64"])[0][2]) == 5004
    fa = tmp_path / "x.fa"
    fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    with pytest.raises(SystemExit):
        _resolve(cli, ["-R", str(fa), "chrA:10-7000"])
    assert "--block" in capsys.readouterr().err
    assert len(_resolve(cli, ["-R", str(fa), "chrA:10-7000", "--block", "128"])[0][2]) == 6990


def test_density_lines_list_the_nonzero_blocks():
    import plot_dot_plot as cli
    counts = np.array([[3, 0], [0, 5]], dtype=np.uint32)
    assert list(cli.density_lines("chr1", 100, 100, 64, counts)) == ["chr1\t100\t164\t100\t164\t3\n", "chr1\t164\t200\t164\t200\t5\n"]


def test_plot_writes_a_png_of_the_expected_size(tmp_path):
    import plot_dot_plot as cli
    from PIL import Image
    seq = "ACGT" * 5 + "CAG" * 10 + "TTGACCATGGTCAA"
    cells = D.kept_cells(seq, 3).astype(np.uint8)
    marked = cells + 2 * (D.kept_cells(seq, 0) & ~cells.astype(bool))
    out = tmp_path / "dots.png"
    cli.plot_dot_plot(marked.tolist(), save_path=str(out), figure_size=3)
    with Image.open(out) as image:
        # 3 inches at 100 dpi, cropped to the axes, which matplotlib's default margins put at 77 % of the figure
        assert image.format == "PNG" and image.size[0] == image.size[1] and 220 <= image.size[0] <= 300
        colours = {c[:3] for _, c in image.convert("RGB").getcolors(1 << 20)}
    assert {(255, 255, 255), (0, 0, 0), (255, 0, 0)} <= colours
    out2 = tmp_path / "default.png"
    cli.plot_dot_plot(cells.tolist(), save_path=str(out2))                        # 5 * 64 / 150 inches
    with Image.open(out2) as image:
        assert image.size[0] == image.size[1] and 155 <= image.size[0] <= 215
    out3 = tmp_path / "density.png"
    cli.plot_density(np.array([[4096, 10], [10, 36]], dtype=np.uint32), 64, 70, save_path=str(out3))
    with Image.open(out3) as image:
        assert image.format == "PNG" and image.size[0] == image.size[1]
