"""CPU: the periodicity matrix (prf_period_bits / prf_period_counts, utils/plot_utils.py, plot_periodicity_matrix.py).
The numpy model (tests/periodicity_model.py) equals the reference's get_period_matrix on every case of
tests/golden/periodicity.jsonl.gz in its set cells, period_classes reproduces the reference's partition of them, the model's
counts are the windowed sums of its bits, and the refusals of the new entry points are decided before the context is looked at
(NULL context, no GPU needed).  The command line's checks and the two plot functions run on the host as well."""
import ctypes
import random

import numpy as np
import pytest

import periodicity_model as P
from conftest import load_jsonl_gz


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("periodicity.jsonl.gz")


def fixture_cells(case):
    """bool[rows, columns] from the hex rows of a fixture case."""
    rows, cols = case["shape"]
    out = np.zeros((rows, cols), dtype=bool)
    for r, text in enumerate(case["cells"]):
        value = int(text, 16)
        out[r] = [(value >> i) & 1 for i in range(cols)]
    return out


def partition(values):
    """Class numbers in order of first appearance of the nonzero entries of one matrix row."""
    seen = {}
    return [seen.setdefault(v, len(seen)) for v in values if v]


def clamped(case):
    """(min, max) after the reference's clamps (utils/plot_utils.py:13-14)."""
    return max(case["min"], 1), min(case["max"], len(case["seq"]) // 2)


def test_the_fixture_is_what_the_tool_promises(golden):
    assert 280 <= len(golden) <= 320
    lengths = {len(c["seq"]) for c in golden}
    assert {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193} <= lengths and max(lengths) <= 600
    assert any(set(c["seq"]) == {"N"} for c in golden)
    assert any({"R", "Y", "K", "N"} <= set(c["seq"]) for c in golden)
    assert any(c["min"] > 1 for c in golden) and any(c["max"] > len(c["seq"]) // 2 for c in golden)
    assert any(c["max"] == 1 for c in golden)
    assert all(c["seq"] == c["seq"].upper() for c in golden)
    assert all(c["shape"] == [max(0, clamped(c)[1]), len(c["seq"])] for c in golden)
    # N == N is a match in the reference: a case of nothing but N has every cell i < len - k set
    c = next(c for c in golden if set(c["seq"]) == {"N"} and len(c["seq"]) == 65)
    assert fixture_cells(c)[0].sum() == 64


def test_model_equals_the_reference_in_set_cells(golden):
    bad = []
    for c in golden:
        lo, hi = clamped(c)
        want = fixture_cells(c)
        got = np.zeros_like(want)
        if hi >= lo:
            got[lo - 1:] = P.period_cells(c["seq"], lo, hi)
        if not np.array_equal(got, want):
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_period_classes_reproduces_the_partition(golden):
    from utils.plot_utils import period_classes
    bad = []
    for c in golden:
        lo, hi = clamped(c)
        if hi < lo:
            continue
        rows = period_classes(c["seq"], P.period_bits(c["seq"], lo, hi), lo)
        assert len(rows) == hi - lo + 1 and all(len(row) == len(c["seq"]) for row in rows)
        if [partition(row) for row in rows] != c["classes"][lo - 1:]:
            bad.append(c["tag"])
        if [[bool(v) for v in row] for row in rows] != fixture_cells(c)[lo - 1:].tolist():
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_period_classes_is_deterministic_and_nonzero():
    from utils.plot_utils import motif_value, period_classes
    seq = "ACGACGACGTTTTNNNN"
    a = period_classes(seq, P.period_bits(seq, 1, 8), 1)
    assert a == period_classes(seq, P.period_bits(seq, 1, 8), 1)
    assert a[2][0] == a[2][3] == motif_value("ACG") and a[0][13] == motif_value("N")
    assert motif_value("") > 0


@pytest.mark.parametrize("window", [64, 128, 192, 4096])
def test_model_counts_are_windowed_sums_of_its_bits(window):
    rng = random.Random(window)
    seq = "".join(rng.choice("ACGTNacgtR") for _ in range(1000)) + "ACG" * 200
    for begin, end in ((0, None), (1, 1599), (63, 700), (65, 10_000), (700, 700)):
        bits = P.period_bits(seq, 1, 40, begin, end)
        counts = P.period_counts(seq, 1, 40, window, begin, end)
        assert counts.dtype == np.uint32 and np.array_equal(counts, P.popcount_per_window(bits, window))
        n = max(0, min(len(seq), len(seq) if end is None else end) - begin)
        assert bits.shape == (40, -(-n // 64)) and counts.shape == (40, -(-n // window))
    # upper-casing, N == N, the end clip: "nN" matches at k = 1, the last position never does
    assert P.period_cells("nNaA", 1, 1).tolist() == [[True, False, True, False]]
    assert P.period_cells("AAAAAA", 2, 2, 1, 5).tolist() == [[True, True, False, False]]


# ---- the C ABI: refusals are decided before the context is looked at (NULL context) ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _one_shot(lib, pn, seq=b"ACGTACGTAC", begin=0, end=10, kmin=1, kmax=4, window=None, capacity=None, dst=True, ctx=None):
    arr, _keep = pn._contig_array([seq])
    buf = (ctypes.c_uint64 * 4096)()
    n, stats = ctypes.c_uint64(0), pn.ScanStats()
    cap = 4096 if capacity is None else capacity
    if window is None:
        return lib.prf_period_bits_seq(ctx, arr, begin, end, kmin, kmax, buf if dst else None, cap, ctypes.byref(n), ctypes.byref(stats))
    return lib.prf_period_counts_seq(ctx, arr, begin, end, kmin, kmax, window, buf if dst else None, cap, ctypes.byref(n),
                                     ctypes.byref(stats))


def _on_genome(lib, pn, begin=0, end=10, kmin=1, kmax=4, window=None, dst=True):
    buf = (ctypes.c_uint64 * 4096)()
    n, stats = ctypes.c_uint64(0), pn.ScanStats()
    if window is None:
        return lib.prf_period_bits(None, None, 0, begin, end, kmin, kmax, buf if dst else None, 4096, ctypes.byref(n), ctypes.byref(stats))
    return lib.prf_period_counts(None, None, 0, begin, end, kmin, kmax, window, buf if dst else None, 4096, ctypes.byref(n),
                                 ctypes.byref(stats))


def test_entry_points_are_declared_bound_and_exported():
    """What tests/test_abi.py checks for prf.h and prf_native.EXPORTS, for prf_period.h and prf_native.PERIOD_EXPORTS."""
    import os
    import re
    from conftest import ROOT
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_period.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.PERIOD_EXPORTS) and len(declared) == 4
    assert not set(declared) & set(pn.EXPORTS)
    assert '#include "prf_period.h"' in open(os.path.join(ROOT, "include", "prf.h")).read()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4


REFUSALS = [
    (dict(kmin=0), "PRF_EINVAL", "min_motif_size"),
    (dict(kmin=5, kmax=4), "PRF_EINVAL", "max_motif_size"),
    (dict(begin=7, end=3), "PRF_EINVAL", "begin"),
    (dict(window=0), "PRF_EINVAL", "window"),
    (dict(window=100), "PRF_EINVAL", "window"),
    (dict(window=32), "PRF_EINVAL", "window"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(window=64, dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(kmax=60001), "PRF_EUNSUPPORTED", "60000"),                    # check_params: above every kmax_hint
    (dict(), "PRF_EINVAL", "NULL context"),                             # valid arguments
    (dict(window=64), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", REFUSALS)
@pytest.mark.parametrize("form", ["genome", "one_shot"])
def test_refusals(form, kwargs, code, text):
    pn, lib = _lib()
    rc = (_on_genome if form == "genome" else _one_shot)(lib, pn, **kwargs)
    assert rc == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(capacity=3), "PRF_EINVAL", "destination holds 3 words"),                  # 4 motif sizes x 1 word
    (dict(window=64, capacity=3), "PRF_EINVAL", "destination holds 3 counts"),
    (dict(seq=b"A" * 200, end=200, window=64, kmax=2, capacity=7), "PRF_EINVAL", "the output has 8"),
    (dict(seq=b"A" * 200, end=100, window=64, kmax=2, capacity=4), "PRF_EINVAL", "NULL context"),   # clipped by `end`: 2 x 2 fit
    (dict(seq=b"A" * 10, end=1 << 40, capacity=4), "PRF_EINVAL", "NULL context"),    # `end` clipped to the sequence
    (dict(seq=b"ACGT-ACGT", end=9), "PRF_ESYMBOL", "position 4"),
    (dict(seq=b"ACGT1", end=5, window=64), "PRF_ESYMBOL", "position 4"),
    (dict(seq=b"", end=0), "PRF_EINVAL", "NULL context"),
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _one_shot(lib, pn, **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


def test_bits_output_above_the_documented_limit_is_refused():
    """PRF_PERIOD_BITS_MAX_WORDS (include/prf.h): 2^28 words.  The sequence is never read: the size is judged first."""
    pn, lib = _lib()
    n = 1 << 26                                   # 2^20 words per motif size x 257 motif sizes > 2^28
    arr = (pn._Contig * 1)()
    block = ctypes.create_string_buffer(16)
    arr[0].ascii, arr[0].len = ctypes.addressof(block), n
    out, stats, dst = ctypes.c_uint64(0), pn.ScanStats(), (ctypes.c_uint64 * 1)()
    rc = lib.prf_period_bits_seq(None, arr, 0, n, 1, 257, dst, 1 << 40, ctypes.byref(out), ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_PERIOD_BITS_MAX_WORDS" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="window"):
        g.period_counts(0, 1, 4, 100)
    with pytest.raises(ValueError, match="motif sizes"):
        g.period_bits(0, 4, 1)
    with pytest.raises(ValueError, match="contig"):
        g.period_bits(3, 1, 4)
    g._h = None


# ---- command line and plots ----

def test_cli_rejects_a_long_range_without_window(tmp_path, capsys):
    import plot_periodicity_matrix as cli
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.resolve_input(parser.parse_args(["ACGT" * 1251]), parser)
    assert "--window" in capsys.readouterr().err
    assert cli.resolve_input(parser.parse_args(["ACGT" * 1250]), parser)[2:] == (0, 5000)
    assert cli.resolve_input(parser.parse_args(["ACGT" * 1251, "--window", "64"]), parser)[2:] == (0, 5004)
    fa = tmp_path / "x.fa"
    fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n>chrB\nACGT\n")
    with pytest.raises(SystemExit):
        cli.resolve_input(parser.parse_args([str(fa), "-i", "chrA:10-7000"]), parser)
    assert "--window" in capsys.readouterr().err
    name, seq, begin, end = cli.resolve_input(parser.parse_args([str(fa), "-i", "chrA:10-9000", "--window", "128"]), parser)
    assert (name, len(seq), begin, end) == ("chrA", 8000, 10, 8000)
    for argv, text in ((["ACGT", "--window", "100"], "multiple of 64"), (["ACGT", "--tsv", "x.tsv"], "--window"),
                       ([str(fa)], "--interval"), ([str(fa), "-i", "chrC:0-5"], "not found"), (["ACGT", "-i", "a:0-3"], "FASTA"),
                       (["ACGT", "--min-motif-size", "0"], "at least 1"), (["AC-GT"], "Invalid input")):
        with pytest.raises(SystemExit):
            cli.resolve_input(parser.parse_args(argv), parser)
        assert text in capsys.readouterr().err


def test_profile_lines_list_the_nonzero_counts():
    import plot_periodicity_matrix as cli
    counts = np.array([[3, 0], [0, 5]], dtype=np.uint32)
    assert list(cli.profile_lines("chr1", 100, 200, 64, 2, counts)) == ["chr1\t100\t164\t2\t3\n", "chr1\t164\t200\t3\t5\n"]


PNG = b"\x89PNG\r\n\x1a\n"


def test_plots_write_a_png(tmp_path):
    from utils.plot_utils import period_classes, plot_periodicity_matrix, plot_results
    seq = "ACGT" * 3 + "CAG" * 10 + "TTGACCATGGTACCAGTN"
    assert len(seq) == 60
    matrix = period_classes(seq, P.period_bits(seq, 1, 10), 1)
    out = tmp_path / "matrix.png"
    plot_periodicity_matrix(matrix, str(out))
    assert out.read_bytes()[:8] == PNG and out.stat().st_size > 1000
    out2 = tmp_path / "results.png"
    plot_results(seq, [(0, 12, "ACGT"), (12, 42, "CAG"), (57, 60, "N")], 10, str(out2))    # a repeat that reaches the last position
    assert out2.read_bytes()[:8] == PNG and out2.stat().st_size > 1000
    out3 = tmp_path / "profile.png"
    plot_periodicity_matrix([[0.5, 0.25], [0.0, 1.0]], str(out3), fractions=[0.4, 0.5], extent=(100, 228), value_label="x")
    assert out3.read_bytes()[:8] == PNG
