"""CPU: the list of diagonal runs of the dot plot of two ranges (prf_dotpair_runs, plot_dot_plot.py --runs-tsv).  The
model (tests/dotruns_model.py) is pinned to the reference's filter by every case of tests/golden/dotpair.jsonl.gz: a cell is kept
at threshold t exactly when it lies on a run of at least t - 1 cells.  The refusals of the new entry points are decided before
the context is looked at (NULL context, no GPU needed), in the documented order; unique_runs, run_cells and the command line run
on the host as well."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import dotpair_model as P
import dotruns_model as R
from conftest import ROOT, load_jsonl_gz


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("dotpair.jsonl.gz")


def test_runs_of_the_model_cover_the_kept_cells_of_every_fixture_case(golden):
    import prf_native
    bad = []
    for c in golden:
        na, nb = len(c["a"]), len(c["b"])
        runs = R.runs(c["a"], c["b"], c["strand"], min_len=max(c["t"] - 1, 1))
        if not np.array_equal(R.cells(runs, na, nb), P.fixture_cells(c)):
            bad.append(c["tag"])
        assert np.array_equal(prf_native.run_cells(runs, na, nb), R.cells(runs, na, nb)), c["tag"]
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"
    assert sum(len(R.runs(c["a"], c["b"], c["strand"], min_len=2)) > 0 for c in golden) > 100


def test_runs_are_maximal_and_sorted():
    a, b = "ACGTTGCAACNN" * 9, "GTTGCAACGTNN" * 7 + "ACGTNNRYAC" * 3
    for strand in "+-":
        raw = P.kept_cells(a, b, strand, 0)
        runs = R.runs(a, b, strand)
        na, nb = raw.shape
        assert [tuple(r) for r in runs[["row", "col", "dir"]].tolist()] == sorted(tuple(r) for r in runs[["row", "col", "dir"]].tolist())
        for i, j, n, d in runs.tolist():
            dj = 1 if d == R.MAIN else -1
            assert all(raw[i + s, j + dj * s] for s in range(n))
            before = i - 1 >= 0 and 0 <= j - dj < nb and raw[i - 1, j - dj]
            after = i + n < na and 0 <= j + dj * n < nb and raw[i + n, j + dj * n]
            assert not before and not after, (i, j, n, d)
        for d in (R.MAIN, R.ANTI):                                            # the runs of one direction partition the raw cells
            part = runs[runs["dir"] == d]
            assert int(part["len"].sum()) == int(raw.sum()) and np.array_equal(R.cells(part, na, nb), raw)


def test_model_windows_add_up_to_the_whole_list(golden):
    rng = random.Random(11)
    for c in golden[::4]:
        na, nb = len(c["a"]), len(c["b"])
        whole = R.runs(c["a"], c["b"], c["strand"], min_len=2)
        r, k = rng.randrange(0, na + 1), rng.randrange(0, nb + 1)
        parts = [R.runs(c["a"], c["b"], c["strand"], rows=rows, cols=cols, min_len=2)
                 for rows in ((0, r), (r, na + 7)) for cols in ((0, k), (k, None))]
        both = np.concatenate(parts)
        assert len(both) == len(whole) and R.same(np.sort(both, order=["row", "col", "dir"]), whole), c["tag"]     # each once, unclipped
    one = R.runs("ACGTACGTACGT", "ACGTACGTACGT", "+", rows=(4, 5), cols=(0, 1), min_len=3)
    assert one.tolist() == [(4, 0, 8, R.MAIN)]                               # the start decides, the length is not clipped
    assert len(R.runs("ACGTACGTACGT", "ACGTACGTACGT", "+", rows=(5, 9), cols=(1, 5), min_len=3)) == 0          # only middles of runs
    assert R.runs("ACGT", "ACGT", "+", directions="anti", min_len=1)["dir"].tolist() == [R.ANTI] * 4


def _brute_unique(runs, strand):
    """One run of every mirror pair, by pairing the runs through their sets of cells."""
    cells = {}
    for i, j, n, d in runs.tolist():
        dj = 1 if d == R.MAIN else -1
        cells[(i, j, n, d)] = frozenset((i + s, j + dj * s) for s in range(n))
    by_cells = {v: k for k, v in cells.items()}
    keep = []
    for run, own in cells.items():
        i, j, n, d = run
        mirror = by_cells[frozenset((y, x) for x, y in own)]                  # raw is symmetric: the mirror image is a run too
        if mirror == run:
            if not (d == R.MAIN and strand == "+"):                           # the trivial diagonal
                keep.append(run)
        elif (d == R.MAIN and j > i) or (d == R.ANTI and run < mirror):       # the upper one; anti: the smaller start row
            keep.append(run)
    return sorted(keep, key=lambda r: (r[0], r[1], r[3]))


def test_unique_runs_against_a_brute_force_pairing():
    import prf_native
    rng = random.Random(3)
    u = "".join(rng.choice("ACGT") for _ in range(23))
    palindrome = "ACCTGAATTCAGGT"                                             # its own reverse complement: a self-mirrored anti run
    assert P.revcomp(palindrome.encode()).decode() == palindrome
    noise = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    seq = noise(40) + u + noise(31) + u + noise(17) + P.revcomp(u.encode()).decode() + noise(29) + palindrome + noise(33) + "NNNSW"
    n = len(seq)
    for strand in "+-":
        runs = R.runs(seq, seq, strand, min_len=3)
        got = prf_native.unique_runs(runs, strand)
        want = _brute_unique(runs, strand)
        assert [tuple(r) for r in got.tolist()] == want, strand
        assert 2 * len(got) >= len(runs) - 1 and len(got) < len(runs)
        if strand == "+":
            assert not ((got["row"] == got["col"]) & (got["dir"] == R.MAIN)).any()
            assert any(r[3] == R.MAIN and r[1] - r[0] == 23 + 31 and r[0] <= 40 and r[0] + r[2] >= 63 for r in got.tolist())    # the direct copy
        else:
            at = seq.index(palindrome)
            assert any(r[3] == R.ANTI and r[0] <= at and r[0] + r[2] >= at + 14 and r[0] == r[1] - r[2] + 1 for r in got.tolist())
            assert any(r[3] == R.ANTI and r[2] >= 23 and r[0] <= 40 for r in got.tolist())                                    # the inverted copy
            assert any(r[3] == R.MAIN and r[0] == r[1] for r in got.tolist())                                                 # N, S, W on the diagonal stay
        # the kept half and its mirror image give back all cells but the trivial diagonal's
        half = prf_native.run_cells(got, n, n)
        full = prf_native.run_cells(runs, n, n)
        if strand == "+":
            full &= ~np.eye(n, dtype=bool) | prf_native.run_cells(runs[runs["dir"] == R.ANTI], n, n)
        assert np.array_equal(half | half.T, full)
    assert len(prf_native.unique_runs(np.zeros(0, dtype=prf_native.DOTRUN_DTYPE))) == 0


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_dotruns.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.DOTRUNS_EXPORTS) and len(declared) == 3
    assert not set(declared) & (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS))
    assert '#include "prf_dotruns.h"' in open(os.path.join(ROOT, "include", "prf.h")).read()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4
    for name, value in (("PRF_DOTRUN_MAX_ROWS", pn.DOTRUN_MAX_ROWS), ("PRF_DOTRUN_LONG_ROWS", pn.DOTRUN_LONG_ROWS),
                        ("PRF_DOTRUN_PROBE", pn.DOTRUN_PROBE), ("PRF_DOTRUN_FOLLOW", pn.DOTRUN_FOLLOW)):
        found = re.search(rf"#define {name} \(?(?:(\d+)ull << (\d+)|(\d+)u)\)?", text)
        assert found and (int(found[1]) << int(found[2]) if found[1] else int(found[3])) == value, name
    assert 2 <= pn.DOTRUN_PROBE <= 63 and pn.DOTRUN_FOLLOW % 64 == 0
    assert np.dtype(pn.DOTRUN_DTYPE).itemsize == 32


def _call(lib, pn, form, seq_a=b"ACGTACGTAC", seq_b=b"ACGTACGTACGT", a=(0, 10), b=(0, 12), strand=0, rows=(0, 10), cols=(0, 12),
          directions=3, min_len=3, capacity=64, dst=True, n_runs=True):
    buf = np.full(64, 0xAB, dtype=np.uint8).repeat(32)
    n, stats = ctypes.c_uint64(77), pn.ScanStats()
    tail = (strand, rows[0], rows[1], cols[0], cols[1], directions, min_len, buf.ctypes.data if dst else None, capacity,
            ctypes.byref(n) if n_runs else None, ctypes.byref(stats))
    if form == "one_shot":
        arr_a, _keep_a = pn._contig_array([seq_a])
        arr_b, _keep_b = pn._contig_array([seq_b])
        rc = lib.prf_dotpair_runs_seq(None, arr_a, *a, arr_b, *b, *tail)
    elif form == "ex":
        rc = lib.prf_dotpair_runs_ex(None, None, 0, *a, 1, *b, *tail, 4096)
    else:
        rc = lib.prf_dotpair_runs(None, None, 0, *a, 1, *b, *tail)
    assert (buf == 0xAB).all() and n.value == 77                              # a refused call writes nothing
    return rc


# each case breaks one rule and every rule behind it: the first in the documented order is the one reported
LATER = dict(rows=(5, 4), cols=(9, 2), strand=2, directions=4, min_len=0, capacity=(1 << 24) + 1, dst=False, n_runs=False)


def _later(*fixed):
    return {k: v for k, v in LATER.items() if k not in fixed}


ORDER = [
    (dict(a=(7, 3), b=(8, 2), **LATER), "PRF_EINVAL", "a_begin 7"),
    (dict(b=(8, 2), **LATER), "PRF_EINVAL", "b_begin 8"),
    (dict(LATER), "PRF_EINVAL", "row0"),
    (_later("rows"), "PRF_EINVAL", "col0"),
    (_later("rows", "cols"), "PRF_EINVAL", "strand is 2"),
    (_later("rows", "cols", "strand"), "PRF_EINVAL", "directions is 4"),
    (dict(_later("rows", "cols", "strand"), directions=0), "PRF_EINVAL", "directions is 0"),
    (_later("rows", "cols", "strand", "directions"), "PRF_EINVAL", "min_len is 0"),
    (_later("rows", "cols", "strand", "directions", "min_len"), "PRF_EUNSUPPORTED", "PRF_DOTRUN_MAX_ROWS"),
    (dict(dst=False, n_runs=False), "PRF_EINVAL", "NULL n_runs"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(dst=False, capacity=0), "PRF_EINVAL", "NULL context"),              # counting only is a valid call
    (dict(strand=0xFFFFFFFF), "PRF_EINVAL", "strand"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(strand=1, directions=1, min_len=1 << 40, capacity=1 << 24), "PRF_EINVAL", "NULL context"),
    (dict(directions=2, rows=(3, 3), a=(4, 4)), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_dotpair_runs")


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(seq_a=b"ACGT-ACGTA"), "PRF_ESYMBOL", "position 4"),
    (dict(seq_b=b"ACGTAC1TACGT"), "PRF_ESYMBOL", "position 6"),
    (dict(seq_b=b"", b=(0, 0)), "PRF_EINVAL", "NULL context"),                # an empty side
    (dict(a=(0, 1 << 40), b=(2, 1 << 63), rows=(0, 1 << 60), cols=(2, 1 << 63)), "PRF_EINVAL", "NULL context"),   # ends are clipped
])
def test_refusals_that_need_the_sequences(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


def test_a_missing_sequence_and_a_window_above_the_limit_are_refused():
    pn, lib = _lib()
    arr, _keep = pn._contig_array([b"ACGT"])
    n, stats = ctypes.c_uint64(0), pn.ScanStats()
    for first, second in ((None, arr), (arr, None)):
        rc = lib.prf_dotpair_runs_seq(None, first, 0, 4, second, 0, 4, 0, 0, 4, 0, 4, 3, 2, None, 0, ctypes.byref(n), ctypes.byref(stats))
        assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()
    # 2^44 cells: judged from the lengths, the sequences are never read
    big = (pn._Contig * 1)()
    block = ctypes.create_string_buffer(16)
    big[0].ascii, big[0].len = ctypes.addressof(block), 1 << 22
    rc = lib.prf_dotpair_runs_seq(None, big, 0, 1 << 22, big, 0, 1 << 22, 1, 0, 1 << 22, 0, 1 << 22, 3, 64, None, 0, ctypes.byref(n),
                                  ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g, other = pn.Genome(None, None, 2, [100, 50]), pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="contig 2"):
        g.dotpair_runs((0, 0, None), (2, 0, None))
    with pytest.raises(ValueError, match="strand"):
        g.dotpair_runs((0, 0, None), (1, 0, None), strand="x")
    with pytest.raises(ValueError, match="directions"):
        g.dotpair_runs((0, 0, None), (1, 0, None), directions="up")
    with pytest.raises(ValueError, match="min_len"):
        g.dotpair_runs((0, 0, None), (1, 0, None), min_len=0)
    with pytest.raises(ValueError, match="cols"):
        g.dotpair_runs((0, 0, None), (1, 0, None), cols=(5, 4))
    with pytest.raises(ValueError, match="begin"):
        g.dotpair_runs((0, 0, None), (1, 7, 3))
    with pytest.raises(ValueError, match="same resident genome"):
        pn._runs(None, (g, 0), (0, None), (other, 0), (0, None), "+", "both", 3, None, None, False, 0)
    with pytest.raises(ValueError, match="both be sequences or both"):
        pn._runs(None, (g, 0), (0, None), "ACGT", (0, None), "+", "both", 3, None, None, False, 0)
    g._h = other._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_inputs(args, parser), cli.resolve_versus(args, parser), args


def test_cli_parses_the_runs_options(tmp_path, capsys):
    import plot_dot_plot as cli
    out, versus, args = _parse(cli, ["ACGTACGT", "--runs-tsv", "r.tsv", "--min-run", "4"])
    assert args.runs_tsv == "r.tsv" and args.min_run == 4 and args.run_directions == "both" and cli.no_image(args)
    assert _parse(cli, ["ACGT", "--runs-tsv", "r.tsv", "--min-run", "1", "--run-directions", "anti"])[2].run_directions == "anti"
    assert not cli.no_image(_parse(cli, ["ACGT", "--runs-tsv", "r.tsv", "--min-run", "9", "-o", "x.png"])[2])
    # nothing changes for a command line without the new options
    out, _, args = _parse(cli, ["ACGTACGT", "-d", str(tmp_path)])
    assert out == [("sequence", 0, "ACGTACGT", str(tmp_path / "dot_plot.png"))] and args.runs_tsv is None and not cli.no_image(args)
    # above 5 000 positions the list needs no --block when no image is asked for
    long_fa = tmp_path / "x.fa"
    long_fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    out, versus, _ = _parse(cli, ["-R", str(long_fa), "chrA:100-7100", "--versus", "chrA:500-6500", "--runs-tsv", "r.tsv", "--min-run", "30"])
    assert len(out[0][2]) == 7000 and versus[:2] == ("chrA", 500) and len(versus[2]) == 6000
    capsys.readouterr()
    for argv, text in ((["ACGT", "--runs-tsv", "r.tsv"], "--min-run"), (["ACGT", "--min-run", "5"], "--runs-tsv"),
                       (["ACGT", "--runs-tsv", "r.tsv", "--min-run", "0"], "at least 1"),
                       (["ACGT", "--runs-tsv", "r.tsv", "--min-run", "3", "--run-directions", "up"], "invalid choice"),
                       (["ACGT", "TTGA", "--runs-tsv", "r.tsv", "--min-run", "3"], "takes one input"),
                       (["-R", str(long_fa), "chrA:0-7000", "--runs-tsv", "r.tsv", "--min-run", "30", "-o", "x.png"], "--block"),
                       (["ACGT", "-R", str(long_fa), "--versus", "chrA:0-7000", "--runs-tsv", "r.tsv", "--min-run", "30", "-o", "x.png"],
                        "--block")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err


def test_run_lines_are_in_genomic_coordinates():
    import plot_dot_plot as cli
    import prf_native
    runs = np.array([(5, 9, 4, 1, 0), (5, 9, 3, 2, 0), (0, 0, 1, 2, 0)], dtype=prf_native.DOTRUN_DTYPE)
    assert list(cli.run_lines("chr1", 100, "chrX", 1000, "-", runs)) == [
        "chr1\t105\t109\tchrX\t1009\t1013\t-\tmain\t4\n",                     # rows 5 .. 8, columns 9 .. 12
        "chr1\t105\t108\tchrX\t1007\t1010\t-\tanti\t3\n",                     # rows 5 .. 7, columns 9, 8, 7
        "chr1\t100\t101\tchrX\t1000\t1001\t-\tanti\t1\n"]


class _StubContext:
    """Serves dotpair_runs from the model, so that the command line's path runs without a GPU."""

    def __init__(self):
        self.calls = []

    def dotpair_runs(self, seq_a, seq_b, strand="+", directions="both", min_len=16):
        import prf_native
        self.calls.append((len(seq_a), len(seq_b), strand, directions, min_len))
        got = R.runs(seq_a, seq_b, strand, directions=directions, min_len=min_len)
        out = np.zeros(len(got), dtype=prf_native.DOTRUN_DTYPE)
        for f in ("row", "col", "len", "dir"):
            out[f] = got[f]
        return out[["row", "col", "len", "dir"]]


def test_cli_writes_the_runs_of_a_stubbed_list(tmp_path, capsys):
    import plot_dot_plot as cli
    rng = random.Random(9)
    u = "".join(rng.choice("ACGT") for _ in range(40))
    noise = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    # the letters next to the copies are chosen so that chance lengthens none of them: A and C are not complements of themselves
    chrom = noise(289) + "C" + noise(9) + "A" + u + "C" + noise(159)
    other = noise(89) + "C" + P.revcomp(u.encode()).decode() + "A" + noise(69)
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + chrom + "\n")
    tsv, ctx = tmp_path / "runs.tsv", _StubContext()
    cli.main(["-R", str(fa), "chrT:250-400", "--versus", "other:50-200", "--strand", "both", "--runs-tsv", str(tsv), "--min-run", "30",
              "-d", str(tmp_path)], context=ctx)
    assert ctx.calls == [(150, 150, "+", "both", 30), (150, 150, "-", "both", 30)]
    lines = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert len(lines) == 1 and lines[0][:4] == ["chrT", "300", "340", "other"] and lines[0][4:] == ["90", "130", "-", "anti", "40"]
    assert not list(tmp_path.glob("*.png")) and "dot plot(s) written" not in capsys.readouterr().out     # no -o: no image
    # without --versus: each repeat once, the trivial diagonal not at all
    seq = chrom[280:360] + "ACGTTA" + chrom[290:350]
    cli.main([seq, "--runs-tsv", str(tsv), "--min-run", "25", "--run-directions", "main", "-d", str(tmp_path)], context=ctx)
    assert tsv.read_text() == "sequence\t10\t70\tsequence\t86\t146\t+\tmain\t60\n" and ctx.calls[-1] == (146, 146, "+", "main", 25)
