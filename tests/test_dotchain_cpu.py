"""CPU: the list of chained diagonal runs of the dot plot of two ranges (prf_dotpair_chains, plot_dot_plot.py
--chains-tsv).  The model (tests/dotchain_model.py: the runs of dotruns_model, grouped, linked, prefix sums) is pinned to an
independent brute force (every line as a string of 0 and 1, the seeds by a regular expression) on every case of
tests/golden/dotpair.jsonl.gz; the walks of the kernels (csrc/dotchain_walk.h) run on the host against a third brute force
(tests/dotchain_walk_check.cpp).  The refusals of the new entry points are decided before the context is looked at (NULL context,
no GPU needed), in the documented order; unique_chains, chain_identity and the command line run on the host as well.  Every list
is compared exactly."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import dotchain_model as C
import dotpair_model as P
import dotruns_model as R
from conftest import ROOT, load_jsonl_gz

PAIRS = [(1, 0), (2, 1), (3, 2), (4, 8), (8, 16)]             # (min_seed, max_gap)


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("dotpair.jsonl.gz")


@pytest.fixture(scope="module")
def modelled(golden):
    """{(case index, min_seed, max_gap): every chain of the case, sorted}, computed once."""
    out = {}
    for k, c in enumerate(golden):
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        every = R.all_runs(raw)
        for min_seed, max_gap in PAIRS:
            out[k, min_seed, max_gap] = C.select(C.all_chains(raw, min_seed, max_gap, every), *raw.shape)
    return out


def _brute(raw, min_seed, max_gap):
    """Every chain, line by line: the line's cells as a string, the seeds as the matches of 1+ that are long enough."""
    na, nb = raw.shape
    found = []
    for d in (R.MAIN, R.ANTI):
        starts = [(0, j) for j in range(nb)] + [(i, 0 if d == R.MAIN else nb - 1) for i in range(1, na)]
        for i0, j0 in starts:
            dj = 1 if d == R.MAIN else -1
            n = min(na - i0, nb - j0 if d == R.MAIN else j0 + 1)
            text = "".join("1" if raw[i0 + t, j0 + dj * t] else "0" for t in range(n))
            chain = None                                        # [first cell, last cell, seeds]
            for m in re.finditer("1+", text):
                if m.end() - m.start() < min_seed:
                    continue
                if chain is not None and m.start() - chain[1] - 1 <= max_gap:
                    chain[1], chain[2] = m.end() - 1, chain[2] + 1
                    continue
                if chain is not None:
                    found.append((i0, j0, dj, d, text, *chain))
                chain = [m.start(), m.end() - 1, 1]
            if chain is not None:
                found.append((i0, j0, dj, d, text, *chain))
    rows = [(i0 + s, j0 + dj * s, e - s + 1, text[s:e + 1].count("1"), d, seeds) for i0, j0, dj, d, text, s, e, seeds in found]
    return np.sort(np.array(rows, dtype=C.DTYPE), order=["row", "col", "dir"])


def test_model_agrees_with_a_brute_force_on_every_fixture_case(golden, modelled):
    assert len(golden) == 159
    bad, total, joined, cases_joined = [], dict.fromkeys(PAIRS, 0), dict.fromkeys(PAIRS, 0), dict.fromkeys(PAIRS, 0)
    for k, c in enumerate(golden):
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        for pair in PAIRS:
            got = modelled[(k, *pair)]
            if not C.same(got, _brute(raw, *pair)):
                bad.append((c["tag"], pair))
            total[pair] += len(got)
            joined[pair] += int((got["seeds"] >= 2).sum())
            cases_joined[pair] += bool((got["seeds"] >= 2).any())
    print({pair: (total[pair], joined[pair], cases_joined[pair]) for pair in PAIRS})
    assert not bad, f"{len(bad)} differ: {bad[:5]}"
    assert joined[(1, 0)] == 0
    for pair in ((2, 1), (3, 2), (4, 8)):                      # no vacuous pass: chains of two and more seeds are compared
        assert joined[pair] >= 1000, (pair, joined[pair])
    assert joined[(8, 16)] >= 1


def test_consequences_of_the_definition(golden, modelled):
    for k, c in enumerate(golden):
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        every = R.all_runs(raw)
        na, nb = raw.shape
        for min_seed, max_gap in PAIRS + [(3, 0), (5, 0)]:
            chains = modelled[k, min_seed, max_gap] if max_gap else C.select(C.all_chains(raw, min_seed, 0, every), na, nb)
            runs = R.select(every, na, nb, min_len=min_seed)
            if max_gap == 0:                                    # the list of runs, with matches = len and seeds = 1
                for min_len in (0, min_seed + 2):
                    want = R.select(every, na, nb, min_len=max(min_seed, min_len))
                    got = chains[chains["len"] >= min_len]
                    assert R.same(got, want) and (got["matches"] == got["len"]).all() and (got["seeds"] == 1).all(), c["tag"]
            assert int(chains["seeds"].sum()) == len(runs), c["tag"]
            assert (chains["matches"] >= chains["seeds"].astype(np.uint64) * min_seed).all()
            assert (chains["len"] - chains["matches"] <= (chains["seeds"].astype(np.uint64) - 1) * max_gap).all()
        # the seeds of all chains are exactly the runs: walk the chains of one pair and collect the seeds cell by cell
        min_seed, max_gap = 3, 2
        seeds = set()
        for i, j, n, _m, d, _s in modelled[k, min_seed, max_gap].tolist():
            dj = 1 if d == R.MAIN else -1
            text = "".join("1" if raw[i + t, j + dj * t] else "0" for t in range(n))
            seeds |= {(i + m.start(), j + dj * m.start(), m.end() - m.start(), d) for m in re.finditer("1+", text) if m.end() - m.start() >= min_seed}
        assert seeds == {tuple(r) for r in R.select(every, na, nb, min_len=min_seed).tolist()}, c["tag"]


def test_model_windows_add_up_to_the_whole_list(golden, modelled):
    rng = random.Random(12)
    for k, c in list(enumerate(golden))[::3]:
        na, nb = len(c["a"]), len(c["b"])
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        every = C.all_chains(raw, 3, 2)
        r, q = rng.randrange(0, na + 1), rng.randrange(0, nb + 1)
        parts = [C.select(every, na, nb, rows, cols) for rows in ((0, r), (r, na + 7)) for cols in ((0, q), (q, None))]
        assert C.same(np.sort(np.concatenate(parts), order=["row", "col", "dir"]), modelled[k, 3, 2]), c["tag"]
    # the start decides; the second seed lies outside the window and still counts
    one = C.chains("ACGTACGTTACGTACGT", "ACGTACGTGACGTACGT", "+", 4, 1, rows=(0, 1), cols=(0, 1), directions="main")
    assert one.tolist() == [(0, 0, 17, 16, R.MAIN, 2)]
    assert len(C.chains("ACGTACGTTACGTACGT", "ACGTACGTGACGTACGT", "+", 4, 1, rows=(9, 10), cols=(9, 10), directions="main")) == 0
    assert C.chains("ACGTACGTTACGTACGT", "ACGTACGTGACGTACGT", "+", 4, 0, rows=(9, 10), cols=(9, 10), directions="main").tolist() == [(9, 9, 8, 8, R.MAIN, 1)]


def _brute_unique(chains, strand):
    """One chain of every mirror pair, by pairing the chains through their end cells."""
    spans = {}
    for i, j, n, m, d, s in chains.tolist():
        dj = 1 if d == R.MAIN else -1
        spans[(i, j, n, m, d, s)] = frozenset(((i, j), (i + n - 1, j + dj * (n - 1)))), d
    by_span = {v: k for k, v in spans.items()}
    keep = []
    for chain, (ends, d) in spans.items():
        mirror = by_span[frozenset((y, x) for x, y in ends), d]   # raw is symmetric: the mirror image is a chain too
        assert mirror[2:] == chain[2:]                            # ... of equal len, matches, dir and seeds
        i, j = chain[:2]
        if mirror == chain:
            if not (d == R.MAIN and strand == "+"):
                keep.append(chain)
        elif (d == R.MAIN and j > i) or (d == R.ANTI and chain < mirror):
            keep.append(chain)
    return sorted(keep, key=lambda r: (r[0], r[1], r[4]))


def _mutated(piece, every, rng):
    """piece with every `every`-th base changed."""
    out = list(piece)
    for at in range(every - 1, len(out), every):
        out[at] = rng.choice([x for x in "ACGT" if x != out[at]])
    return "".join(out)


def test_unique_chains_against_a_brute_force_pairing():
    import prf_native
    rng = random.Random(5)
    noise = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    u = noise(60)
    palindrome = "ACCTGAATGCATTCAGGT"
    assert P.revcomp(palindrome.encode()).decode() == palindrome
    broken = palindrome[:4] + "T" + palindrome[5:]          # one base changed: cells 4 and 13 of its anti-diagonal, mirror images of each other
    seq = noise(30) + u + noise(25) + _mutated(u, 9, rng) + noise(19) + P.revcomp(_mutated(u, 11, rng).encode()).decode() + noise(21) + broken + noise(17) + "NNSW"
    n = len(seq)
    for strand in "+-":
        chains = C.chains(seq, seq, strand, 4, 2)
        got = prf_native.unique_chains(chains, strand)
        assert [tuple(r) for r in got.tolist()] == _brute_unique(chains, strand), strand
        assert 2 * len(got) >= len(chains) - 1 and len(got) < len(chains)
        identity = prf_native.chain_identity(got)
        assert identity.dtype == np.float64 and np.array_equal(identity, got["matches"] / got["len"])
        if strand == "+":
            assert not ((got["row"] == got["col"]) & (got["dir"] == R.MAIN)).any()
            copy = [r for r in got.tolist() if r[4] == R.MAIN and r[1] - r[0] == 85 and r[2] >= 56]
            assert len(copy) == 1 and copy[0][5] >= 6 and 50 <= copy[0][3] < copy[0][2]          # the diverged direct copy, one line
        else:
            inverted = [r for r in got.tolist() if r[4] == R.ANTI and r[2] >= 56 and r[5] >= 5]
            assert inverted and all(r[3] < r[2] for r in inverted)                              # the diverged inverted copy
            at = seq.index(broken)
            own = [r for r in got.tolist() if r[4] == R.ANTI and r[0] == at and r[0] == r[1] - r[2] + 1]
            assert len(own) == 1 and own[0][2:4] == (18, 16) and own[0][5] == 3                   # the palindrome with a mismatch stays, once
    assert len(prf_native.unique_chains(np.zeros(0, dtype=prf_native.DOTCHAIN_DTYPE))) == 0
    assert len(prf_native.chain_identity(np.zeros(0, dtype=prf_native.DOTCHAIN_DTYPE))) == 0


# ---- the walks of the kernels, on the host ----

def test_walks_of_the_kernels_against_a_brute_force_on_the_host(tmp_path):
    """csrc/dotchain_walk.h is the text the kernels run; the stand-alone program checks it on random lines, under the sanitizers."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/dotchain_walk_check.cpp")
    exe = tmp_path / "walk_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "dotchain_walk_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, lines, chains, handed = done.stdout.split()
    assert word == "ok" and int(lines) == 6000 and int(chains) > 10_000 and int(handed) > 10_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_dotchain.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.DOTCHAIN_EXPORTS) and len(declared) == 3
    assert not set(declared) & (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS))
    assert '#include "prf_dotchain.h"' in open(os.path.join(ROOT, "include", "prf.h")).read()
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4
    for name, value in (("PRF_DOTCHAIN_MAX_GAP", pn.DOTCHAIN_MAX_GAP), ("PRF_DOTCHAIN_MAX_ROWS", pn.DOTCHAIN_MAX_ROWS),
                        ("PRF_DOTCHAIN_LONG_ROWS", pn.DOTCHAIN_LONG_ROWS), ("PRF_DOTCHAIN_FOLLOW", pn.DOTCHAIN_FOLLOW)):
        found = re.search(rf"#define {name} \(?(?:(\d+)ull << (\d+)|(\d+)u)\)?", text)
        assert found and (int(found[1]) << int(found[2]) if found[1] else int(found[3])) == value, name
    assert pn.DOTCHAIN_MAX_GAP == 4096 and pn.DOTCHAIN_FOLLOW % 64 == 0
    assert np.dtype(pn.DOTCHAIN_DTYPE).itemsize == 40 and [n for n, _ in pn.DOTCHAIN_DTYPE] == list(C.FIELDS)
    struct = re.search(r"typedef struct prf_dotchain \{(.*?)\} prf_dotchain;", text, flags=re.S)[1]
    assert re.findall(r"\b(row|col|len|matches|dir|seeds)\b", struct) == list(C.FIELDS)


def _call(lib, pn, form, seq_a=b"ACGTACGTAC", seq_b=b"ACGTACGTACGT", a=(0, 10), b=(0, 12), strand=0, rows=(0, 10), cols=(0, 12),
          directions=3, min_seed=3, max_gap=2, min_len=0, capacity=64, dst=True, n_chains=True):
    buf = np.full(64, 0xAB, dtype=np.uint8).repeat(40)
    n, stats = ctypes.c_uint64(77), pn.ScanStats()
    tail = (strand, rows[0], rows[1], cols[0], cols[1], directions, min_seed, max_gap, min_len, buf.ctypes.data if dst else None, capacity,
            ctypes.byref(n) if n_chains else None, ctypes.byref(stats))
    if form == "one_shot":
        arr_a, _keep_a = pn._contig_array([seq_a])
        arr_b, _keep_b = pn._contig_array([seq_b])
        rc = lib.prf_dotpair_chains_seq(None, arr_a, *a, arr_b, *b, *tail)
    elif form == "ex":
        rc = lib.prf_dotpair_chains_ex(None, None, 0, *a, 1, *b, *tail, 4096)
    else:
        rc = lib.prf_dotpair_chains(None, None, 0, *a, 1, *b, *tail)
    assert (buf == 0xAB).all() and n.value == 77                              # a refused call writes nothing
    return rc


# each case breaks one rule and every rule behind it: the first in the documented order is the one reported
LATER = dict(rows=(5, 4), cols=(9, 2), strand=2, directions=4, min_seed=0, max_gap=4097, capacity=(1 << 24) + 1, dst=False, n_chains=False)


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
    (_later("rows", "cols", "strand", "directions"), "PRF_EINVAL", "min_seed is 0"),
    (_later("rows", "cols", "strand", "directions", "min_seed"), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (_later("rows", "cols", "strand", "directions", "min_seed", "max_gap"), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_ROWS"),
    (dict(dst=False, n_chains=False), "PRF_EINVAL", "NULL n_chains"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(dst=False, capacity=0), "PRF_EINVAL", "NULL context"),              # counting only is a valid call
    (dict(strand=0xFFFFFFFF), "PRF_EINVAL", "strand"),
    (dict(max_gap=0xFFFFFFFF), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(min_len=0, max_gap=4096, min_seed=1 << 40, capacity=1 << 24), "PRF_EINVAL", "NULL context"),   # min_len 0: no filter
    (dict(strand=1, directions=1, min_len=1 << 40, max_gap=0), "PRF_EINVAL", "NULL context"),
    (dict(directions=2, rows=(3, 3), a=(4, 4)), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_dotpair_chains")


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
        rc = lib.prf_dotpair_chains_seq(None, first, 0, 4, second, 0, 4, 0, 0, 4, 0, 4, 3, 2, 1, 0, None, 0, ctypes.byref(n), ctypes.byref(stats))
        assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()
    big = (pn._Contig * 1)()                                                  # 2^44 cells: judged from the lengths, the sequences are never read
    block = ctypes.create_string_buffer(16)
    big[0].ascii, big[0].len = ctypes.addressof(block), 1 << 22
    rc = lib.prf_dotpair_chains_seq(None, big, 0, 1 << 22, big, 0, 1 << 22, 1, 0, 1 << 22, 0, 1 << 22, 3, 64, 8, 0, None, 0, ctypes.byref(n),
                                    ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g, other = pn.Genome(None, None, 2, [100, 50]), pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="contig 2"):
        g.dotpair_chains((0, 0, None), (2, 0, None), min_seed=4, max_gap=2)
    with pytest.raises(ValueError, match="strand"):
        g.dotpair_chains((0, 0, None), (1, 0, None), strand="x")
    with pytest.raises(ValueError, match="directions"):
        g.dotpair_chains((0, 0, None), (1, 0, None), directions="up")
    with pytest.raises(ValueError, match="min_seed"):
        g.dotpair_chains((0, 0, None), (1, 0, None), min_seed=0)
    with pytest.raises(ValueError, match="max_gap"):
        g.dotpair_chains((0, 0, None), (1, 0, None), min_seed=4, max_gap=4097)
    with pytest.raises(ValueError, match="max_gap"):
        g.dotpair_chains((0, 0, None), (1, 0, None), min_seed=4, max_gap=-1)
    with pytest.raises(ValueError, match="min_len"):
        g.dotpair_chains((0, 0, None), (1, 0, None), min_seed=4, max_gap=1, min_len=-1)
    with pytest.raises(ValueError, match="cols"):
        g.dotpair_chains((0, 0, None), (1, 0, None), cols=(5, 4))
    with pytest.raises(ValueError, match="same resident genome"):
        pn._chains(None, (g, 0), (0, None), (other, 0), (0, None), "+", "both", 3, 1, 0, None, None, False, 0)
    with pytest.raises(ValueError, match="both be sequences or both"):
        pn._chains(None, (g, 0), (0, None), "ACGT", (0, None), "+", "both", 3, 1, 0, None, None, False, 0)
    g._h = other._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_inputs(args, parser), cli.resolve_versus(args, parser), args


def test_cli_parses_the_chains_options(tmp_path, capsys):
    import plot_dot_plot as cli
    out, versus, args = _parse(cli, ["ACGTACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2"])
    assert (args.chains_tsv, args.min_seed, args.max_gap, args.min_chain, args.min_identity, args.run_directions) == ("c.tsv", 4, 2, None, None, "both")
    assert cli.no_image(args) and args.runs_tsv is None
    args = _parse(cli, ["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "1", "--max-gap", "0", "--min-chain", "30", "--min-identity", "0.9",
                        "--run-directions", "anti"])[2]
    assert (args.min_chain, args.min_identity, args.run_directions) == (30, 0.9, "anti")
    assert not cli.no_image(_parse(cli, ["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "9", "--max-gap", "4096", "-o", "x.png"])[2])
    # nothing changes for a command line without the new options
    out, _, args = _parse(cli, ["ACGTACGT", "-d", str(tmp_path)])
    assert out == [("sequence", 0, "ACGTACGT", str(tmp_path / "dot_plot.png"))] and args.chains_tsv is None and not cli.no_image(args)
    assert cli.no_image(_parse(cli, ["ACGT", "--runs-tsv", "r.tsv", "--min-run", "4"])[2])
    # above 5 000 positions the list needs no --block when no image is asked for
    long_fa = tmp_path / "x.fa"
    long_fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    out, versus, _ = _parse(cli, ["-R", str(long_fa), "chrA:100-7100", "--versus", "chrA:500-6500", "--chains-tsv", "c.tsv", "--min-seed", "12",
                                  "--max-gap", "8"])
    assert len(out[0][2]) == 7000 and versus[:2] == ("chrA", 500) and len(versus[2]) == 6000
    capsys.readouterr()
    base = ["ACGT", "--chains-tsv", "c.tsv"]
    for argv, text in ((base, "--min-seed"), (base + ["--min-seed", "4"], "--max-gap"), (base + ["--max-gap", "4"], "--min-seed"),
                       (["ACGT", "--min-seed", "5"], "--chains-tsv"), (["ACGT", "--max-gap", "5"], "--chains-tsv"),
                       (["ACGT", "--min-chain", "5"], "--chains-tsv"), (["ACGT", "--min-identity", "0.5"], "--chains-tsv"),
                       (base + ["--min-seed", "0", "--max-gap", "1"], "at least 1"),
                       (base + ["--min-seed", "3", "--max-gap", "4097"], "between 0 and 4096"),
                       (base + ["--min-seed", "3", "--max-gap", "-1"], "between 0 and 4096"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--min-chain", "-2"], "at least 0"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--min-identity", "1.5"], "between 0 and 1"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--run-directions", "up"], "invalid choice"),
                       (["ACGT", "TTGA", "--chains-tsv", "c.tsv", "--min-seed", "3", "--max-gap", "1"], "takes one input"),
                       (["-R", str(long_fa), "chrA:0-7000", "--chains-tsv", "c.tsv", "--min-seed", "30", "--max-gap", "1", "-o", "x.png"], "--block")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_chain_lines_are_in_genomic_coordinates():
    import plot_dot_plot as cli
    import prf_native
    chains = np.array([(5, 9, 40, 37, 1, 3), (5, 9, 3, 3, 2, 1), (0, 0, 7, 6, 2, 2)], dtype=prf_native.DOTCHAIN_DTYPE)
    assert list(cli.chain_lines("chr1", 100, "chrX", 1000, "-", chains)) == [
        "chr1\t105\t145\tchrX\t1009\t1049\t-\tmain\t40\t37\t3\t0.9250\n",
        "chr1\t105\t108\tchrX\t1007\t1010\t-\tanti\t3\t3\t1\t1.0000\n",
        "chr1\t100\t107\tchrX\t994\t1001\t-\tanti\t7\t6\t2\t0.8571\n"]


class _StubContext:
    """Serves dotpair_chains from the model, so that the command line's path runs without a GPU."""

    def __init__(self):
        self.calls = []

    def dotpair_chains(self, seq_a, seq_b, strand="+", directions="both", min_seed=16, max_gap=0, min_len=0):
        import prf_native
        self.calls.append((len(seq_a), len(seq_b), strand, directions, min_seed, max_gap, min_len))
        got = C.chains(seq_a, seq_b, strand, min_seed, max_gap, min_len, directions=directions)
        out = np.zeros(len(got), dtype=prf_native.DOTCHAIN_DTYPE)
        for f in C.FIELDS:
            out[f] = got[f]
        return out


def test_cli_writes_the_chains_of_a_stubbed_list(tmp_path, capsys):
    import plot_dot_plot as cli
    rng = random.Random(9)
    noise = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    u = noise(60)
    v = u[:20] + ("A" if u[20] != "A" else "C") + u[21:41] + ("G" if u[41] != "G" else "T") + u[42:]       # two changed bases: three runs of 20, 20, 18
    # the letters next to the copies are chosen so that chance lengthens none of them: A and C are not complements of themselves
    chrom = noise(289) + "C" + noise(9) + "A" + u + "C" + noise(139)
    other = noise(69) + "C" + P.revcomp(v.encode()).decode() + "A" + noise(69)
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + chrom + "\n")
    tsv, ctx = tmp_path / "chains.tsv", _StubContext()
    common = ["-R", str(fa), "chrT:250-400", "--versus", "other:50-200", "--strand", "both", "--chains-tsv", str(tsv), "-d", str(tmp_path)]
    cli.main(common + ["--min-seed", "15", "--max-gap", "1"], context=ctx)
    assert ctx.calls == [(150, 150, "+", "both", 15, 1, 0), (150, 150, "-", "both", 15, 1, 0)]
    lines = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert lines == [["chrT", "300", "360", "other", "70", "130", "-", "anti", "60", "58", "3", "0.9667"]]
    assert not list(tmp_path.glob("*.png")) and "dot plot(s) written" not in capsys.readouterr().out     # no -o: no image
    cli.main(common + ["--min-seed", "15", "--max-gap", "0", "--min-chain", "19"], context=ctx)            # unjoined: the runs of 20
    assert [line.split("\t")[8:] for line in tsv.read_text().splitlines()] == [["20", "20", "1", "1.0000"]] * 2 and ctx.calls[-1][4:] == (15, 0, 19)
    cli.main(common + ["--min-seed", "15", "--max-gap", "1", "--min-identity", "0.97"], context=ctx)       # filtered on the host
    assert tsv.read_text() == "" and ctx.calls[-1][4:] == (15, 1, 0)
    # without --versus: each repeat once, the trivial diagonal not at all
    seq = chrom[280:370] + "ACGTTC" + v      # A in front of u, C in front of v: chance lengthens nothing
    cli.main([seq, "--chains-tsv", str(tsv), "--min-seed", "15", "--max-gap", "1", "--run-directions", "main", "-d", str(tmp_path)], context=ctx)
    assert tsv.read_text() == "sequence\t20\t80\tsequence\t96\t156\t+\tmain\t60\t58\t3\t0.9667\n" and ctx.calls[-1] == (156, 156, "+", "main", 15, 1, 0)
