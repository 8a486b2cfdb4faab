"""CPU: the list of chains on the period lines of one range (prf_period_chains, plot_periodicity_matrix.py
--chains-tsv).  The model (tests/periodchain_model.py: dotchain_model.all_chains on the band of the range's dot plot with itself) is
pinned to an independent brute force (every line as a string of 0 and 1, the seeds by a regular expression) on the 276 distinct
sequences of tests/golden/dotpair.jsonl.gz, with floors on the number of chains compared, and to the REFERENCE's rows on its own
fixtures: every row of the perfect scan is the maximal run of line k = len(motif) at its start.  The word source of the kernels
(csrc/periodchain_word.h) and the walks over it run on the host under the sanitizers (tests/periodchain_word_check.cpp).  The
refusals of the new entry points are decided before the context is looked at (NULL context, no GPU needed), in the documented order;
tandem_rows and the command line's arguments run on the host as well.  Every list is compared exactly."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import periodchain_model as M
from conftest import ROOT, load_jsonl_gz

PAIRS = [(1, 0), (2, 1), (3, 2), (4, 8), (8, 16)]             # (min_seed, max_gap)
KMAX = 64
# (chains, of them joined) of the model over the 276 sequences, k = 1 .. 64: {n_matches: {pair: ...}}
FLOORS = {1: {(1, 0): (206_096, 0), (2, 1): (57_502, 7_606), (3, 2): (22_729, 2_494), (4, 8): (9_618, 1_503), (8, 16): (1_754, 12)},
          0: {(1, 0): (197_550, 0), (2, 1): (51_732, 6_093), (3, 2): (18_475, 1_878), (4, 8): (7_171, 1_080), (8, 16): (1_150, 6)}}


def fixture_sequences():
    """The distinct sequences of the dot-plot fixture, in the order of their first appearance."""
    seen = {}
    for c in load_jsonl_gz("dotpair.jsonl.gz"):
        for s in (c["a"], c["b"]):
            seen.setdefault(s, None)
    return list(seen)


def brute(seq, n_matches, kmin, kmax, min_seed, max_gap):
    """Every chain, line by line: the line's cells as a string, the seeds as the matches of 1+ that are long enough."""
    s = seq.upper()
    n, rows = len(s), []
    for k in range(kmin, min(kmax, n - 1) + 1):
        text = "".join("1" if s[t] == s[t + k] and (n_matches or s[t] != "N") else "0" for t in range(n - k))
        chain = None                                            # [first cell, last cell, seeds]
        for m in list(re.finditer("1+", text)) + [None]:
            if m is not None and m.end() - m.start() < min_seed:
                continue
            if m is not None and chain is not None and m.start() - chain[1] - 1 <= max_gap:
                chain[1], chain[2] = m.end() - 1, chain[2] + 1
                continue
            if chain is not None:
                rows.append((chain[0], chain[1] - chain[0] + 1, text[chain[0]:chain[1] + 1].count("1"), k, chain[2]))
            chain = None if m is None else [m.start(), m.end() - 1, 1]
    return np.sort(np.array(rows, dtype=M.DTYPE), order=["start", "k"])


def test_model_agrees_with_a_brute_force_on_every_fixture_sequence():
    seqs = fixture_sequences()
    assert len(seqs) == 276 and sum("N" in s.upper() for s in seqs) == 119 and max(map(len, seqs)) == 195 and min(map(len, seqs)) == 0
    assert sum(bool(set(s.upper()) - set("ACGTN")) for s in seqs) == 54
    bad = []
    total = {nm: dict.fromkeys(PAIRS, 0) for nm in (0, 1)}
    joined = {nm: dict.fromkeys(PAIRS, 0) for nm in (0, 1)}
    for at, s in enumerate(seqs):
        for nm in (0, 1):
            raw = M.band_cells(s, nm, 1, KMAX)
            every = M.runs_of(raw)
            for pair in PAIRS:
                got = M.all_chains(raw, *pair, every)
                if not M.same(got, brute(s, nm, 1, KMAX, *pair)) or not M.same(got, M.line_chains(s, nm, 1, KMAX, *pair)):
                    bad.append((at, nm, pair))
                total[nm][pair] += len(got)
                joined[nm][pair] += int((got["seeds"] >= 2).sum())
    print(total, joined)
    assert not bad, f"{len(bad)} differ: {bad[:5]}"
    for nm in (0, 1):                                           # no vacuous pass
        for pair in PAIRS:
            assert total[nm][pair] >= FLOORS[nm][pair][0] and joined[nm][pair] >= FLOORS[nm][pair][1], (nm, pair, total[nm][pair], joined[nm][pair])


def test_model_windows_and_periods_add_up_and_ranges_are_cut_first():
    seqs = [s for s in fixture_sequences() if len(s) >= 120][:12]
    for s in seqs:
        n = len(s)
        whole = M.chains(s, 1, 40, 3, 2)
        parts = [M.chains(s, ka, kb, 3, 2, positions=pos) for ka, kb in ((1, 7), (8, 40)) for pos in ((0, 50), (50, 51), (51, n + 9))]
        assert M.same(np.sort(np.concatenate(parts), order=["start", "k"]), whole)
        assert M.same(M.chains(s, 1, 40, 3, 2, begin=17, end=101), M.chains(s[17:101], 1, 40, 3, 2))
        assert M.same(M.chains(s, 1, 40, 3, 2, min_len=9), whole[whole["len"] >= 9])
    # the start decides; the second seed lies outside the window and still counts
    seq = "ACGTACGTACTTACGTACGT"                                  # line 4: 1111 1101 1101 1111
    assert M.chains(seq, 4, 4, 4, 5, positions=(0, 1)).tolist() == [(0, 16, 14, 4, 2)]
    assert len(M.chains(seq, 4, 4, 4, 5, positions=(1, 20))) == 0
    assert M.chains(seq, 4, 4, 4, 4, positions=(1, 20)).tolist() == [(11, 5, 5, 4, 1)]


def _eligible(c):
    """Status ok, min_repeats >= 2, no interval: the whole sequence was scanned and a row is a run of at least k cells."""
    st = c["settings"]
    return c.get("status") == "ok" and st["min_repeats"] >= 2 and not any("interval" in key for key in list(st) + list(c))


def test_every_reference_row_is_the_maximal_run_of_its_line():
    """(start, end, motif) of the perfect scan = the run of line k = len(motif) that starts at `start`, end - start - k cells long,
    under "equal and not N": the list at max_gap = 0 holds the perfect scan's rows."""
    rows = cases = 0
    for c in load_jsonl_gz("fuzz_small.jsonl.gz") + load_jsonl_gz("adversarial.jsonl.gz") + load_jsonl_gz("iupac.jsonl.gz"):
        if not _eligible(c):
            continue
        cases += 1
        if not c["rows"]:
            continue
        s = c["seq"].upper()
        ks = sorted({len(m) for _, _, m in c["rows"]})
        runs = brute(s, 0, ks[0], ks[-1], 1, 0)
        have = {(a, k): n for a, n, _, k, _ in runs.tolist()}
        for start, end, motif in c["rows"]:
            k = len(motif)
            assert have.get((start, k)) == end - start - k, (c.get("tag"), start, end, motif)
            rows += 1
    assert rows == 9_277 and cases > 100


def test_the_model_itself_holds_the_reference_rows_on_the_short_cases():
    """The same invariant through the model proper (the n x n band), on the cases short enough for it."""
    rows = 0
    for c in load_jsonl_gz("adversarial.jsonl.gz") + load_jsonl_gz("iupac.jsonl.gz"):
        if not _eligible(c) or not c["rows"] or len(c["seq"]) > 400:
            continue
        ks = sorted({len(m) for _, _, m in c["rows"]})
        got = M.chains(c["seq"], ks[0], ks[-1], 1, 0)
        have = {(a, k): n for a, n, _, k, _ in got.tolist()}
        for start, end, motif in c["rows"]:
            assert have.get((start, len(motif))) == end - start - len(motif), (c.get("tag"), start, end, motif)
            rows += 1
    assert rows >= 20


# ---- the word source and the walks of the kernels, on the host ----

def test_word_source_and_walks_against_a_brute_force_on_the_host(tmp_path):
    """csrc/periodchain_word.h and csrc/dotchain_walk.h are the text the kernels run; the stand-alone program checks them on random
    and hand-made lines with both N rules, 3 and 8 planes, under the sanitizers."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/periodchain_word_check.cpp")
    exe = tmp_path / "word_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "periodchain_word_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, lines, chains, words, handed = done.stdout.split()
    assert word == "ok" and int(lines) == 1500 * 2 * 13 and int(chains) > 10_000 and int(words) > 100_000 and int(handed) > 10_000


# ---- tandem_rows ----

def _chains(*rows):
    import prf_native
    return np.array(list(rows), dtype=prf_native.PCHAIN_DTYPE)


def test_tandem_rows_fields_and_multiples():
    import prf_native as pn
    # a period-3 repeat over [100, 160) and its images at 6 and 9; a containing row with a non-multiple k; equal spans
    chains = _chains((100, 57, 55, 3, 2), (100, 54, 52, 6, 2), (100, 51, 49, 9, 2),
                     (90, 76, 70, 4, 3),             # [90, 170) at k = 4 holds [100, 160); 3 is no multiple of 4, 4 none of 3: both stay
                     (100, 56, 56, 4, 1),            # [100, 160) at k = 4: inside the k = 4 row above (no smaller period divides): stays
                     (100, 48, 48, 12, 1),           # [100, 160) at k = 12: a multiple of 3, 4 and 6 with equal span: dropped
                     (300, 20, 20, 5, 1), (300, 15, 15, 10, 1),      # equal spans [300, 325): the multiple goes
                     (301, 14, 14, 10, 1),           # [301, 325) at 10 inside [300, 325) at 5: dropped
                     (299, 16, 16, 10, 1),           # starts in front of the period-5 row: kept
                     (300, 16, 16, 10, 1))           # ends behind it: kept
    rows = pn.tandem_rows(chains, drop_multiples=False)
    assert rows.dtype == np.dtype(pn.TANDEM_DTYPE) and len(rows) == len(chains)
    assert rows["start"].tolist() == chains["start"].tolist() and rows["k"].tolist() == chains["k"].tolist()
    assert rows["end"].tolist() == [160, 160, 160, 170, 160, 160, 325, 325, 325, 325, 326]
    assert np.array_equal(rows["copies"], (chains["len"] + chains["k"]) / chains["k"]) and rows["copies"][0] == 20.0
    assert np.array_equal(rows["identity"], chains["matches"] / chains["len"]) and rows["identity"][3] == 70 / 76
    assert rows["matches"].tolist() == chains["matches"].tolist() and rows["seeds"].tolist() == chains["seeds"].tolist()
    kept = pn.tandem_rows(chains)
    assert [(r[0], r[1], r[2]) for r in kept.tolist()] == [(100, 160, 3), (90, 170, 4), (100, 160, 4), (300, 325, 5), (299, 325, 10), (300, 326, 10)]
    # brute force of the definition on a random list
    rng = np.random.default_rng(3)
    many = _chains(*[(int(a), int(n), int(n), int(k), 1) for a, n, k in zip(rng.integers(0, 60, 400), rng.integers(1, 40, 400), rng.integers(1, 13, 400))])
    many = np.unique(many)
    full = pn.tandem_rows(many, drop_multiples=False)
    want = [i for i, (a, b, k) in enumerate(zip(full["start"].tolist(), full["end"].tolist(), full["k"].tolist()))
            if not any(q < k and k % q == 0 and a2 <= a and b2 >= b for a2, b2, q in zip(full["start"].tolist(), full["end"].tolist(), full["k"].tolist()))]
    assert pn.tandem_rows(many).tolist() == full[want].tolist() and 0 < len(want) < len(full)
    assert len(pn.tandem_rows(_chains())) == 0 and len(pn.tandem_rows(chains[:1])) == 1


def test_tandem_rows_of_the_model_find_a_diverged_repeat_once():
    import prf_native as pn
    unit = "ACGGTCA"
    body = list(unit * 12)
    for at in (10, 31, 55, 70):                                 # substitutions at arbitrary places
        body[at] = "T" if body[at] != "T" else "G"
    seq = "CATTGCAGGCTTAACGTGCA" + "".join(body) + "TTGACCGATAGGCTAGCTTA"
    got = M.chains(seq, 1, 30, 5, 3)
    chains = np.zeros(len(got), dtype=pn.PCHAIN_DTYPE)
    for f in M.FIELDS:
        chains[f] = got[f]
    rows, full = pn.tandem_rows(chains), pn.tandem_rows(chains, drop_multiples=False)
    big = rows[(rows["k"] == 7) & (rows["end"] - rows["start"] >= 60)]                       # the repeat, one row
    assert len(big) == 1 and big["start"][0] <= 21 and big["end"][0] >= 102 and big["seeds"][0] >= 4 and 0.85 < big["identity"][0] < 1
    inside = lambda r: (r["k"] % 7 == 0) & (r["k"] > 7) & (r["start"] >= big["start"][0]) & (r["end"] <= big["end"][0])   # noqa: E731
    assert inside(full).sum() >= 2 and inside(rows).sum() == 0                            # its images at 14, 21, 28 were there


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_periodchain.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.PERIODCHAIN_EXPORTS) and len(declared) == 3
    older = (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS) |
             set(pn.DOTCHAIN_EXPORTS) | set(pn.DOTLINK_EXPORTS))
    assert not set(declared) & older
    assert open(os.path.join(ROOT, "include", "prf.h")).read().count('#include "prf_periodchain.h"') == 1
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4
    for name, value in (("PRF_PCHAIN_MAX_ROWS", pn.PCHAIN_MAX_ROWS), ("PRF_PCHAIN_LONG_ROWS", pn.PCHAIN_LONG_ROWS)):
        found = re.search(rf"#define {name} \((\d+)ull << (\d+)\)", text)
        assert found and int(found[1]) << int(found[2]) == value, name
    assert pn.PCHAIN_MAX_ROWS == 1 << 24
    assert np.dtype(pn.PCHAIN_DTYPE).itemsize == 32 and [n for n, _ in pn.PCHAIN_DTYPE] == list(M.FIELDS)
    struct = re.search(r"typedef struct prf_pchain \{(.*?)\} prf_pchain;", text, flags=re.S)[1]
    assert re.findall(r"\b(start|len|matches|k|seeds);", struct) == list(M.FIELDS)


def _call(lib, pn, form, seq=b"ACGTACGTACGT", span=(0, 12), pos=(0, 12), kmin=1, kmax=6, n_matches=0, min_seed=3, max_gap=2, min_len=0,
          capacity=64, dst=True, n_chains=True):
    buf = np.full(64 * 32, 0xAB, dtype=np.uint8)
    n, stats = ctypes.c_uint64(77), pn.ScanStats()
    tail = (*span, *pos, kmin, kmax, n_matches, min_seed, max_gap, min_len, buf.ctypes.data if dst else None, capacity,
            ctypes.byref(n) if n_chains else None, ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_period_chains_seq(None, arr, *tail)
    elif form == "ex":
        rc = lib.prf_period_chains_ex(None, None, 0, *tail, 4096)
    else:
        rc = lib.prf_period_chains(None, None, 0, *tail)
    assert (buf == 0xAB).all() and n.value == 77                              # a refused call writes nothing
    return rc


# each case breaks one rule and every rule behind it: the first in the documented order is the one reported
LATER = dict(pos=(5, 4), kmin=0, n_matches=2, min_seed=0, max_gap=4097, capacity=(1 << 24) + 1, dst=False, n_chains=False)


def _later(*fixed):
    return {k: v for k, v in LATER.items() if k not in fixed}


ORDER = [
    (dict(span=(7, 3), **LATER), "PRF_EINVAL", "begin 7"),
    (dict(LATER), "PRF_EINVAL", "pos0 5"),
    (_later("pos"), "PRF_EINVAL", "kmin is 0"),
    (dict(_later("pos", "kmin"), kmin=9, kmax=8), "PRF_EINVAL", "kmin 9 is above kmax 8"),
    (_later("pos", "kmin"), "PRF_EINVAL", "n_matches is 2"),
    (_later("pos", "kmin", "n_matches"), "PRF_EINVAL", "min_seed is 0"),
    (_later("pos", "kmin", "n_matches", "min_seed"), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (_later("pos", "kmin", "n_matches", "min_seed", "max_gap"), "PRF_EUNSUPPORTED", "PRF_PCHAIN_MAX_ROWS"),
    (dict(dst=False, n_chains=False), "PRF_EINVAL", "NULL n_chains"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(dst=False, capacity=0), "PRF_EINVAL", "NULL context"),              # counting only is a valid call
    (dict(n_matches=0xFFFFFFFF), "PRF_EINVAL", "n_matches"),
    (dict(max_gap=0xFFFFFFFF), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(n_matches=1, min_len=1 << 40, max_gap=4096, min_seed=1 << 40, capacity=1 << 24), "PRF_EINVAL", "NULL context"),
    (dict(kmin=500, kmax=0xFFFFFFFF, pos=(3, 3), span=(4, 4)), "PRF_EINVAL", "NULL context"),   # empty lines and an empty window are no error
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_period_chains")


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(seq=b""), "PRF_EINVAL", "NULL context"),                            # an empty sequence
    (dict(span=(2, 1 << 63), pos=(1, 1 << 63)), "PRF_EINVAL", "NULL context"),   # ends are clipped
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


def test_a_missing_sequence_and_a_window_above_the_limit_are_refused():
    pn, lib = _lib()
    n, stats = ctypes.c_uint64(0), pn.ScanStats()
    rc = lib.prf_period_chains_seq(None, None, 0, 4, 0, 4, 1, 2, 0, 3, 1, 0, None, 0, ctypes.byref(n), ctypes.byref(stats))
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()
    big = (pn._Contig * 1)()                                                  # judged from the lengths, the sequence is never read
    block = ctypes.create_string_buffer(16)
    big[0].ascii, big[0].len = ctypes.addressof(block), 1 << 32
    rc = lib.prf_period_chains_seq(None, big, 0, 1 << 32, 0, 1 << 32, 1, 1025, 0, 12, 8, 0, None, 0, ctypes.byref(n), ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()
    # the window counts, not the range: 2^20 starts x 1025 lines pass this check (and the bytes are looked at next)
    rc = lib.prf_period_chains_seq(None, big, 0, 1 << 32, 5, 5 + (1 << 20), 1, 1025, 0, 12, 8, 0, None, 0, ctypes.byref(n), ctypes.byref(stats))
    assert rc == pn.PRF_ESYMBOL


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 2, [100, 50])
    with pytest.raises(ValueError, match="contig 2"):
        g.period_chains(2, 0, None, 1, 6, 4, 2)
    with pytest.raises(ValueError, match="periods"):
        g.period_chains(0, 0, None, 0, 6, 4, 2)
    with pytest.raises(ValueError, match="periods"):
        g.period_chains(0, 0, None, 7, 6, 4, 2)
    with pytest.raises(ValueError, match="min_seed"):
        g.period_chains(0, 0, None, 1, 6, 0, 2)
    with pytest.raises(ValueError, match="max_gap"):
        g.period_chains(0, 0, None, 1, 6, 4, 4097)
    with pytest.raises(ValueError, match="max_gap"):
        g.period_chains(0, 0, None, 1, 6, 4, -1)
    with pytest.raises(ValueError, match="min_len"):
        g.period_chains(0, 0, None, 1, 6, 4, 1, min_len=-1)
    with pytest.raises(ValueError, match="positions"):
        g.period_chains(0, 0, None, 1, 6, 4, 1, positions=(5, 4))
    with pytest.raises(ValueError, match="begin"):
        g.period_chains(0, 30, 20, 1, 6, 4, 1)
    g._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_input(args, parser), args


def test_cli_parses_the_chains_options(tmp_path, capsys):
    import plot_periodicity_matrix as cli
    (chrom, seq, begin, end), args = _parse(cli, ["ACGTACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2"])
    assert (chrom, seq, begin, end) == ("sequence", "ACGTACGT", 0, 8)
    assert (args.chains_tsv, args.min_seed, args.max_gap, args.min_chain, args.min_identity, args.keep_multiples, args.n_matches,
            args.chain_window) == ("c.tsv", 4, 2, 0, 0.0, False, False, 1 << 22)
    args = _parse(cli, ["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "1", "--max-gap", "0", "--min-chain", "30", "--min-identity", "0.9",
                        "--keep-multiples", "--n-matches", "--chain-window", "1000"])[1]
    assert (args.min_chain, args.min_identity, args.keep_multiples, args.n_matches, args.chain_window) == (30, 0.9, True, True, 1000)
    # nothing changes for a command line without the new options
    (_, seq, _, _), args = _parse(cli, ["ACGTACGT", "--max-motif-size", "4"])
    assert seq == "ACGTACGT" and args.chains_tsv is None and args.window is None and args.output_path == "periodicity_matrix.png"
    # above 5 000 positions the list needs no --window
    long_fa = tmp_path / "x.fa"
    long_fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    (chrom, seq, begin, end), _ = _parse(cli, [str(long_fa), "-i", "chrA:100-7100", "--chains-tsv", "c.tsv", "--min-seed", "12", "--max-gap", "8"])
    assert (chrom, len(seq), begin, end) == ("chrA", 8000, 100, 7100)
    capsys.readouterr()
    base = ["ACGT", "--chains-tsv", "c.tsv"]
    for argv, text in ((base, "--min-seed"), (base + ["--min-seed", "4"], "--max-gap"), (base + ["--max-gap", "4"], "--min-seed"),
                       (["ACGT", "--min-seed", "5"], "--chains-tsv"), (["ACGT", "--max-gap", "5"], "--chains-tsv"),
                       (base + ["--min-seed", "0", "--max-gap", "1"], "at least 1"),
                       (base + ["--min-seed", "3", "--max-gap", "4097"], "0 .. 4096"),
                       (base + ["--min-seed", "3", "--max-gap", "-1"], "0 .. 4096"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--min-chain", "-2"], "at least 0"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--min-identity", "1.5"], "0 .. 1"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--chain-window", "0"], "at least 1"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--window", "64"], "belong to the profile"),
                       (base + ["--min-seed", "3", "--max-gap", "1", "--min-motif-size", "0"], "at least 1"),
                       ([str(long_fa), "-i", "chrA:0-7000"], "--window")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_chain_lines_are_in_genomic_coordinates():
    import plot_periodicity_matrix as cli
    import prf_native as pn
    seq = "ttttttttttacgacgacgacgatacgtttt"
    rows = pn.tandem_rows(_chains((2, 11, 10, 3, 2), (0, 4, 4, 1, 1)))
    assert list(cli.chain_lines("chr1", 8, seq, rows)) == ["chr1\t10\t24\t3\t4.667\t0.9091\t10\t2\tACG\n", "chr1\t8\t13\t1\t5.000\t1.0000\t4\t1\tT\n"]
