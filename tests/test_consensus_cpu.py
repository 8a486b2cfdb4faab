"""The consensus motifs of tandem repeats (include/prf_consensus.h) without a GPU: the CPU model against an independent
brute force, the fact that ties the product to the reference's rows, the host helpers, the C ABI and its refusals (no context is
needed to be refused), the binding's argument checks, the command line, and the per-lane text of the kernels on the host under
the sanitizers."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import consensus_model as M
from conftest import ROOT, load_jsonl_gz


def fixture_sequences():
    """The distinct sequences of the dot-plot fixture, in the order of their first appearance."""
    seen = {}
    for c in load_jsonl_gz("dotpair.jsonl.gz"):
        for s in (c["a"], c["b"]):
            seen.setdefault(s, None)
    return list(seen)


def brute(seq, start, end, k):
    """(motif, agree, acgt, counts) position by position: no slicing, no argmax."""
    counts = [[0, 0, 0, 0] for _ in range(k)]
    for q in range(start, end):
        letter = seq[q].upper()
        if letter in "ACGT":
            counts[(q - start) % k]["ACGT".index(letter)] += 1
    motif, agree = "", 0
    for column in counts:
        most = max(column)
        agree += most
        motif += "N" if most == 0 else [b for b, c in zip("ACGT", column) if c == most][0]
    return motif, agree, sum(map(sum, counts)), counts


def test_model_agrees_with_a_brute_force_on_every_fixture_sequence():
    seqs = fixture_sequences()
    assert len(seqs) == 276
    rng = random.Random(18)
    compared = tied = empty = 0
    for s in seqs:
        if not s:
            continue
        rows = []
        for _ in range(24):
            start = rng.randrange(len(s))
            rows.append((start, rng.randint(start + 1, len(s)), rng.randint(1, 64)))
        rows += [(0, len(s), 1), (0, len(s), 64), (len(s) - 1, len(s), 3)]
        got, motifs, counts = M.consensus(s, M.repeats(*rows))
        assert counts.shape == (sum(k for _, _, k in rows), 4)
        for (start, end, k), row, motif in zip(rows, got.tolist(), motifs):
            want = brute(s, start, end, k)
            offset = row[0]
            assert (motif, row[1], row[2], row[3], row[4]) == (want[0], want[1], want[2], k, 0), (s, start, end, k)
            assert counts[offset:offset + k].tolist() == want[3]
            compared += 1
            tied += any(sorted(c)[-1] == sorted(c)[-2] > 0 for c in want[3])
            empty += "N" in motif
        assert got["offset"].tolist() == np.concatenate([[0], np.cumsum(got["k"][:-1])]).tolist()
    print(compared, tied, empty)
    assert compared == 275 * 27 and tied >= 1_000 and empty >= 1_000           # 275 sequences hold a position; no vacuous pass


def _eligible(c):
    """Status ok, min_repeats >= 2, no interval: as tests/test_periodchain_cpu.py has it."""
    st = c["settings"]
    return c.get("status") == "ok" and st["min_repeats"] >= 2 and not any("interval" in key for key in list(st) + list(c))


def reference_rows():
    """(sequence, rows (start, end, motif) whose motif is all ACGT) of every eligible case, and the number of the other rows."""
    cases, other = [], 0
    for c in load_jsonl_gz("fuzz_small.jsonl.gz") + load_jsonl_gz("adversarial.jsonl.gz") + load_jsonl_gz("iupac.jsonl.gz"):
        if not _eligible(c) or not c["rows"]:
            continue
        plain = [(a, b, m) for a, b, m in c["rows"] if not set(m.upper()) - set("ACGT")]
        other += len(c["rows"]) - len(plain)
        if plain:
            cases.append((c["seq"], plain))
    return cases, other


def test_every_reference_row_is_its_own_consensus():
    """A perfect repeat is the consensus of itself: consensus == motif and agree == end - start at k = len(motif), for every
    reference row whose motif is all ACGT."""
    cases, other = reference_rows()
    rows = 0
    for seq, plain in cases:
        got, motifs, _ = M.consensus(seq, M.repeats(*[(a, b, len(m)) for a, b, m in plain]))
        for (a, b, m), row, motif in zip(plain, got.tolist(), motifs):
            assert motif == m.upper() and row[1] == b - a == row[2], (seq, a, b, m)
            rows += 1
    assert rows == 8_718 and other == 559


def test_ties_empty_columns_n_lower_case_and_iupac():
    one = lambda seq, *row: M.consensus(seq, M.repeats(row))                   # noqa: E731
    # ties go to the first of A, C, G, T
    assert one("ACCA", 0, 4, 1)[1] == ["A"] and one("CAAC", 0, 4, 1)[1] == ["A"]
    assert one("GTTG", 0, 4, 1)[1] == ["G"] and one("TGCC", 0, 4, 2)[1] == ["CC"]
    assert one("TCGA", 0, 4, 1)[1] == ["A"]
    # columns without a position, and columns without a base
    got, motifs, counts = one("ACG", 0, 3, 5)
    assert motifs == ["ACGNN"] and got.tolist() == [(0, 3, 3, 5, 0)] and counts[3:].sum() == 0
    got, motifs, counts = one("NNNNNN", 0, 6, 2)
    assert motifs == ["NN"] and got.tolist() == [(0, 0, 0, 2, 0)] and counts.sum() == 0
    got, motifs, _ = one("ANANAN", 0, 6, 2)
    assert motifs == ["AN"] and got.tolist() == [(0, 3, 3, 2, 0)]
    # lower case counts as upper case; IUPAC letters count for nothing
    assert one("acgtACGt", 0, 8, 4)[1] == ["ACGT"] and one("acgtACGt", 0, 8, 4)[0]["agree"][0] == 8
    got, motifs, _ = one("ARYGARYG", 0, 8, 4)
    assert motifs == ["ANNG"] and got.tolist() == [(0, 4, 4, 4, 0)]
    # a range: rows are relative to begin, and nothing behind end counts
    got, motifs, _ = M.consensus("TTTTACGACGACCTTTT", M.repeats((0, 9, 3), (1, 9, 3)), begin=4, end=13)
    assert motifs == ["ACG", "CGA"] and got.tolist() == [(0, 8, 9, 3, 0), (3, 7, 8, 3, 0)]


# ---- the host helpers ----

def test_primitive_and_canonical_motif():
    import prf_native as pn
    assert [pn.primitive_period(m) for m in ("A", "AAAA", "ACAC", "ACGACG", "ACGACT", "ACGTA", "ANAN")] == [1, 1, 2, 3, 6, 5, 2]
    # rotation: every phase of one motif has one key
    assert {pn.canonical_motif(m) for m in ("CAG", "AGC", "GCA")} == {"AGC"}
    # reverse complement: CTG is CAG read from the other strand
    assert {pn.canonical_motif(m) for m in ("CTG", "TGC", "GCT")} == {"AGC"}
    assert pn.canonical_motif("TTAGGG") == pn.canonical_motif("CCCTAA") == "AACCCT"
    # a palindromic motif is its own reverse complement
    assert pn.canonical_motif("ACGT") == "ACGT" and pn.canonical_motif("GTAC") == "ACGT" and pn.canonical_motif("AT") == "AT"
    # N pairs with N; lower case is folded; anything else is refused
    assert pn.canonical_motif("NTTG") == pn.canonical_motif("CAAN") == "AANC" and pn.canonical_motif("gca") == "AGC"
    assert pn.canonical_motif("") == "" and pn.canonical_motif("T") == "A"
    with pytest.raises(ValueError, match="A, C, G, T, N"):
        pn.canonical_motif("ACRT")


def test_consensus_rows_fields():
    import prf_native as pn
    chains = np.array([(2, 11, 10, 3, 2), (0, 1, 1, 1, 1), (22, 8, 8, 4, 1)], dtype=pn.PCHAIN_DTYPE)
    tandem = pn.tandem_rows(chains)
    seq = "ttttttttttacgacgacgacgatacgtttACACACACACACtt"
    cons, motifs, _ = M.consensus(seq, tandem, begin=8)
    rows = pn.consensus_rows(tandem, cons.astype(pn.CONSENSUS_DTYPE), motifs)
    assert [name for name, _ in pn.TANDEM_CONSENSUS_DTYPE] == [name for name, _ in pn.TANDEM_DTYPE] + ["consensus_identity", "primitive"]
    for name, _ in pn.TANDEM_DTYPE:
        assert rows[name].tolist() == tandem[name].tolist()
    assert motifs == ["ACG", "T", "ACAC"] and rows["primitive"].tolist() == [3, 1, 2]
    assert rows["consensus_identity"].tolist() == [13 / 14, 1.0, 1.0]         # acgacgacgacgat: one t against the column's A
    with pytest.raises(ValueError, match="period_consensus returned"):
        pn.consensus_rows(tandem, cons[:2].astype(pn.CONSENSUS_DTYPE), motifs[:2])
    with pytest.raises(ValueError, match="period_consensus returned"):
        pn.consensus_rows(tandem, cons[::-1].astype(pn.CONSENSUS_DTYPE), motifs)
    assert len(pn.consensus_rows(tandem[:0], cons[:0].astype(pn.CONSENSUS_DTYPE), [])) == 0


# ---- the per-lane text of the kernels, on the host ----

def test_item_text_against_a_brute_force_on_the_host(tmp_path):
    """csrc/consensus_word.h is the text the kernels run; the stand-alone program checks it and the item cutting on random and
    hand-made ranges in every regime, with slices smaller than k, under the sanitizers.  Its source of plane words refuses any
    word outside the range's, outside the item's, asked for twice or out of order."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/consensus_word_check.cpp")
    exe = tmp_path / "consensus_word_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "consensus_word_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, rows, items, words, positions = done.stdout.split()
    assert word == "ok" and int(rows) == 600 * 12 and int(items) > 50_000 and int(words) > 100_000 and int(positions) > 1_000_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_consensus.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.CONSENSUS_EXPORTS) and len(declared) == 3
    older = (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS) |
             set(pn.DOTCHAIN_EXPORTS) | set(pn.DOTLINK_EXPORTS) | set(pn.PERIODCHAIN_EXPORTS) | set(pn.PERIODLINK_EXPORTS))
    assert not set(declared) & older
    assert open(os.path.join(ROOT, "include", "prf.h")).read().count('#include "prf_consensus.h"') == 1
    assert all(hasattr(lib, name) and getattr(lib, name).argtypes for name in declared)
    assert lib.prf_abi_version() == 4
    for name, value in (("PRF_CONSENSUS_MAX_ROWS", pn.CONSENSUS_MAX_ROWS), ("PRF_CONSENSUS_MAX_LETTERS", pn.CONSENSUS_MAX_LETTERS)):
        found = re.search(rf"#define {name} \((\d+)ull << (\d+)\)", text)
        assert found and int(found[1]) << int(found[2]) == value, name
    assert pn.CONSENSUS_MAX_ROWS == 1 << 24 and pn.CONSENSUS_MAX_LETTERS == 1 << 26
    assert int(re.search(r"#define PRF_CONSENSUS_SLICE (\d+)u", text)[1]) == pn.CONSENSUS_SLICE
    assert np.dtype(pn.REPEAT_DTYPE).itemsize == 24 and np.dtype(pn.CONSENSUS_DTYPE).itemsize == 32
    assert pn.CONSENSUS_DTYPE == M.DTYPE and pn.REPEAT_DTYPE == M.REPEAT_DTYPE
    struct = re.search(r"typedef struct prf_consensus \{(.*?)\} prf_consensus;", text, flags=re.S)[1]
    assert re.findall(r"\b(offset|agree|acgt|k|reserved);", struct) == list(M.FIELDS)
    struct = re.search(r"typedef struct prf_repeat \{(.*?)\} prf_repeat;", text, flags=re.S)[1]
    assert re.findall(r"\b(start|end|k|reserved);", struct) == ["start", "end", "k", "reserved"]


ROWS = ((0, 12, 3),)


def _call(lib, pn, form, seq=b"ACGTACGTACGT", span=(0, 12), rows=ROWS, n_rows=None, dst=True, motifs=True, capacity=64, counts=True,
          written=False):
    table = np.zeros(max(1, len(rows or ())), dtype=pn.REPEAT_DTYPE)
    for at, row in enumerate(rows or ()):
        table[at] = tuple(row) + (0,) * (4 - len(row))
    out = np.full(64 * 32, 0xAB, dtype=np.uint8)
    letters = np.full(64, 0xAB, dtype=np.uint8)
    sums = np.full(64 * 16, 0xAB, dtype=np.uint8)
    stats = pn.ScanStats()
    stats.n_hits = 77
    tail = (*span, table.ctypes.data if rows is not None else None, len(rows or ()) if n_rows is None else n_rows,
            out.ctypes.data if dst else None, letters.ctypes.data if motifs else None, capacity, sums.ctypes.data if counts else None,
            ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_period_consensus_seq(None, arr, *tail)
    elif form == "ex":
        rc = lib.prf_period_consensus_ex(None, None, 0, *tail, 100)
    else:
        rc = lib.prf_period_consensus(None, None, 0, *tail)
    assert written or ((out == 0xAB).all() and (letters == 0xAB).all() and (sums == 0xAB).all() and stats.n_hits == 77)   # a refused call writes nothing
    return rc


BIG_K = (1 << 26) + 1
# each case breaks one rule and, where a call can, the rules behind it: the first in the documented order is the one reported
ORDER = [
    (dict(span=(7, 3), n_rows=(1 << 24) + 1, rows=None, dst=False, motifs=False), "PRF_EINVAL", "begin 7"),
    (dict(n_rows=(1 << 24) + 1, rows=None, dst=False, motifs=False), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_ROWS"),
    (dict(rows=None, n_rows=1, dst=False, motifs=False), "PRF_EINVAL", "NULL rows"),
    (dict(rows=((0, 0, 0),), dst=False, motifs=False), "PRF_EINVAL", "NULL destination"),
    (dict(rows=((0, 0, 0),), motifs=False), "PRF_EINVAL", "NULL motifs"),
    (dict(rows=((0, 12, 3), (5, 5, 0, 1), (0, 12, BIG_K)), capacity=1), "PRF_EINVAL", "row 1: k is 0"),
    (dict(rows=((0, 12, 3), (5, 5, 2, 1), (0, 12, 0)), capacity=1), "PRF_EINVAL", "row 1: start 5"),
    (dict(rows=((7, 5, 2), (0, 12, 0)), capacity=1), "PRF_EINVAL", "row 0: start 7"),
    (dict(rows=((0, 12, 3), (0, 12, BIG_K, 9), (0, 1 << 33, 1)), capacity=1), "PRF_EINVAL", "row 1: reserved is 9"),
    (dict(rows=((0, 12, BIG_K), (0, 1 << 33, 1), (0, 12, 0)), capacity=1), "PRF_EUNSUPPORTED", "row 1: a column of more than 2^32 - 1"),
    (dict(rows=((0, (1 << 32) - 1, 1),), capacity=0), "PRF_EINVAL", "holds 0 letters"),     # 2^32 - 1 positions in a column pass
    (dict(rows=((0, 12, BIG_K),), capacity=1), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_LETTERS"),
    (dict(rows=((0, 12, 1 << 25), (0, 13, 1 << 25), (3, 12, 1)), capacity=1 << 27), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_LETTERS"),
    (dict(rows=((0, 12, 3), (0, 13, 4)), capacity=6), "PRF_EINVAL", "holds 6 letters, the k of the rows add up to 7"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(counts=False, rows=((0, 12, 1 << 25), (0, 1, 1 << 25)), capacity=1 << 26), "PRF_EINVAL", "NULL context"),   # the limits themselves pass
    (dict(rows=((11, 12, 62), (0, 12, 1), (0, 12, 1)), span=(0, 1 << 63)), "PRF_EINVAL", "NULL context"),   # rows may repeat; end is clipped
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_period_consensus")


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(rows=((0, 12, 3), (0, 13, 4))), "PRF_EINVAL", "row 1: end 13 is behind the range's 12 positions"),
    (dict(rows=((0, 9, 3), (2, 10, 4)), span=(3, 12)), "PRF_EINVAL", "row 1: end 10 is behind the range's 9 positions"),
    (dict(rows=((0, 13, 4),), seq=b"ACGT-ACGTACG"), "PRF_EINVAL", "row 0: end 13"),     # the rows are judged before the bytes
    (dict(seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(rows=((0, 1, 1),), seq=b""), "PRF_EINVAL", "row 0: end 1 is behind the range's 0 positions"),
    (dict(span=(2, 1 << 63), rows=((0, 10, 3),)), "PRF_EINVAL", "NULL context"),      # ends are clipped
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_no_rows_is_no_work_and_no_error(form):
    pn, lib = _lib()
    assert _call(lib, pn, form, rows=None, n_rows=0, dst=False, motifs=False, counts=False) == pn.PRF_OK
    assert _call(lib, pn, form, rows=(), capacity=0) == pn.PRF_OK
    assert _call(lib, pn, form, rows=(), span=(7, 3)) == pn.PRF_EINVAL          # ... but the range is still judged


def test_a_missing_sequence_is_refused():
    pn, lib = _lib()
    row = np.array([(0, 4, 2, 0)], dtype=pn.REPEAT_DTYPE)
    out, letters = np.zeros(1, dtype=pn.CONSENSUS_DTYPE), np.zeros(8, dtype=np.uint8)
    rc = lib.prf_period_consensus_seq(None, None, 0, 4, row.ctypes.data, 1, out.ctypes.data, letters.ctypes.data, 8, None, None)
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 2, [100, 50])
    ok = M.repeats((0, 10, 3))
    with pytest.raises(ValueError, match="contig 2"):
        g.period_consensus(2, 0, None, ok)
    with pytest.raises(ValueError, match="begin"):
        g.period_consensus(0, 30, 20, ok)
    with pytest.raises(ValueError, match="fields start, end and k"):
        g.period_consensus(0, 0, None, np.zeros(3, dtype=[("start", "<u8"), ("len", "<u8"), ("k", "<u4")]))
    with pytest.raises(ValueError, match="fields start, end and k"):
        g.period_consensus(0, 0, None, [(0, 10, 3)])
    with pytest.raises(ValueError, match="repeat 1: k"):
        g.period_consensus(0, 0, None, M.repeats((0, 10, 3), (0, 10, 0)))
    with pytest.raises(ValueError, match=r"repeat 0: \[5, 5\)"):
        g.period_consensus(0, 0, None, M.repeats((5, 5, 3)))
    with pytest.raises(ValueError, match=r"repeat 1: \[0, 51\) is not a stretch of the range's 50 positions"):
        g.period_consensus(1, 0, None, M.repeats((0, 50, 3), (0, 51, 3)))
    with pytest.raises(ValueError, match=r"range's 20 positions"):
        g.period_consensus(0, 10, 30, M.repeats((0, 21, 3)))
    with pytest.raises(ValueError, match="add up to"):
        g.period_consensus(0, 0, None, M.repeats((0, 10, 1 << 26), (0, 10, 1)))
    with pytest.raises(ValueError, match="slice_positions"):
        g.period_consensus(0, 0, None, ok, slice_positions=-1)
    g._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_input(args, parser), args


def test_cli_parses_the_consensus_options(capsys):
    import plot_periodicity_matrix as cli
    base = ["ACGTACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2"]
    args = _parse(cli, base)[1]
    assert (args.consensus, args.min_consensus_identity) == (False, None)
    args = _parse(cli, base + ["--consensus", "--min-consensus-identity", "0.8"])[1]
    assert (args.consensus, args.min_consensus_identity) == (True, 0.8)
    capsys.readouterr()
    groups = ["ACGT", "--groups-tsv", "g.tsv", "--min-seed", "4", "--max-gap", "2", "--max-shift", "2"]
    for argv, text in ((["ACGT", "--consensus"], "--consensus belongs to --chains-tsv"),
                       (["ACGT", "--window", "64", "--consensus"], "--consensus belongs to --chains-tsv"),
                       (groups + ["--consensus"], "drift at an indel"),
                       (base + ["--min-consensus-identity", "0.5"], "belongs to --consensus"),
                       (base + ["--consensus", "--min-consensus-identity", "1.5"], "0 .. 1"),
                       (base + ["--consensus", "--min-consensus-identity", "-0.1"], "0 .. 1")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_consensus_batches_respect_both_limits():
    import plot_periodicity_matrix as cli
    ks = [3, 5, 2, 9, 1, 1, 7]
    assert list(cli.consensus_batches(ks, 100, 100)) == [(0, 7)]
    assert list(cli.consensus_batches(ks, 3, 100)) == [(0, 3), (3, 6), (6, 7)]
    assert list(cli.consensus_batches(ks, 100, 10)) == [(0, 3), (3, 5), (5, 7)]
    assert list(cli.consensus_batches(ks, 2, 8)) == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 7)]    # a row above the limit goes alone
    assert list(cli.consensus_batches([], 2, 8)) == []
    for rows, letters in ((1, 1), (2, 9), (3, 12), (7, 28)):
        parts = list(cli.consensus_batches(ks, rows, letters))
        assert [a for a, _ in parts] + [len(ks)] == [0] + [b for _, b in parts]
        assert all(b - a <= rows and (sum(ks[a:b]) <= letters or b - a == 1) for a, b in parts)


class _FakeGenome:
    """What list_chains asks of a resident genome, answered by the model: fixed chains, and the consensus of the CPU model."""

    def __init__(self, seq, chains):
        self.seq, self.chains, self.calls = seq, chains, []

    def period_chains(self, contig, begin, end, *args):
        self.calls.append("chains")
        return self.chains

    def period_consensus(self, contig, begin, end, repeats):
        import prf_native as pn
        self.calls.append(("consensus", len(repeats)))
        rows, motifs, _ = M.consensus(self.seq, repeats, begin, end)
        return rows.astype(pn.CONSENSUS_DTYPE), motifs

    def free(self):
        self.calls.append("free")


class _FakeContext:
    def __init__(self, genome):
        self.genome = genome

    def load(self, seqs, kmax_hint):
        return self.genome


def test_cli_lines_with_and_without_consensus(tmp_path):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    seq = "ttttttttttacgacgacgacgatacgtttt"
    chains = np.array([(10, 11, 10, 3, 2), (0, 9, 9, 1, 1)], dtype=pn.PCHAIN_DTYPE)
    plain, named, kept = (str(tmp_path / name) for name in ("plain.tsv", "named.tsv", "kept.tsv"))
    base = [seq, "--chains-tsv", plain, "--min-seed", "3", "--max-gap", "2", "--keep-multiples"]
    genome = _FakeGenome(seq, chains)
    cli.main(base, context=_FakeContext(genome))
    # without --consensus: the lines of chain_lines, byte for byte, and the consensus is never asked for
    want = ["sequence\t10\t24\t3\t4.667\t0.9091\t10\t2\tACG\n", "sequence\t0\t10\t1\t10.000\t1.0000\t9\t1\tT\n"]
    assert open(plain).read() == "".join(want) and genome.calls == ["chains", "free"]
    genome = _FakeGenome(seq, chains)
    cli.main(base[:2] + [named] + base[3:] + ["--consensus"], context=_FakeContext(genome))
    assert genome.calls == ["chains", ("consensus", 2), "free"]
    assert open(named).read() == want[0][:-1] + "\tACG\t0.9286\t3\tACG\n" + want[1][:-1] + "\tT\t1.0000\t1\tA\n"
    cli.main(base[:2] + [kept] + base[3:] + ["--consensus", "--min-consensus-identity", "0.95"], context=_FakeContext(_FakeGenome(seq, chains)))
    assert open(kept).read() == want[1][:-1] + "\tT\t1.0000\t1\tA\n"
