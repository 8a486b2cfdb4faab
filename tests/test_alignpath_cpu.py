"""CPU: the alignment of tandem repeats to their motifs with its path (include/prf_alignpath.h): the model
(tests/alignpath_model.py) against an independent full-matrix traceback on explicit triples, its invariants and closed forms; the
planted inputs of tests/phased_cases.py; the host helpers of prf_native (path_cigar, path_copies, aligned_consensus,
refine_motifs); the C ABI (what is declared, bound and exported, and every refusal in its documented order, which needs no
device); and the per-lane text of the kernels on the host, under the sanitizers."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_model as A
import alignpath_model as P
import phased_cases as K
from conftest import ROOT
from test_align_cpu import _cases


# ---- the model against a full matrix of explicit triples ----

def full_matrix(seq, motif):
    """(alignment, path, deleted (position in front, column)): every cell a tuple (edits, indels, consumed), T and D' both kept,
    the two bits by their definition, then the walk."""
    s, m = seq.upper(), motif.upper()
    n, k = len(s), len(m)
    add = lambda cell, step: tuple(a + b for a, b in zip(cell, step))
    D = [(0, 0, 0)] * k
    ins, dele = [], []
    for i in range(n):
        across = [add(D[(j - 1) % k], (0 if s[i] == m[j] and s[i] in "ACGT" else 1, 0, 1)) for j in range(k)]
        down = [add(D[j], (1, 1, 0)) for j in range(k)]
        T = [min(a, d) for a, d in zip(across, down)]
        ins.append([d < a for a, d in zip(across, down)])
        new = list(T)
        for _ in range(2):                                                     # deletions from the left, twice around: the wrap
            for j in range(k):
                new[j] = min(new[j], add(new[(j - 1) % k], (1, 1, 1)))
        dele.append([new[j] < T[j] for j in range(k)])
        D = new
    col = min(range(k), key=lambda j: (D[j], j))
    edits, indels, consumed = D[col]
    path, deleted = [0] * n, []
    i, j = n - 1, col
    while i >= 0:
        if dele[i][j]:
            deleted.append((i, j))
            j = (j - 1) % k
        elif ins[i][j]:
            path[i] = j | P.INS
            i -= 1
        else:
            path[i] = j | (0 if s[i] == m[j] and s[i] in "ACGT" else P.SUB)
            j = (j - 1) % k
            i -= 1
    return (edits, indels, consumed, (col + 1 - consumed) % k, col), path, deleted


def _invariants(seq, motif, al, path, counts, deleted):
    n, k = len(seq), len(motif)
    ins, sub = (path & P.INS) != 0, (path & P.SUB) != 0
    assert not (path & 0x3C00).any() and ((path & P.COLUMN) < k).all() and not (ins & sub).any()
    assert not ins[0] and int(path[0]) & P.COLUMN == al[3]                       # position 0 is never an insertion
    assert not deleted or deleted[0] != (n - 1, al[4])                           # the final cell is never a deletion cell
    assert int(ins.sum()) + len(deleted) == al[1]
    assert int(sub.sum()) + int(ins.sum()) + len(deleted) == al[0]
    assert n - int(ins.sum()) + len(deleted) == al[2]
    runs = {}
    for i, _ in deleted:
        runs[i] = runs.get(i, 0) + 1
    assert all(run < k for run in runs.values())                                 # a run of deletions is shorter than k
    # the deletions from the path alone: directly behind the position in front of them
    behind = P.deletions_behind(path, k)
    assert runs == {i: int(d) for i, d in enumerate(behind) if d}
    assert counts[:, 4].sum() == len(deleted) and counts[:, 5].sum() == ins.sum()
    assert counts[:, :4].sum() == sum(1 for c, flag in zip(seq.upper(), ins) if c in "ACGT" and not flag)


def test_model_agrees_with_a_full_matrix_traceback():
    n_cases = gapped = wrapped = with_ins = 0
    for seq, motif in _cases(3_200, 311):
        al, path, counts, deleted = P.path_one(seq, motif)
        want = full_matrix(seq, motif)
        assert al == want[0] == tuple(A.align_one(seq, motif)), (seq, motif)     # the path's triple is align_one's
        assert path.tolist() == want[1] and deleted == want[2], (seq, motif)
        _invariants(seq, motif, al, path, counts, deleted)
        n_cases, gapped, with_ins = n_cases + 1, gapped + bool(deleted), with_ins + bool((path & P.INS).any())
        wrapped += any(j == 0 for _, j in deleted) and len(motif) > 1
    assert n_cases >= 3_000 and gapped > 80 and with_ins > 200 and wrapped > 10                 # the inputs: deletions, insertions, runs through column 0


def test_the_final_cell_is_never_a_deletion_cell():
    for seq, motif in _cases(1_500, 312):
        _, _, from_del = P.forward(A._SEQ[P._bytes(seq)], A.motif_codes(motif))
        assert not from_del[-1, P.path_one(seq, motif)[0][4]], (seq, motif)


def test_closed_forms():
    rng = random.Random(313)
    for k in (1, 2, 3, 5, 7, 64, 65, 130):
        motif = ""
        while not motif or not K.primitive(motif):
            motif = "".join(rng.choice("ACGT") for _ in range(k))
        for phase in sorted({0, 1 % k, k - 1, rng.randrange(k)}):
            for n in (k, k + 1, 3 * k + 2):
                seq = "".join(motif[(phase + t) % k] for t in range(n))
                al, path, counts, deleted = P.path_one(seq, motif)
                assert np.array_equal(path, P.perfect(motif, phase, n)) and not deleted, (motif, phase, n)
                sizes = np.bincount((phase + np.arange(n)) % k, minlength=k)
                want = np.zeros((k, 6), dtype=np.uint32)
                want[np.arange(k), ["ACGT".index(c) for c in motif]] = sizes      # the counts are the sizes of the columns
                assert np.array_equal(counts, want)
    for n in (1, 2, 9, 100):
        al, path, counts, deleted = P.path_one("A" * n, "C")
        assert (path == P.SUB).all() and not deleted and counts.tolist() == [[n, 0, 0, 0, 0, 0]]      # all SUB at column 0
        assert (P.path_one("N" * n, "N")[1] == P.SUB).all() and not P.path_one("N" * n, "N")[2].any()
        assert not P.path_one("a" * n, "A")[1].any()
    al, path, counts, deleted = P.path_one("ACGTACGTTACGTACGT", "ACGT")
    assert al == (1, 1, 16, 0, 3) and int((path & P.INS != 0).sum()) == 1 and not deleted
    al, path, counts, deleted = P.path_one("ACGTACGACGTACGT", "ACGT")
    assert al == (1, 1, 16, 0, 3) and deleted == [(6, 3)] and path.tolist() == [0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3]
    assert counts[:, 4].tolist() == [0, 0, 0, 1]


# ---- the planted inputs ----

def _planted_inputs():
    for key in list(K.SEEDS) + [7, 17, 40]:
        motif, seq = K.planted(*key) if isinstance(key, tuple) else K.close_pair(key)
        yield key, motif, seq[K.FLANK:len(seq) - K.FLANK]


def test_the_aligned_consensus_is_the_planted_motif():
    """All 30 of tests/phased_cases.py, the three close pairs (which DESIGN 19 cuts into pieces) among them: the body against the
    planted motif gives the planted motif back; from a motif with one wrong letter, one round restores it."""
    import prf_native as pn
    seen = 0
    for key, motif, body in _planted_inputs():
        al, path, counts, deleted = P.path_one(body, motif)
        assert pn.aligned_consensus(counts, motif) == motif, key
        at = len(motif) // 3
        wrong = motif[:at] + next(c for c in "ACGT" if c != motif[at]) + motif[at + 1:]
        assert pn.aligned_consensus(P.path_one(body, wrong)[2], wrong) == motif, key
        if isinstance(key, tuple):                                              # the number of INS entries, not their places
            d, kind = key[1], key[2]
            assert int((path & P.INS != 0).sum()) == (d if kind != "del" else 0) and len(deleted) == (d if kind != "ins" else 0), key
        else:
            assert int((path & P.INS != 0).sum()) == 2 and not deleted, key
        seen += 1
    assert seen == 30


class _ModelGenome:
    """What refine_motifs asks of a resident genome, answered by the model."""

    def __init__(self, seq):
        self.seq, self.calls = seq, 0

    def motif_align_path(self, contig, begin, end, repeats, motifs, with_counts=False, trace_bytes=0):
        import prf_native as pn
        self.calls += 1
        rows, path, counts = P.align_path(self.seq, repeats, motifs, begin, end)
        firsts = np.concatenate([[0], np.cumsum(repeats["end"] - repeats["start"])]).astype(np.int64)
        return rows.astype(pn.ALIGNMENT_DTYPE), [path[a:b] for a, b in zip(firsts[:-1], firsts[1:])], counts


def test_refine_motifs_over_the_model():
    import prf_native as pn
    inputs = list(_planted_inputs())[::5]
    seq, rows, motifs = "", [], []
    for _, motif, body in inputs:
        rows.append((len(seq) + 3, len(seq) + 3 + len(body), len(motif)))
        motifs.append(motif)
        seq += "TTT" + body
    table = A.repeats(*rows)
    wrong = [m[:len(m) // 3] + next(c for c in "ACGT" if c != m[len(m) // 3]) + m[len(m) // 3 + 1:] for m in motifs]
    mixed = wrong[:3] + motifs[3:]
    g = _ModelGenome(seq)
    refined, align, changed = pn.refine_motifs(g, 0, 0, None, table, mixed, rounds=4)
    assert refined == motifs and changed.tolist() == [1, 1, 1] + [0] * (len(motifs) - 3)
    assert g.calls == 2 and A.same(align.astype(A.DTYPE), A.align(seq, table, motifs))     # stops when nothing changes
    g = _ModelGenome(seq)
    refined, align, changed = pn.refine_motifs(g, 0, 0, None, table, "".join(mixed), rounds=1)
    assert refined == motifs and g.calls == 2 and A.same(align.astype(A.DTYPE), A.align(seq, table, motifs))   # aligned once more
    with pytest.raises(ValueError, match="rounds"):
        pn.refine_motifs(g, 0, 0, None, table, mixed, rounds=0)


# ---- the host helpers ----

def _cigar_counts(cigar):
    found = re.findall(r"(\d+)([=XID])", cigar)
    assert "".join(n + op for n, op in found) == cigar
    assert all(a[1] != b[1] for a, b in zip(found, found[1:]))                   # runs are maximal
    return {op: sum(int(n) for n, o in found if o == op) for op in "=XID"}


def test_path_cigar_and_path_copies():
    import prf_native as pn
    assert pn.path_cigar(P.path_one("ACGTACGTTACGTACGT", "ACGT")[1], 4) in ("8=1I8=", "7=1I9=")
    assert pn.path_cigar(P.path_one("ACGTACGACGTACGT", "ACGT")[1], 4) == "7=1D8="
    assert pn.path_cigar(P.path_one("ACGTACGTACCTACGT", "ACGT")[1], 4) == "10=1X5="
    assert pn.path_cigar(np.zeros(0, dtype=np.uint16), 4) == "" and len(pn.path_copies(np.zeros(0, dtype=np.uint16), 0, 4)) == 0
    copies = pn.path_copies(P.path_one("GTACGTACCTACGACGTAC", "ACGT")[1], 100, 4)
    assert copies.dtype == np.dtype(pn.PATH_COPY_DTYPE) and copies["copy"].tolist() == [0, 1, 2, 3, 4]
    assert copies["start"].tolist() == [100, 104, 108, 112, 115] and copies["end"].tolist() == [104, 108, 112, 115, 119]
    assert copies["subs"].tolist() == [0, 0, 1, 0, 0] and copies["dels"].tolist() == [0, 0, 0, 1, 0] and not copies["ins"].any()
    n_cases = 0
    for seq, motif in _cases(1_200, 314):
        al, path, counts, deleted = P.path_one(seq, motif)
        n, k = len(seq), len(motif)
        subs, ins, dele = A.derived(n, k, *al[:3])[:3]
        got = _cigar_counts(pn.path_cigar(path, k))
        assert (got["X"], got["I"], got["D"]) == (subs, ins, dele) and got["="] + got["X"] + got["I"] == n, (seq, motif)
        assert pn.path_deletions(path, k).tolist() == P.deletions_behind(path, k).tolist()
        copies = pn.path_copies(path, 7, k)
        assert copies["start"][0] == 7 and copies["end"][-1] == 7 + n and (copies["start"][1:] == copies["end"][:-1]).all()
        assert (copies["subs"].sum(), copies["ins"].sum(), copies["dels"].sum()) == (subs, ins, dele)
        first = int(path[0]) & P.COLUMN                                          # every copy but the first begins where the path enters the start column
        for start in copies["start"][1:].tolist():
            assert int(path[start - 7]) & P.COLUMN == first and not int(path[start - 7]) & P.INS
        n_cases += 1
    assert n_cases >= 1_000


def test_aligned_consensus():
    import prf_native as pn
    counts = np.array([[3, 3, 0, 0, 9, 9], [0, 1, 2, 2, 0, 0], [0, 0, 0, 0, 5, 5], [0, 0, 0, 7, 0, 0], [1, 0, 0, 0, 0, 0]], dtype=np.uint32)
    assert pn.aligned_consensus(counts, "TTnTT") == "AGnTA"                      # ties in the order A, C, G, T; no counts: the letter stays
    assert pn.aligned_consensus(counts, ["TT", "nTT"]) == ["AG", "nTA"] and pn.aligned_consensus(counts, b"TTnTT") == "AGnTA"
    assert pn.aligned_consensus(counts[:, :4], "TTnTT") == "AGnTA"
    with pytest.raises(ValueError, match="needs the counts"):
        pn.aligned_consensus(counts, "TTTT")


# ---- the per-lane text of the kernels, on the host ----

def test_lane_text_against_a_full_matrix_on_the_host(tmp_path):
    """csrc/alignpath_word.h is the text the kernels run; the stand-alone program checks the layout of the trace, the step of the
    walk, the batch dealer at budgets of one row, several rows and an oversized row, and 64 emulated lanes (forward, packing,
    walk) against a full-matrix traceback on explicit triples in every kernel's range of k, under the sanitizers.  Nothing is
    loaded into this process."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/alignpath_word_check.cpp")
    exe = tmp_path / "alignpath_word_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "alignpath_word_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, rows, cells, batches = done.stdout.split()
    assert word == "ok" and int(rows) == 300 and int(cells) > 1_000_000 and int(batches) > 1_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_alignpath.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.ALIGNPATH_EXPORTS) == ["prf_motif_align_path", "prf_motif_align_path_ex", "prf_motif_align_path_seq"]
    older = [pn.EXPORTS, pn.PERIOD_EXPORTS, pn.DOTPLOT_EXPORTS, pn.DOTPAIR_EXPORTS, pn.DOTRUNS_EXPORTS, pn.DOTCHAIN_EXPORTS, pn.DOTLINK_EXPORTS,
             pn.PERIODCHAIN_EXPORTS, pn.PERIODLINK_EXPORTS, pn.CONSENSUS_EXPORTS, pn.PHASED_EXPORTS, pn.ALIGN_EXPORTS]
    assert len(older) == 12 and not set(declared) & set().union(*older)
    header = open(os.path.join(ROOT, "include", "prf.h")).read()
    assert header.count('#include "prf_alignpath.h"') == 1 and header.index('#include "prf_alignpath.h"') < header.index("#ifdef __cplusplus\n}")
    between = header[header.index('#include "prf_align.h"') + len('#include "prf_align.h"'):header.index('#include "prf_alignpath.h"')]
    assert not re.sub(r"/\*.*?\*/", "", between, flags=re.S).strip()              # directly behind prf_align.h
    assert all(hasattr(lib, name) and getattr(lib, name).argtypes for name in declared)
    assert len(lib.prf_motif_align_path_ex.argtypes) == len(lib.prf_motif_align_path.argtypes) + 1 == 15
    raw = ctypes.CDLL(pn.LIB_PATH)                                             # exported: the loader finds them by name
    assert all(hasattr(raw, name) for name in declared)
    assert lib.prf_abi_version() == 4
    found = re.search(r"#define PRF_ALIGNPATH_MAX_POSITIONS \((\d+)ull << (\d+)\)", text)
    assert int(found[1]) << int(found[2]) == pn.ALIGNPATH_MAX_POSITIONS == P.MAX_POSITIONS == 1 << 30
    found = re.search(r"#define PRF_ALIGNPATH_TRACE_BYTES \((\d+)ull << (\d+)\)", text)
    assert int(found[1]) << int(found[2]) == 1 << 30
    for name, value in (("INS", 0x8000), ("SUB", 0x4000), ("COLUMN", 0x03FF)):
        assert int(re.search(rf"#define PRF_PATH_{name} (0x[0-9A-Fa-f]+)u", text)[1], 16) == getattr(pn, f"PATH_{name}") == getattr(P, name) == value
    # the header in front and its declarations stay as they are
    older_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_align.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", older_text))) == sorted(pn.ALIGN_EXPORTS)


ROWS = ((0, 12, 3),)
FORMS = ["genome", "ex", "one_shot"]


def _call(lib, pn, form, seq=b"ACGTACGTACGT", span=(0, 12), rows=ROWS, n_rows=None, motifs=b"ACG", length=None, dst=True, reserved=0, path=True,
          capacity=1 << 12, counts=True):
    table = np.zeros(max(1, len(rows or ())), dtype=pn.REPEAT_DTYPE)
    for at, row in enumerate(rows or ()):
        table[at] = tuple(row) + (reserved if at == len(rows) - 1 else 0,)
    out = np.full(64 * 24, 0xAB, dtype=np.uint8)
    entries = np.full(1 << 12, 0xABAB, dtype=np.uint16)
    sums = np.full(1 << 14, 0xABABABAB, dtype=np.uint32)
    stats = pn.ScanStats()
    stats.n_hits = 77
    tail = (*span, table.ctypes.data if rows is not None else None, len(rows or ()) if n_rows is None else n_rows, motifs,
            len(motifs or b"") if length is None else length, out.ctypes.data if dst else None, entries.ctypes.data if path else None, capacity,
            sums.ctypes.data if counts else None, ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_motif_align_path_seq(None, arr, *tail)
    elif form == "ex":
        rc = lib.prf_motif_align_path_ex(None, None, 0, *tail, 4_096)
    else:
        rc = lib.prf_motif_align_path(None, None, 0, *tail)
    assert (out == 0xAB).all() and (entries == 0xABAB).all() and (sums == 0xABABABAB).all() and stats.n_hits == 77    # a refused call writes nothing
    return rc


LONG = (1 << 19) + 1
# each case breaks one rule and, where a call can, the rules behind it: the first in the documented order is the one reported
ORDER = [
    (dict(span=(7, 3), n_rows=(1 << 24) + 1, rows=None, motifs=None, dst=False, path=False), "PRF_EINVAL", "begin 7"),
    (dict(n_rows=(1 << 24) + 1, rows=None, motifs=None, dst=False, path=False), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_ROWS"),
    (dict(rows=None, n_rows=1, motifs=None, dst=False, path=False), "PRF_EINVAL", "NULL rows"),
    (dict(rows=((0, 12, 0),), motifs=None, dst=False, path=False), "PRF_EINVAL", "NULL motifs"),
    (dict(rows=((0, 12, 0),), dst=False, path=False), "PRF_EINVAL", "NULL destination"),
    (dict(rows=((0, 12, 0),), path=False), "PRF_EINVAL", "NULL path"),
    (dict(rows=((0, 12, 3), (5, 5, 0), (0, 12, 2_000)), length=0, capacity=0), "PRF_EINVAL", "row 1: k is 0"),
    (dict(rows=((0, 12, 3), (5, 5, 2_000)), reserved=9, length=0, capacity=0), "PRF_EINVAL", "row 1: start 5 is not in front of end 5"),
    (dict(rows=((0, 12, 3), (0, LONG, 2_000)), reserved=9, length=0, capacity=0), "PRF_EINVAL", "row 1: reserved is 9"),
    (dict(rows=((0, 12, 3), (0, LONG, 1_025), (0, 0, 0)), length=0, capacity=0), "PRF_EUNSUPPORTED", "row 1: k = 1025 is above 1024 (PRF_ALIGN_MAX_K)"),
    (dict(rows=((0, 12, 3), (7, 7 + LONG, 1_024), (0, 0, 0)), length=0, capacity=0), "PRF_EUNSUPPORTED", "row 1: 524289 positions are above 524288 (PRF_ALIGN_MAX_LEN)"),
    (dict(rows=((0, 12, 3), (7, 6 + LONG, 1_024)), length=1_026, motifs=b"ACR" + b"A" * 1_024, capacity=0), "PRF_EINVAL",
     "holds 1026 letters, the k of the rows add up to 1027"),
    (dict(rows=((0, 1 << 19, 1),) * 2_049, motifs=b"R" * 2_049, capacity=0), "PRF_EUNSUPPORTED", "add up to 1074266112 positions, above 1073741824 (PRF_ALIGNPATH_MAX_POSITIONS)"),
    (dict(rows=((0, 12, 3), (0, 13, 4)), motifs=b"ACGAC-T", capacity=24), "PRF_EINVAL", "the path holds 24 entries, the rows add up to 25 positions"),
    (dict(rows=((0, 12, 3), (0, 13, 4)), motifs=b"ACGAC-T", capacity=25), "PRF_EINVAL", "row 1: column 2 of the motif is the byte 0x2d"),
    (dict(rows=((0, 13, 3),), motifs=b"ARG"), "PRF_EINVAL", "row 0: column 1 of the motif is the byte 0x52"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(counts=False, capacity=12), "PRF_EINVAL", "NULL context"),          # the counts are optional, the path may be exactly as long
    (dict(rows=((0, 12, 3), (2, 9, 4)), motifs=b"acgNnTG", length=9), "PRF_EINVAL", "NULL context"),    # either case, N, room to spare
    (dict(rows=((0, 1 << 19, 1_024),), motifs=b"A" * 1_024, span=(0, 1 << 63), capacity=1 << 19), "PRF_EINVAL", "NULL context"),   # the limits themselves pass
    (dict(rows=((0, 1 << 19, 1),) * 2_048, motifs=b"A" * 2_048, span=(0, 1 << 63), capacity=1 << 30), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", FORMS)
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    if form == "one_shot" and kwargs.get("span") == (0, 1 << 63):             # the one-shot form knows the length: a sequence that holds the row
        kwargs = dict(kwargs, seq=b"A" * (1 << 19))
    rc = _call(lib, pn, form, **kwargs)
    message = lib.prf_last_error().decode()
    assert rc == getattr(pn, code), message
    assert text in message and message.startswith({"genome": "prf_motif_align_path:", "ex": "prf_motif_align_path_ex:", "one_shot": "prf_motif_align_path_seq:"}[form])


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(rows=((0, 12, 3), (0, 13, 4)), motifs=b"ACGACGT"), "PRF_EINVAL", "row 1: end 13 is behind the range's 12 positions"),
    (dict(rows=((0, 13, 3),), seq=b"ACGT-ACGTACG"), "PRF_EINVAL", "row 0: end 13"),           # the rows are judged before the bytes
    (dict(seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(span=(2, 1 << 63), rows=((0, 10, 3),)), "PRF_EINVAL", "NULL context"),              # ends are clipped
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


@pytest.mark.parametrize("form", FORMS)
def test_no_rows_is_no_work_and_no_error(form):
    pn, lib = _lib()
    assert _call(lib, pn, form, rows=None, n_rows=0, motifs=None, dst=False, path=False, counts=False) == pn.PRF_OK
    assert _call(lib, pn, form, rows=(), motifs=b"") == pn.PRF_OK
    assert _call(lib, pn, form, rows=(), span=(7, 3)) == pn.PRF_EINVAL          # ... but the range is still judged


def test_a_missing_sequence_is_refused():
    pn, lib = _lib()
    table, out, path = A.repeats((0, 4, 2)), np.zeros(1, dtype=pn.ALIGNMENT_DTYPE), np.zeros(4, dtype=np.uint16)
    rc = lib.prf_motif_align_path_seq(None, None, 0, 4, table.ctypes.data, 1, b"AC", 2, out.ctypes.data, path.ctypes.data, 4, None, None)
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 2, [100, 50])
    ok = A.repeats((0, 10, 3))
    with pytest.raises(ValueError, match="contig 2"):
        g.motif_align_path(2, 0, None, ok, ["ACG"])
    with pytest.raises(ValueError, match="fields start, end and k"):
        g.motif_align_path(0, 0, None, [(0, 10, 3)], ["ACG"])
    with pytest.raises(ValueError, match=r"repeat 1: \[0, 51\) is not a stretch of the range's 50 positions"):
        g.motif_align_path(1, 0, None, A.repeats((0, 50, 3), (0, 51, 3)), ["ACG", "ACG"])
    with pytest.raises(ValueError, match=r"repeat 1: k = 1025 is more than an alignment takes \(1024\)"):
        g.motif_align_path(0, 0, None, A.repeats((0, 50, 3), (0, 50, 1_025)), ["ACG", "A" * 1_025])
    with pytest.raises(ValueError, match="repeat 0: the motif has 4 letters, k is 3"):
        g.motif_align_path(0, 0, None, ok, ["ACGT"])
    with pytest.raises(ValueError, match="trace_bytes"):
        g.motif_align_path(0, 0, None, ok, ["ACG"], trace_bytes=-1)
    big = pn.Genome(None, None, 1, [1 << 20])
    with pytest.raises(ValueError, match=r"repeat 0: 524289 positions are more than an alignment takes \(524288\)"):
        big.motif_align_path(0, 0, None, A.repeats((1, (1 << 19) + 2, 3)), ["ACG"])
    many = np.zeros(2_049, dtype=pn.REPEAT_DTYPE)
    many["end"], many["k"] = 1 << 19, 1
    with pytest.raises(ValueError, match=r"add up to 1074266112 positions, more than one call's path takes \(1073741824\)"):
        big.motif_align_path(0, 0, None, many, "A" * 2_049)
    g._h = big._h = None


# ---- command line ----

def _fake_genome(seq):
    from test_align_cpu import _FakeGenome

    class _PathGenome(_FakeGenome):
        """... and motif_align_path, answered by the model."""

        def motif_align_path(self, contig, begin, end, repeats, motifs, with_counts=False, trace_bytes=0):
            import prf_native as pn
            assert repeats["k"].max() <= pn.ALIGN_MAX_K and (repeats["end"] - repeats["start"]).max() <= pn.ALIGN_MAX_LEN
            self.calls.append(("path", len(repeats), with_counts))
            rows, path, counts = P.align_path(self.seq, repeats, motifs, begin, end)
            firsts = np.concatenate([[0], np.cumsum(repeats["end"] - repeats["start"])]).astype(np.int64)
            out = (rows.astype(pn.ALIGNMENT_DTYPE), [path[a:b] for a, b in zip(firsts[:-1], firsts[1:])])
            return out + (counts,) if with_counts else out

    return _PathGenome(seq)


def test_cli_parses_the_path_options(capsys):
    import plot_periodicity_matrix as cli
    from test_align_cpu import _parse
    chains = ["ACGTACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2", "--consensus"]
    args = _parse(cli, chains + ["--align"])[1]
    assert (args.align_path, args.refine, args.copies_tsv) == (False, 0, None)
    args = _parse(cli, chains + ["--align", "--align-path", "--refine", "2", "--copies-tsv", "x.tsv"])[1]
    assert (args.align_path, args.refine, args.copies_tsv) == (True, 2, "x.tsv")
    capsys.readouterr()
    for argv, text in ((chains + ["--align-path"], "--align-path belongs to --align"),
                       (chains + ["--refine", "1"], "--refine belongs to --align"),
                       (chains + ["--copies-tsv", "x.tsv"], "--copies-tsv belongs to --align"),
                       (chains + ["--align", "--refine", "-1"], "0 .. 100"),
                       (chains + ["--align", "--refine", "101"], "0 .. 100")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_cli_lines_with_and_without_the_path_options(tmp_path, monkeypatch):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    from test_align_cpu import _FakeContext, _columns
    motif, body = K.planted(17, 2, "both")
    seq = body + K.planted(7, 1, "ins")[1]
    files = {name: str(tmp_path / f"{name}.tsv") for name in ("plain", "same", "cigar", "refined", "copies", "all", "kept", "kcopies", "capped", "gcigar", "gplain")}
    cbase = ["--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--consensus", "--align"]
    # ---- without the new flags: the lines of before, and motif_align answers, not motif_align_path
    genome = _fake_genome(seq)
    cli.main([seq, "--chains-tsv", files["plain"]] + cbase, context=_FakeContext(genome))
    plain = open(files["plain"]).read().splitlines()
    assert len(plain) >= 3 and not [c for c in genome.calls if c[0] == "path"] and [c for c in genome.calls if c[0] == "align"]
    for line in plain:
        f = line.split("\t")
        assert len(f) == 19 and f[13:] == _columns(seq, int(f[1]), int(f[2]), int(f[3]), f[9])
    # ---- --align-path: one more column, the CIGAR of the model's path
    genome = _fake_genome(seq)
    cli.main([seq, "--chains-tsv", files["cigar"], "--align-path"] + cbase, context=_FakeContext(genome))
    cigar = open(files["cigar"]).read().splitlines()
    assert [c for c in genome.calls if c[0] in ("path", "align")] == [("path", len(plain), False)]
    for before, line in zip(plain, cigar):
        f = before.split("\t")
        text = pn.path_cigar(P.path_one(seq[int(f[1]):int(f[2])], f[9])[1], int(f[3]))
        assert line == before + "\t" + text
        got = _cigar_counts(text)
        assert [str(got["X"]), str(got["I"]), str(got["D"])] == f[14:17]
    assert len(cigar) == len(plain)                                            # the gapped ones are the groups, below
    # ---- --refine: the motif, its key and the six columns are those of the last round; `refined` counts the rounds that changed
    genome = _fake_genome(seq)
    cli.main([seq, "--chains-tsv", files["refined"], "--refine", "3"] + cbase, context=_FakeContext(genome))
    refined = open(files["refined"]).read().splitlines()
    assert len(refined) == len(plain)
    moved = 0
    for before, line in zip(plain, refined):
        f, r = before.split("\t"), line.split("\t")
        table = A.repeats((int(f[1]), int(f[2]), int(f[3])))
        want, _, changed = pn.refine_motifs(_fake_genome(seq), 0, 0, None, table, [f[9]], rounds=3)
        assert len(r) == 20 and r[:9] == f[:9] and r[9] == want[0] and r[10:12] == f[10:12] and r[12] == pn.canonical_motif(want[0])
        assert r[13:19] == _columns(seq, int(f[1]), int(f[2]), int(f[3]), want[0]) and r[19] == str(int(changed[0]))
        assert int(r[13]) <= int(f[13])                                          # the refined motif is no further from the repeat
        moved += r[9] != f[9]
    # ---- --copies-tsv: the main file stays, the copies add up to the rows
    cli.main([seq, "--chains-tsv", files["same"], "--copies-tsv", files["copies"]] + cbase, context=_FakeContext(_fake_genome(seq)))
    assert open(files["same"]).read().splitlines() == plain
    copies = [line.split("\t") for line in open(files["copies"]).read().splitlines()]
    assert all(len(c) == 10 for c in copies)
    for before in plain:
        f = before.split("\t")
        mine = [c for c in copies if c[:4] == f[:4]]
        assert [int(c[4]) for c in mine] == list(range(len(mine))) and mine[0][5] == f[1] and mine[-1][6] == f[2]
        assert all(a[6] == b[5] for a, b in zip(mine, mine[1:]))
        assert [str(sum(int(c[col]) for c in mine)) for col in (7, 8, 9)] == f[14:17]
        assert abs(len(mine) - float(f[18])) < 2
    # ---- all three with the filter: the lines that pass, and their copies only
    cli.main([seq, "--chains-tsv", files["all"], "--align-path", "--refine", "1", "--copies-tsv", files["kcopies"]] + cbase, context=_FakeContext(_fake_genome(seq)))
    everything = open(files["all"]).read().splitlines()
    assert all(len(line.split("\t")) == 21 and re.fullmatch(r"(\d+[=XID])+", line.split("\t")[19]) for line in everything)
    cli.main([seq, "--chains-tsv", files["kept"], "--align-path", "--refine", "1", "--copies-tsv", files["kcopies"], "--min-aligned-identity", "0.99"] + cbase,
             context=_FakeContext(_fake_genome(seq)))
    kept = open(files["kept"]).read().splitlines()
    assert kept == [line for line in everything if float(line.split("\t")[17]) >= 0.99] and 0 < len(kept) < len(everything)
    assert {tuple(c.split("\t")[:4]) for c in open(files["kcopies"]).read().splitlines()} == {tuple(line.split("\t")[:4]) for line in kept}
    # ---- a repeat above a limit: '.' in the new columns as well
    monkeypatch.setattr(pn, "ALIGN_MAX_K", 10)
    cli.main([seq, "--chains-tsv", files["capped"], "--align-path", "--refine", "1"] + cbase, context=_FakeContext(_fake_genome(seq)))
    capped = open(files["capped"]).read().splitlines()
    wide = [int(line.split("\t")[3]) > 10 for line in plain]
    assert any(wide) and not all(wide)
    for line, full, w in zip(capped, everything, wide):
        assert line == ("\t".join(line.split("\t")[:13] + ["."] * 8) if w else full)
    monkeypatch.undo()
    # ---- --groups-tsv takes the same flags
    gbase = ["--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--max-shift", "4", "--min-group", "100", "--group-consensus", "--align"]
    cli.main([seq, "--groups-tsv", files["gplain"]] + gbase, context=_FakeContext(_fake_genome(seq)))
    cli.main([seq, "--groups-tsv", files["gcigar"], "--align-path"] + gbase, context=_FakeContext(_fake_genome(seq)))
    old, new = open(files["gplain"]).read().splitlines(), open(files["gcigar"]).read().splitlines()
    assert len(old) == len(new) >= 1
    for before, line in zip(old, new):
        f = before.split("\t")
        assert line == before + "\t" + pn.path_cigar(P.path_one(seq[int(f[1]):int(f[2])], f[10])[1], int(f[3]))
        if f[3] == "17":
            got = _cigar_counts(line.split("\t")[-1])
            assert (got["I"], got["D"]) == (2, 2)
