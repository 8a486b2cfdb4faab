"""CPU: the alignment of tandem repeats to their motifs (include/prf_align.h): the model (tests/align_model.py) against an
independent brute force and closed forms; the chain from the consensus models into it; prf_native.alignment_rows; the C ABI (what
is declared, bound and exported, and every refusal in its documented order, which needs no device); the binding's own checks; the
command line over a stand-in genome answered by the models; and the per-lane text of the kernel on the host, under the
sanitizers."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_model as A
import consensus_model as C
import periodchain_model as PC
import periodlink_model as PL
import phased_cases as K
import phased_model as M
from conftest import ROOT, load_jsonl_gz


# ---- the model against a brute force ----

def brute(seq, motif):
    """The definition: from every start column the motif written out 2 n + 1 letters long, a plain edit-distance table whose
    cells are tuples (edits, indels), no wrap; every number of consumed letters ends an alignment."""
    s, m = seq.upper(), motif.upper()
    n, k = len(s), len(m)
    best = None
    for a in range(k):
        text = "".join(m[(a + t) % k] for t in range(2 * n + 1))
        prev = [(c, c) for c in range(len(text) + 1)]                          # nothing of s against c letters: c deletions
        for i in range(1, n + 1):
            cur = [(prev[0][0] + 1, prev[0][1] + 1)]
            for c in range(1, len(text) + 1):
                hit = s[i - 1] == text[c - 1] and s[i - 1] in "ACGT"
                cur.append(min((prev[c - 1][0] + (0 if hit else 1), prev[c - 1][1]), (prev[c][0] + 1, prev[c][1] + 1),
                               (cur[c - 1][0] + 1, cur[c - 1][1] + 1)))
            prev = cur
        for c, (edits, indels) in enumerate(prev):
            cand = (edits, indels, c, (a + c - 1) % k)
            best = cand if best is None or cand < best else best
    edits, indels, consumed, end_column = best
    return edits, indels, consumed, (end_column + 1 - consumed) % k, end_column


def _cases(count, seed):
    rng = random.Random(seed)
    for case in range(count):
        k, n = rng.randint(1, 7), rng.randint(1, 14)
        motif = "".join(rng.choice("ACGTN" if case % 3 == 0 else "ACGT") for _ in range(k))
        if case % 5 == 4:
            motif = motif.lower() if case % 2 else motif[: k // 2] + motif[k // 2:].lower()
        if case % 2:
            seq = "".join(rng.choice("ACGTacgtN") for _ in range(n))
        else:                                                                  # the motif from a phase, with up to 3 planted edits
            phase = rng.randrange(k)
            body = [motif[(phase + t) % k].upper() for t in range(n + 3)]
            for _ in range(rng.randint(0, 3)):
                at, kind = rng.randrange(len(body)), rng.choice("SID")
                if kind == "S":
                    body[at] = rng.choice("ACGT")
                elif kind == "I":
                    body.insert(at, rng.choice("acgt"))
                elif len(body) > 1:
                    del body[at]
            seq = "".join(body)[:n]
            if case % 7 == 0:
                seq = seq.lower()
        yield seq, motif


def test_model_agrees_with_a_brute_force():
    n_cases = with_n = lower = gapped = 0
    for seq, motif in _cases(3_200, 211):
        got, want = A.align_one(seq, motif), brute(seq, motif)
        assert tuple(got) == want, (seq, motif)
        n_cases, with_n, lower, gapped = n_cases + 1, with_n + ("N" in motif.upper()), lower + (seq != seq.upper()), gapped + (want[1] > 0)
        assert want[2] >= 1 and want[1] <= want[0] <= len(seq)
    assert n_cases >= 3_000 and with_n > 300 and lower > 500 and gapped > 300


def test_closed_forms():
    rng = random.Random(212)
    for k in (1, 2, 3, 5, 7, 64, 65, 130):
        motif = ""
        while not motif or not K.primitive(motif):
            motif = "".join(rng.choice("ACGT") for _ in range(k))
        for phase in sorted({0, 1 % k, k - 1, rng.randrange(k)}):
            for n in (1, k, k + 1, 3 * k + 2):
                seq = "".join(motif[(phase + t) % k] for t in range(n))
                if k == 1 or n >= k:                                           # shorter than the motif: another phase may fit as well
                    assert A.align_one(seq, motif) == (0, 0, n, phase, (phase + n - 1) % k), (motif, phase, n)
                assert A.align_one(seq, motif)[:3] == (0, 0, n)
    for n in (1, 2, 9, 100):
        assert A.align_one("A" * n, "C") == (n, 0, n, 0, 0)
        assert A.align_one("A" * n, "N") == (n, 0, n, 0, 0) and A.align_one("N" * n, "N") == (n, 0, n, 0, 0)
        assert A.align_one("a" * n, "A") == (0, 0, n, 0, 0)
    # rotating the motif turns the columns and leaves the counts
    for seq, motif in _cases(300, 213):
        base = A.align_one(seq, motif)
        for turn in range(1, len(motif)):
            turned = A.align_one(seq, motif[turn:] + motif[:turn])
            assert turned[:3] == base[:3], (seq, motif, turn)
    # one inserted base, one deleted base
    assert A.align_one("ACGTACGTTACGTACGT", "ACGT") == (1, 1, 16, 0, 3)
    assert A.align_one("ACGTACGACGTACGT", "ACGT") == (1, 1, 16, 0, 3)
    assert A.align_one("ACGTACGTACCTACGT", "ACGT") == (1, 0, 16, 0, 3)
    with pytest.raises(ValueError, match="column 2"):
        A.motif_codes("ACRT")


def test_derived_counts():
    assert A.derived(17, 4, 1, 1, 16) == (0, 1, 0, 16, 16 / 17, 4.0)
    assert A.derived(15, 4, 1, 1, 16) == (0, 0, 1, 15, 15 / 16, 4.0)
    assert A.derived(16, 4, 1, 0, 16) == (1, 0, 0, 15, 15 / 16, 4.0)


def test_alignment_rows():
    import prf_native as pn
    seq = "ACGTACGTTACGTACGT" + "ACGTACGACGTACGT" + "GGGG"
    rows = np.zeros(3, dtype=pn.TANDEM_DTYPE)
    rows["start"], rows["end"], rows["k"], rows["matches"] = [0, 17, 32], [17, 32, 36], [4, 4, 1], [7, 8, 9]
    al = A.align(seq, rows, ["ACGT", "ACGT", "C"]).astype(pn.ALIGNMENT_DTYPE)
    out = pn.alignment_rows(rows, al)
    assert out.dtype.names == tuple(name for name, _ in pn.TANDEM_DTYPE) + tuple(name for name, _ in pn.ALIGNED_FIELDS)
    assert out["matches"].tolist() == [7, 8, 9] and out["edits"].tolist() == [1, 1, 4]
    assert out["subs"].tolist() == [0, 0, 4] and out["ins"].tolist() == [1, 0, 0] and out["del"].tolist() == [0, 1, 0]
    assert out["aligned_matches"].tolist() == [16, 15, 0]
    assert out["aligned_identity"].tolist() == [16 / 17, 15 / 16, 0.0] and out["aligned_copies"].tolist() == [4.0, 4.0, 4.0]
    for at in range(3):
        n = int(rows["end"][at] - rows["start"][at])
        assert tuple(out[at].tolist()[-6:]) == A.derived(n, int(rows["k"][at]), *al[at].tolist()[:3])
    groups = np.zeros(1, dtype=pn.TANDEM_GROUP_DTYPE)                         # the rows of tandem_groups name their k `period`
    groups["start"], groups["end"], groups["period"] = 0, 17, 4
    assert pn.alignment_rows(groups, al[:1])["aligned_copies"].tolist() == [4.0]
    with pytest.raises(ValueError, match="needs the rows motif_align returned"):
        pn.alignment_rows(rows, al[:2])
    with pytest.raises(ValueError, match="needs the rows motif_align returned"):
        pn.alignment_rows(rows[::-1], al)                                      # the counts do not fit the lengths
    assert len(pn.alignment_rows(rows[:0], al[:0])) == 0


# ---- the chains of the consensus products into the alignment ----

def test_edits_are_at_most_the_disagreements_with_the_consensus():
    """consensus_model -> align_model on the sequences of the dot-plot fixture: substituting every position that disagrees with
    its column's letter is one alignment, so edits <= (end - start) - agree."""
    cases = load_jsonl_gz(os.path.join(ROOT, "tests", "golden", "dotpair.jsonl.gz"))
    rng = random.Random(214)
    seen = strictly = 0
    for case in cases:
        for seq in (v for v in case.values() if isinstance(v, str) and len(v) >= 12 and re.fullmatch(r"[A-Za-z]+", v)):
            seq = seq[:160]
            rows = []
            for _ in range(3):
                k = rng.randint(1, 9)
                start = rng.randrange(len(seq) - 8)
                rows.append((start, min(len(seq), start + rng.randint(2, 6) * k + rng.randrange(k)), k))
            table = C.repeats(*rows)
            cons, motifs, _ = C.consensus(seq, table)
            al = A.align(seq, table, motifs)
            bound = (table["end"] - table["start"]).astype(np.int64) - cons["agree"].astype(np.int64)
            assert (al["edits"].astype(np.int64) <= bound).all(), (seq, rows)
            seen, strictly = seen + len(rows), strictly + int((al["edits"] < bound).sum())
    assert seen >= 300 and strictly > 0


def _lists(seq, period):
    import prf_native as pn
    kmax = period + 8
    chains = PC.chains(seq, 1, kmax, K.MIN_SEED[period], K.MAX_GAP).astype(pn.PCHAIN_DTYPE)
    links = PL.links(seq, 1, kmax, K.MIN_SEED[period], K.MAX_GAP, K.MAX_SHIFT).astype(pn.PLINK_DTYPE)
    return chains, links


@pytest.mark.parametrize("kind", ["ins", "del", "both"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("period", [7, 17, 40])
def test_a_planted_gapped_repeat_aligns_with_its_indels(period, d, kind):
    """The models of DESIGN 16, 17 and 19 on the planted inputs, then the whole group against the motif of its piece: an insertion
    or a deletion of d bases among s substitutions gives indels == d and edits <= s + d (both: 2 d), and the aligned identity
    lies strictly above the ungapped consensus identity of the same (start, end, P)."""
    import prf_native as pn
    motif, seq = K.planted(period, d, kind)
    chains, links = _lists(seq, period)
    groups = pn.join_period_chains(chains, links)
    at = K.body_group(groups, period, len(seq))
    pieces, segments = pn.group_segments(chains, links)
    cons, motifs, _ = M.consensus(seq, pieces["k"].tolist(), segments)
    rows, names = pn.group_consensus_rows(groups, pieces, cons.astype(pn.CONSENSUS_DTYPE), motifs)
    start, end = int(groups["start"][at]), int(groups["end"][at])
    al = A.align(seq, A.repeats((start, end, period)), [names[at]])
    planted = d * (2 if kind == "both" else 1)
    assert al["indels"][0] == planted and al["edits"][0] <= K.SUBSTITUTIONS + planted
    full = pn.alignment_rows(groups[at:at + 1][["start", "end", "period"]], al.astype(pn.ALIGNMENT_DTYPE))[0]
    assert full["ins"] == (d if kind != "del" else 0) and full["del"] == (d if kind != "ins" else 0)
    flat, _, _ = C.consensus(seq, C.repeats((start, end, period)))
    assert full["aligned_identity"] > flat["agree"][0] / (end - start)
    assert abs(full["aligned_copies"] - (end - start - full["ins"] + full["del"]) / period) < 1e-12


# ---- the per-lane text of the kernel, on the host ----

def test_lane_text_against_a_plain_recurrence_on_the_host(tmp_path):
    """csrc/align_word.h is the text the kernel runs; the stand-alone program checks the deal of the columns for every k, the
    packing at the limits, the sentinel, the tie rule, the host's sort, and 64 emulated lanes against the recurrence on explicit
    triples in every kernel's range of k, under the sanitizers.  Nothing is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/align_word_check.cpp")
    exe = tmp_path / "align_word_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "align_word_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, deals, rows, cells = done.stdout.split()
    assert word == "ok" and int(deals) == 1_024 and int(rows) == 260 and int(cells) > 1_000_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_align.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.ALIGN_EXPORTS) == ["prf_motif_align", "prf_motif_align_seq"]     # no _ex form: no knob to turn
    older = (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS) |
             set(pn.DOTCHAIN_EXPORTS) | set(pn.DOTLINK_EXPORTS) | set(pn.PERIODCHAIN_EXPORTS) | set(pn.PERIODLINK_EXPORTS) |
             set(pn.CONSENSUS_EXPORTS) | set(pn.PHASED_EXPORTS))
    assert not set(declared) & older
    header = open(os.path.join(ROOT, "include", "prf.h")).read()
    assert header.count('#include "prf_align.h"') == 1 and header.index('#include "prf_align.h"') < header.index("#ifdef __cplusplus\n}")
    assert header.index('#include "prf_phased.h"') < header.index('#include "prf_align.h"')
    assert all(hasattr(lib, name) and getattr(lib, name).argtypes for name in declared)
    raw = ctypes.CDLL(pn.LIB_PATH)                                             # exported: the loader finds them by name
    assert all(hasattr(raw, name) for name in declared) and not hasattr(raw, "prf_motif_align_ex")
    assert lib.prf_abi_version() == 4
    assert int(re.search(r"#define PRF_ALIGN_MAX_K (\d+)u", text)[1]) == pn.ALIGN_MAX_K == A.MAX_K == 1_024
    found = re.search(r"#define PRF_ALIGN_MAX_LEN \((\d+)ull << (\d+)\)", text)
    assert int(found[1]) << int(found[2]) == pn.ALIGN_MAX_LEN == A.MAX_LEN == 1 << 19
    assert np.dtype(pn.ALIGNMENT_DTYPE).itemsize == 24 and pn.ALIGNMENT_DTYPE == A.DTYPE
    struct = re.search(r"typedef struct prf_alignment \{(.*?)\} prf_alignment;", text, flags=re.S)[1]
    assert re.findall(r"\b(\w+);", struct) == list(A.FIELDS) and re.findall(r"\b(uint\d+_t)\b", struct) == ["uint32_t"] * 6
    # the two headers in front and their declarations stay as they are
    for name, exports in (("prf_consensus.h", pn.CONSENSUS_EXPORTS), ("prf_phased.h", pn.PHASED_EXPORTS)):
        older_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", older_text))) == sorted(exports)


ROWS = ((0, 12, 3),)


def _call(lib, pn, form, seq=b"ACGTACGTACGT", span=(0, 12), rows=ROWS, n_rows=None, motifs=b"ACG", length=None, dst=True, reserved=0):
    table = np.zeros(max(1, len(rows or ())), dtype=pn.REPEAT_DTYPE)
    for at, row in enumerate(rows or ()):
        table[at] = tuple(row) + (reserved if at == len(rows) - 1 else 0,)
    out = np.full(64 * 24, 0xAB, dtype=np.uint8)
    stats = pn.ScanStats()
    stats.n_hits = 77
    tail = (*span, table.ctypes.data if rows is not None else None, len(rows or ()) if n_rows is None else n_rows, motifs,
            len(motifs or b"") if length is None else length, out.ctypes.data if dst else None, ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_motif_align_seq(None, arr, *tail)
    else:
        rc = lib.prf_motif_align(None, None, 0, *tail)
    assert (out == 0xAB).all() and stats.n_hits == 77                          # a refused call writes nothing
    return rc


LONG = (1 << 19) + 1
# each case breaks one rule and, where a call can, the rules behind it: the first in the documented order is the one reported
ORDER = [
    (dict(span=(7, 3), n_rows=(1 << 24) + 1, rows=None, motifs=None, dst=False), "PRF_EINVAL", "begin 7"),
    (dict(n_rows=(1 << 24) + 1, rows=None, motifs=None, dst=False), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_ROWS"),
    (dict(rows=None, n_rows=1, motifs=None, dst=False), "PRF_EINVAL", "NULL rows"),
    (dict(rows=((0, 12, 0),), motifs=None, dst=False), "PRF_EINVAL", "NULL motifs"),
    (dict(rows=((0, 12, 0),), dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(rows=((0, 12, 3), (5, 5, 0), (0, 12, 2_000)), length=0), "PRF_EINVAL", "row 1: k is 0"),
    (dict(rows=((0, 12, 3), (5, 5, 2_000)), reserved=9, length=0), "PRF_EINVAL", "row 1: start 5 is not in front of end 5"),
    (dict(rows=((0, 12, 3), (0, LONG, 2_000)), reserved=9, length=0), "PRF_EINVAL", "row 1: reserved is 9"),
    (dict(rows=((0, 12, 3), (0, LONG, 1_025), (0, 0, 0)), length=0), "PRF_EUNSUPPORTED", "row 1: k = 1025 is above 1024 (PRF_ALIGN_MAX_K)"),
    (dict(rows=((0, 12, 3), (7, 7 + LONG, 1_024), (0, 0, 0)), length=0), "PRF_EUNSUPPORTED", "row 1: 524289 positions are above 524288 (PRF_ALIGN_MAX_LEN)"),
    (dict(rows=((0, 12, 3), (7, 6 + LONG, 1_024)), length=1_026, motifs=b"ACR" + b"A" * 1_024), "PRF_EINVAL", "holds 1026 letters, the k of the rows add up to 1027"),
    (dict(rows=((0, 12, 3), (0, 13, 4)), motifs=b"ACGAC-T"), "PRF_EINVAL", "row 1: column 2 of the motif is the byte 0x2d"),
    (dict(rows=((0, 13, 3),), motifs=b"ARG"), "PRF_EINVAL", "row 0: column 1 of the motif is the byte 0x52"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(rows=((0, 12, 3), (2, 9, 4)), motifs=b"acgNnTG", length=9), "PRF_EINVAL", "NULL context"),    # either case, N, room to spare
    (dict(rows=((0, 1 << 19, 1_024),), motifs=b"A" * 1_024, span=(0, 1 << 63)), "PRF_EINVAL", "NULL context"),   # the limits themselves pass
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    if form == "one_shot" and kwargs.get("span") == (0, 1 << 63):             # the one-shot form knows the length: a sequence that holds the row
        kwargs = dict(kwargs, seq=b"A" * (1 << 19))
    rc = _call(lib, pn, form, **kwargs)
    message = lib.prf_last_error().decode()
    assert rc == getattr(pn, code), message
    assert text in message and message.startswith("prf_motif_align")


def test_the_letter_limit_is_judged_before_the_letters():
    pn, lib = _lib()
    rows = tuple((0, 12, 1_024) for _ in range((1 << 16) + 1))
    assert _call(lib, pn, "genome", rows=rows, motifs=b"-", length=1 << 40) == pn.PRF_EUNSUPPORTED
    assert "PRF_CONSENSUS_MAX_LETTERS" in lib.prf_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(rows=((0, 12, 3), (0, 13, 4)), motifs=b"ACGACGT"), "PRF_EINVAL", "row 1: end 13 is behind the range's 12 positions"),
    (dict(rows=((0, 9, 3), (2, 10, 3)), motifs=b"ACGACG", span=(3, 12)), "PRF_EINVAL", "row 1: end 10 is behind the range's 9 positions"),
    (dict(rows=((0, 13, 3),), seq=b"ACGT-ACGTACG"), "PRF_EINVAL", "row 0: end 13"),           # the rows are judged before the bytes
    (dict(seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(rows=((0, 1, 3),), seq=b""), "PRF_EINVAL", "row 0: end 1 is behind the range's 0 positions"),
    (dict(span=(2, 1 << 63), rows=((0, 10, 3),)), "PRF_EINVAL", "NULL context"),              # ends are clipped
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


@pytest.mark.parametrize("form", ["genome", "one_shot"])
def test_no_rows_is_no_work_and_no_error(form):
    pn, lib = _lib()
    assert _call(lib, pn, form, rows=None, n_rows=0, motifs=None, dst=False) == pn.PRF_OK
    assert _call(lib, pn, form, rows=(), motifs=b"") == pn.PRF_OK
    assert _call(lib, pn, form, rows=(), span=(7, 3)) == pn.PRF_EINVAL          # ... but the range is still judged
    rc = lib.prf_motif_align_seq(None, None, 0, 4, None, 0, None, 0, None, None)
    assert rc == pn.PRF_OK


def test_a_missing_sequence_is_refused():
    pn, lib = _lib()
    table, out = A.repeats((0, 4, 2)), np.zeros(1, dtype=pn.ALIGNMENT_DTYPE)
    rc = lib.prf_motif_align_seq(None, None, 0, 4, table.ctypes.data, 1, b"AC", 2, out.ctypes.data, None)
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 2, [100, 50])
    ok = A.repeats((0, 10, 3))
    with pytest.raises(ValueError, match="contig 2"):
        g.motif_align(2, 0, None, ok, ["ACG"])
    with pytest.raises(ValueError, match="begin"):
        g.motif_align(0, 30, 20, ok, ["ACG"])
    with pytest.raises(ValueError, match="fields start, end and k"):
        g.motif_align(0, 0, None, [(0, 10, 3)], ["ACG"])
    with pytest.raises(ValueError, match="repeat 1: k must be at least 1"):
        g.motif_align(0, 0, None, A.repeats((0, 10, 3), (0, 10, 0)), ["ACG", ""])
    with pytest.raises(ValueError, match=r"repeat 0: \[5, 5\)"):
        g.motif_align(0, 0, None, A.repeats((5, 5, 3)), ["ACG"])
    with pytest.raises(ValueError, match=r"repeat 1: \[0, 51\) is not a stretch of the range's 50 positions"):
        g.motif_align(1, 0, None, A.repeats((0, 50, 3), (0, 51, 3)), ["ACG", "ACG"])
    with pytest.raises(ValueError, match=r"repeat 1: k = 1025 is more than an alignment takes \(1024\)"):
        g.motif_align(0, 0, None, A.repeats((0, 50, 3), (0, 50, 1_025)), ["ACG", "A" * 1_025])
    big = pn.Genome(None, None, 1, [1 << 20])
    with pytest.raises(ValueError, match=r"repeat 0: 524289 positions are more than an alignment takes \(524288\)"):
        big.motif_align(0, 0, None, A.repeats((1, (1 << 19) + 2, 3)), ["ACG"])
    with pytest.raises(ValueError, match="2 motifs for 1 repeats"):
        g.motif_align(0, 0, None, ok, ["ACG", "ACG"])
    with pytest.raises(ValueError, match="repeat 0: the motif has 4 letters, k is 3"):
        g.motif_align(0, 0, None, ok, ["ACGT"])
    with pytest.raises(ValueError, match="the motifs hold 4 letters, the k of the repeats add up to 3"):
        g.motif_align(0, 0, None, ok, "ACGT")
    with pytest.raises(ValueError, match="the motifs hold 2 letters"):
        g.motif_align(0, 0, None, ok, b"AC")
    with pytest.raises(ValueError, match="motifs must be a list of str"):
        g.motif_align(0, 0, None, ok, [3])
    g._h = big._h = None
    # the one path of the repeats' checks: period_consensus says the same of the same rows
    g = pn.Genome(None, None, 2, [100, 50])
    for call in (lambda r: g.period_consensus(1, 0, None, r), lambda r: g.motif_align(1, 0, None, r, ["ACG", "ACG"])):
        with pytest.raises(ValueError, match=r"repeat 1: \[0, 51\) is not a stretch of the range's 50 positions"):
            call(A.repeats((0, 50, 3), (0, 51, 3)))
    g._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_input(args, parser), args


def test_cli_parses_the_align_options(capsys):
    import plot_periodicity_matrix as cli
    chains = ["ACGTACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2"]
    groups = ["ACGTACGT", "--groups-tsv", "g.tsv", "--min-seed", "4", "--max-gap", "2", "--max-shift", "2"]
    args = _parse(cli, chains + ["--consensus"])[1]
    assert (args.align, args.min_aligned_identity) == (False, None)
    args = _parse(cli, chains + ["--consensus", "--align", "--min-aligned-identity", "0.8"])[1]
    assert (args.align, args.min_aligned_identity) == (True, 0.8)
    assert _parse(cli, groups + ["--group-consensus", "--align"])[1].align
    capsys.readouterr()
    for argv, text in ((chains + ["--align"], "--align needs the motifs"),
                       (groups + ["--align"], "--align needs the motifs"),
                       (["ACGT", "--align"], "--align needs the motifs"),
                       (chains + ["--consensus", "--min-aligned-identity", "0.5"], "belongs to --align"),
                       (chains + ["--consensus", "--align", "--min-aligned-identity", "1.5"], "0 .. 1"),
                       (groups + ["--group-consensus", "--align", "--min-aligned-identity", "-0.1"], "0 .. 1")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


class _FakeGenome:
    """What list_chains and list_groups ask of a resident genome, answered by the models."""

    def __init__(self, seq):
        self.seq, self.calls = seq, []

    def period_chains(self, contig, begin, end, kmin, kmax, min_seed, max_gap, min_len, n_matches, positions):
        import prf_native as pn
        self.calls.append("chains")
        return PC.chains(self.seq, kmin, kmax, min_seed, max_gap, n_matches, min_len, begin, end, positions).astype(pn.PCHAIN_DTYPE)

    def period_links(self, contig, begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches, positions):
        import prf_native as pn
        self.calls.append("links")
        return PL.links(self.seq, kmin, kmax, min_seed, max_gap, max_shift, n_matches, begin, end, positions).astype(pn.PLINK_DTYPE)

    def period_consensus(self, contig, begin, end, repeats):
        import prf_native as pn
        self.calls.append(("consensus", len(repeats)))
        rows, motifs, _ = C.consensus(self.seq, repeats, begin, end)
        return rows.astype(pn.CONSENSUS_DTYPE), motifs

    def phased_consensus(self, contig, begin, end, ks, segments):
        import prf_native as pn
        self.calls.append(("phased", len(ks), len(segments)))
        rows, motifs, _ = M.consensus(self.seq, ks, segments, begin, end)
        return rows.astype(pn.CONSENSUS_DTYPE), motifs

    def motif_align(self, contig, begin, end, repeats, motifs):
        import prf_native as pn
        assert repeats["k"].max() <= pn.ALIGN_MAX_K and (repeats["end"] - repeats["start"]).max() <= pn.ALIGN_MAX_LEN
        self.calls.append(("align", len(repeats)))
        return A.align(self.seq, repeats, motifs, begin, end).astype(pn.ALIGNMENT_DTYPE)

    def free(self):
        self.calls.append("free")


class _FakeContext:
    def __init__(self, genome):
        self.genome = genome

    def load(self, seqs, kmax_hint):
        return self.genome


def _columns(seq, start, end, k, motif):
    al = A.align_one(seq[start:end], motif)
    subs, ins, dele, _, identity, copies = A.derived(end - start, k, *al[:3])
    return [str(al[0]), str(subs), str(ins), str(dele), f"{identity:.4f}", f"{copies:.2f}"]


def test_cli_lines_with_and_without_align(tmp_path, monkeypatch):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    motif, body = K.planted(17, 2, "both")
    seq = body + K.planted(7, 1, "ins")[1]
    files = {name: str(tmp_path / f"{name}.tsv") for name in ("groups", "galigned", "gkept", "chains", "caligned", "ckept", "split", "capped")}
    gbase = ["--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--max-shift", "4", "--min-group", "100", "--group-consensus"]
    # ---- --groups-tsv: without --align the file is what it was and nothing is aligned
    genome = _FakeGenome(seq)
    cli.main([seq, "--groups-tsv", files["groups"]] + gbase, context=_FakeContext(genome))
    assert not [c for c in genome.calls if c[0] == "align"]
    genome = _FakeGenome(seq)
    cli.main([seq, "--groups-tsv", files["galigned"], "--align"] + gbase, context=_FakeContext(genome))
    old, new = open(files["groups"]).read().splitlines(), open(files["galigned"]).read().splitlines()
    assert len(old) == len(new) >= 1 and genome.calls[-2:] == [("align", len(old)), "free"]
    seventeen = 0
    for before, line in zip(old, new):
        assert line.startswith(before + "\t")
        f = before.split("\t")
        assert line[len(before) + 1:].split("\t") == _columns(seq, int(f[1]), int(f[2]), int(f[3]), f[10])
        if f[3] == "17":
            seventeen += 1
            more = line[len(before) + 1:].split("\t")
            assert more[2:4] == ["2", "2"] and int(more[0]) <= 4 + K.SUBSTITUTIONS and float(more[4]) > float(f[11]) * float(f[15])
    assert seventeen == 1
    cli.main([seq, "--groups-tsv", files["gkept"], "--align", "--min-aligned-identity", "0.9999"] + gbase, context=_FakeContext(_FakeGenome(seq)))
    assert open(files["gkept"]).read().splitlines() == [line for line in new if float(line.split("\t")[-2]) >= 0.9999]
    # ---- --chains-tsv: each repeat against its own consensus
    cbase = ["--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--consensus"]
    cli.main([seq, "--chains-tsv", files["chains"]] + cbase, context=_FakeContext(_FakeGenome(seq)))
    genome = _FakeGenome(seq)
    cli.main([seq, "--chains-tsv", files["caligned"], "--align"] + cbase, context=_FakeContext(genome))
    old, new = open(files["chains"]).read().splitlines(), open(files["caligned"]).read().splitlines()
    assert len(old) == len(new) >= 3 and genome.calls[-2:] == [("align", len(old)), "free"]
    for before, line in zip(old, new):
        f = before.split("\t")
        assert line.startswith(before + "\t") and line[len(before) + 1:].split("\t") == _columns(seq, int(f[1]), int(f[2]), int(f[3]), f[9])
        assert re.fullmatch(r"\d\.\d{4}", line.split("\t")[-2]) and re.fullmatch(r"\d+\.\d{2}", line.split("\t")[-1])
    cli.main([seq, "--chains-tsv", files["ckept"], "--align", "--min-aligned-identity", "0.99"] + cbase, context=_FakeContext(_FakeGenome(seq)))
    kept = open(files["ckept"]).read().splitlines()
    assert kept == [line for line in new if float(line.split("\t")[-2]) >= 0.99] and 0 < len(kept) < len(new)
    # ---- batches: with room for one row per call every repeat goes alone, and the lines are the same
    monkeypatch.setattr(pn, "CONSENSUS_MAX_ROWS", 1)
    genome = _FakeGenome(seq)
    cli.main([seq, "--chains-tsv", files["split"], "--align"] + cbase, context=_FakeContext(genome))
    assert [c for c in genome.calls if c[0] == "align"] == [("align", 1)] * len(old) and open(files["split"]).read().splitlines() == new
    monkeypatch.undo()
    # ---- a repeat above a limit: '.' in the six columns, dropped when the filter is given
    monkeypatch.setattr(pn, "ALIGN_MAX_K", 10)
    genome = _FakeGenome(seq)
    cli.main([seq, "--chains-tsv", files["capped"], "--align"] + cbase, context=_FakeContext(genome))
    capped = open(files["capped"]).read().splitlines()
    wide = [int(line.split("\t")[3]) > 10 for line in old]
    assert any(wide) and not all(wide)
    assert capped == [before + "\t.\t.\t.\t.\t.\t." if w else line for before, line, w in zip(old, new, wide)]
    cli.main([seq, "--chains-tsv", files["capped"], "--align", "--min-aligned-identity", "0.0"] + cbase, context=_FakeContext(_FakeGenome(seq)))
    assert open(files["capped"]).read().splitlines() == [line for line, w in zip(new, wide) if not w]
