"""CPU: the local alignment of windows around tandem repeats to their motifs (include/prf_alignlocal.h): the model
(tests/alignlocal_model.py) against the brute force over tuples and closed forms; against the global alignment of DESIGN 20; the
planted inputs of tests/phased_cases.py through the chain of models; prf_native.flank_repeats and local_rows; the C ABI (what is
declared, bound and exported, and every refusal in its documented order, which needs no device); the binding's own checks; the
command line over a stand-in genome answered by the models; and the per-lane text of the kernel on the host, under the
sanitizers."""
import ctypes
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_model as A
import alignlocal_model as L
import phased_cases as K
import phased_model as M
from conftest import ROOT
from test_align_cpu import _FakeContext, _FakeGenome, _lists

TRF = (2, 7, 7)


# ---- the model against the brute force ----

def _cases(count, seed):
    rng = random.Random(seed)
    for case in range(count):
        k, n = rng.randint(1, 5), rng.randint(1, 11)
        alphabet = ("A", "AC", "ACGT", "ACGTN")[case % 4]
        motif = "".join(rng.choice(alphabet) for _ in range(k))
        if case % 5 == 4:
            motif = motif.lower() if case % 2 else motif[: k // 2] + motif[k // 2:].lower()
        if case % 2:
            seq = "".join(rng.choice(alphabet + alphabet.lower()) for _ in range(n))
        else:                                                                  # a flank, the motif from a phase with up to 3 edits, a flank
            phase = rng.randrange(k)
            body = [motif[(phase + t) % k].upper() for t in range(n + 3)]
            for _ in range(rng.randint(0, 3)):
                at, kind = rng.randrange(len(body)), rng.choice("SID")
                if kind == "S":
                    body[at] = rng.choice(alphabet)
                elif kind == "I":
                    body.insert(at, rng.choice(alphabet.lower()))
                elif len(body) > 1:
                    del body[at]
            flank = rng.randint(0, 3)
            seq = ("".join(rng.choice("ACGT") for _ in range(flank)) + "".join(body))[:max(1, n - flank)] + "".join(rng.choice("ACGT") for _ in range(flank))
            seq = seq[:n]
            if case % 7 == 0:
                seq = seq.lower()
        yield seq, motif, L.WEIGHTS[rng.randrange(len(L.WEIGHTS))]


def test_model_agrees_with_the_brute_force():
    n_cases = zero = lower = two = 0
    seen = set()
    for seq, motif, weights in _cases(3_200, 221):
        want = L.brute(seq, motif, weights)
        assert L.one_triples(seq, motif, weights) == want, (seq, motif, weights)
        assert L.one(seq, motif, weights) == want, (seq, motif, weights)
        n_cases, zero, lower = n_cases + 1, zero + (want[0] == 0), lower + (seq != seq.upper())
        two += len(set(motif.upper())) <= 2
        seen.add(weights)
        assert want == (0, 0, 0, 0, 0) or (want[0] >= weights[0] and 0 <= want[1] < want[2] <= len(seq) and max(want[3:]) < len(motif))
    assert n_cases >= 3_000 and zero > 20 and lower > 500 and two > 1_000 and seen == set(L.WEIGHTS)


def _primitive_acg(k, rng):
    motif = ""
    while not motif or not K.primitive(motif):
        motif = "".join(rng.choice("ACG") for _ in range(k))
    return motif


def test_closed_forms():
    """Flanks of T against a primitive motif over A, C, G: the flanks match nothing."""
    rng = random.Random(222)
    for k in (1, 2, 3, 5, 7, 64, 65, 130):
        motif = _primitive_acg(k, rng)
        for phase in sorted({0, 1 % k, k - 1, rng.randrange(k)}):
            for copies_len in (k, k + 1, 3 * k + 2):
                for flank in (0, 1, 9):
                    body = "".join(motif[(phase + t) % k] for t in range(copies_len))
                    for weights in (TRF, (1, 16, 16), (16, 1, 1)):
                        got = L.one("T" * flank + body + "T" * (flank + 2), motif, weights)
                        assert got == (weights[0] * copies_len, flank, flank + copies_len, phase, (phase + copies_len - 1) % k), (motif, phase, copies_len)
                        turn = 1 + phase % k                                   # rotating the motif leaves score, first and end
                        assert L.one("T" * flank + body + "T" * (flank + 2), motif[turn % k:] + motif[:turn % k], weights)[:3] == got[:3]
    # one substitution at offset d from the left edge, the right side longer than the left: kept iff match * d > mismatch
    motif = _primitive_acg(7, rng)
    for weights in (TRF, (2, 3, 5), (3, 1, 2), (1, 1, 1)):
        match, mismatch, _ = weights
        for d in range(1, 12):
            n = 40
            body = list((motif * 8)[:n])
            body[d] = "T"
            got = L.one("TTT" + "".join(body) + "TT", motif, weights)
            right = n - d - 1
            if match * d > mismatch:
                assert got == (match * (n - 1) - mismatch, 3, 3 + n, 0, (n - 1) % 7), (weights, d, got)
            else:
                assert got == (match * right, 3 + d + 1, 3 + n, (d + 1) % 7, (n - 1) % 7), (weights, d, got)
            for turn in range(1, 7):
                assert L.one("TTT" + "".join(body) + "TT", motif[turn:] + motif[:turn], weights)[:3] == got[:3], (weights, d, turn)
    # nothing matches: the zero row
    for n in (1, 2, 9, 100):
        assert L.one("N" * n, "ACG", TRF) == (0, 0, 0, 0, 0) and L.one("A" * n, "N", TRF) == (0, 0, 0, 0, 0)
        assert L.one("N" * n, "N", TRF) == (0, 0, 0, 0, 0) and L.one("T" * n, "ACG", (16, 1, 1)) == (0, 0, 0, 0, 0)
        assert L.one("a" * n, "A", TRF) == (2 * n, 0, n, 0, 0)
    # ... on any input it leaves score and end; where two alignments of one score end at one position in different columns, the
    # least end column decides, which a rotation renames, and `first` may follow ('AcCacCAaC' against CCCCA and CCCAC)
    moved = 0
    for seq, motif, weights in _cases(300, 223):
        base = L.one(seq, motif, weights)
        for turn in range(1, len(motif)):
            turned = L.one(seq, motif[turn:] + motif[:turn], weights)
            assert (turned[0], turned[2]) == (base[0], base[2]), (seq, motif, turn)
            moved += turned[1] != base[1]
    assert moved < 30
    # one inserted base, one deleted base, and an edit so near the edge that it is trimmed
    assert L.one("TTACGTACGTTACGTACGTTT", "ACG", (2, 7, 3)) == L.brute("TTACGTACGTTACGTACGTTT", "ACG", (2, 7, 3))
    assert L.one("ACGACGACGTACGACGACG", "ACG", (2, 7, 3)) == (2 * 18 - 3, 0, 19, 0, 2)
    assert L.one("ACGACGACACGACGACG", "ACG", (2, 7, 3)) == (2 * 17 - 3, 0, 17, 0, 2)
    assert L.one("ATTACGACGACG", "ACG", TRF) == (2 * 9, 3, 12, 0, 2)


def test_the_score_is_at_least_that_of_the_global_alignment():
    """For every case: the global alignment (unit costs) of the refined interval, and of the whole window, is one
    alignment among those the local one chooses from."""
    strictly = seen = 0
    for seq, motif, weights in _cases(1_200, 224):
        score, first, end = L.one(seq, motif, weights)[:3]
        n = len(seq)
        edits, indels, consumed = A.align_one(seq, motif)[:3]
        subs, ins, dele, matches = A.derived(n, len(motif), edits, indels, consumed)[:4]
        whole = max(0, L.bound(weights, subs, ins, dele, matches))
        assert score >= whole, (seq, motif, weights)
        if score:
            edits, indels, consumed = A.align_one(seq[first:end], motif)[:3]
            subs, ins, dele, matches = A.derived(end - first, len(motif), edits, indels, consumed)[:4]
            assert score >= L.bound(weights, subs, ins, dele, matches), (seq, motif, weights)
            seen += 1
        strictly += score > whole
    assert seen > 800 and strictly > 100


# ---- the planted inputs through the chain of models ----

@pytest.mark.parametrize("kind", ["ins", "del", "both"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("period", [7, 17, 40])
def test_a_planted_gapped_repeat_is_refined_to_its_body(period, d, kind):
    """The models of DESIGN 16, 17 and 19 on the planted inputs, then the group's [start, end) padded by 50 against the motif of its
    chosen piece at (2, 7, 7): the refined interval holds the planted body [FLANK, n - FLANK).
    ONE INPUT DOES NOT: (7, 2, "del") plants one of its four substitutions on the third position from the body's right end (the
    body ends ...TTTC TTC where the motif TTTCCTC has ...TTTC CTC).  The two matches behind it are worth 4, the substitution costs
    7: the closed form of test_closed_forms (kept iff match * d > mismatch, here 2 * 2 < 7) trims those three positions, and the
    refined interval ends exactly there.  The claim stands for the other 26."""
    import prf_native as pn
    motif, seq = K.planted(period, d, kind)
    n = len(seq)
    chains, links = _lists(seq, period)
    groups = pn.join_period_chains(chains, links)
    at = K.body_group(groups, period, n)
    pieces, segments = pn.group_segments(chains, links)
    cons, motifs, _ = M.consensus(seq, pieces["k"].tolist(), segments)
    _rows, names = pn.group_consensus_rows(groups, pieces, cons.astype(pn.CONSENSUS_DTYPE), motifs)
    rows = groups[at:at + 1][["start", "end", "period"]]
    windows, sent = pn.flank_repeats(rows, 50, n)
    assert sent.all() and windows["k"][0] == period and windows["start"][0] == 0 and windows["end"][0] == n
    local = L.local(seq, windows, [names[at]], TRF)
    out = pn.local_rows(rows, windows, local.astype(pn.LOCAL_ALIGNMENT_DTYPE))[0]
    first, end = int(out["local_start"]), int(out["local_end"])
    if (period, d, kind) == (7, 2, "del"):
        assert seq[n - K.FLANK - 3] != (motif * 40)[n - K.FLANK - 3 - K.FLANK + d] and first <= K.FLANK and end == n - K.FLANK - 3
    else:
        assert first <= K.FLANK and end >= n - K.FLANK, (period, d, kind, first, end)
    indels = d * (2 if kind == "both" else 1)
    assert out["score"] >= 2 * (end - first - K.SUBSTITUTIONS - indels) - 7 * (K.SUBSTITUTIONS + indels) - 2 * 7 * 2    # two flank positions at most
    # the composition: the global alignment of the refined interval
    edits, n_indels, _ = A.align_one(seq[first:end], names[at])[:3]
    assert n_indels == indels and edits <= K.SUBSTITUTIONS + indels + 2


# ---- flank_repeats and local_rows ----

def test_flank_repeats_and_local_rows(monkeypatch):
    import prf_native as pn
    rows = np.zeros(5, dtype=pn.TANDEM_DTYPE)
    rows["start"], rows["end"], rows["k"] = [0, 30, 960, 100, 100], [20, 90, 1_000, 200, 200], [3, 7, 5, 2_000, 4]
    windows, sent = pn.flank_repeats(rows, 50, 1_000)
    assert windows.dtype == np.dtype(pn.REPEAT_DTYPE) and sent.tolist() == [True, True, True, False, True]
    assert windows["start"].tolist() == [0, 0, 910, 100, 50] and windows["end"].tolist() == [70, 140, 1_000, 200, 250]      # clipped at 0 and at n
    assert windows["k"].tolist() == [3, 7, 5, 2_000, 4]
    assert pn.flank_repeats(rows, 0, 1_000)[0]["start"].tolist() == rows["start"].tolist()
    groups = np.zeros(1, dtype=pn.TANDEM_GROUP_DTYPE)                          # the rows of tandem_groups name their k `period`
    groups["start"], groups["end"], groups["period"] = 60, 90, 17
    assert pn.flank_repeats(groups, 10, 95)[0].tolist() == [(50, 95, 17, 0)]
    # the flank is cut to what fits the length limit; a row above it is not sent
    monkeypatch.setattr(pn, "ALIGN_MAX_LEN", 120)
    windows, sent = pn.flank_repeats(rows, 50, 1_000)
    assert sent.tolist() == [True, True, True, False, True]
    assert (windows["end"] - windows["start"]).max() <= 120
    assert windows[1].tolist() == (0, 120, 7, 0) and windows[4].tolist() == (90, 210, 4, 0) and windows[0].tolist() == (0, 70, 3, 0)
    rows["end"][4] = 221
    windows, sent = pn.flank_repeats(rows, 50, 1_000)
    assert not sent[4] and windows[4].tolist() == (100, 221, 4, 0)
    rows["end"][4] = 219                                                       # one position of room: in front
    assert pn.flank_repeats(rows, 50, 1_000)[0][4].tolist() == (99, 219, 4, 0)
    monkeypatch.undo()
    with pytest.raises(ValueError, match=r"repeat 2: \[960, 1000\) is not a stretch of the range's 999 positions"):
        pn.flank_repeats(rows, 5, 999)
    with pytest.raises(ValueError, match="flank"):
        pn.flank_repeats(rows, -1, 1_000)
    # local_rows
    rows["end"][4] = 200
    windows, sent = pn.flank_repeats(rows, 50, 1_000)
    local = np.zeros(5, dtype=pn.LOCAL_ALIGNMENT_DTYPE)
    local["score"], local["first"], local["end"] = [40, 0, 33, 0, 9], [0, 5, 45, 0, 60], [25, 9, 90, 0, 140]
    out = pn.local_rows(rows, windows, local)
    assert out.dtype.names == tuple(name for name, _ in pn.TANDEM_DTYPE) + ("local_start", "local_end", "score")
    assert out["local_start"].tolist() == [0, 30, 955, 100, 110] and out["local_end"].tolist() == [25, 90, 1_000, 200, 190]
    assert out["score"].tolist() == [40, 0, 33, 0, 9] and out["start"].tolist() == rows["start"].tolist()
    with pytest.raises(ValueError, match="needs the windows of these rows"):
        pn.local_rows(rows, windows[:4], local)
    local["end"][2] = 91                                                       # behind the window
    with pytest.raises(ValueError, match="needs the windows of these rows"):
        pn.local_rows(rows, windows, local)
    assert len(pn.local_rows(rows[:0], windows[:0], local[:0])) == 0


# ---- the per-lane text of the kernel, on the host ----

def test_lane_text_against_the_recurrence_on_the_host(tmp_path):
    """csrc/alignlocal_word.h is the text the kernel runs; the stand-alone program checks the packing at the field maxima, the
    saturating subtraction at score == w and w + 1, the stale labels of the prefix pass, the order of the best key, and 64
    emulated lanes against the recurrence on explicit triples in every kernel's range of k, under the sanitizers.  Nothing is
    loaded into this process."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/alignlocal_word_check.cpp")
    exe = tmp_path / "alignlocal_word_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "alignlocal_word_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, packs, rows, cells = done.stdout.split()
    assert word == "ok" and int(packs) == 54 and int(rows) == 300 and int(cells) > 1_000_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text))), text


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    declared, text = _declared("prf_alignlocal.h")
    assert declared == sorted(pn.ALIGNLOCAL_EXPORTS) == ["prf_motif_align_local", "prf_motif_align_local_seq"]      # no _ex form: no knob
    older = [pn.EXPORTS, pn.PERIOD_EXPORTS, pn.DOTPLOT_EXPORTS, pn.DOTPAIR_EXPORTS, pn.DOTRUNS_EXPORTS, pn.DOTCHAIN_EXPORTS, pn.DOTLINK_EXPORTS,
             pn.PERIODCHAIN_EXPORTS, pn.PERIODLINK_EXPORTS, pn.CONSENSUS_EXPORTS, pn.PHASED_EXPORTS, pn.ALIGN_EXPORTS, pn.ALIGNPATH_EXPORTS]
    assert len(older) == 13 and not set(declared) & set().union(*older)
    header = open(os.path.join(ROOT, "include", "prf.h")).read()
    assert header.count('#include "prf_alignlocal.h"') == 1 and '#include "prf_alignpath.h"\n#include "prf_alignlocal.h"\n' in header
    assert header.index('#include "prf_alignlocal.h"') < header.index("#ifdef __cplusplus\n}")
    assert all(hasattr(lib, name) and getattr(lib, name).argtypes for name in declared)
    raw = ctypes.CDLL(pn.LIB_PATH)                                             # exported: the loader finds them by name
    assert all(hasattr(raw, name) for name in declared) and not hasattr(raw, "prf_motif_align_local_ex")
    assert lib.prf_abi_version() == 4
    assert int(re.search(r"#define PRF_ALIGNLOCAL_MAX_WEIGHT (\d+)u", text)[1]) == pn.ALIGNLOCAL_MAX_WEIGHT == L.MAX_WEIGHT == 16
    assert np.dtype(pn.LOCAL_ALIGNMENT_DTYPE).itemsize == 24 and pn.LOCAL_ALIGNMENT_DTYPE == L.DTYPE
    struct = re.search(r"typedef struct prf_local_alignment \{(.*?)\} prf_local_alignment;", text, flags=re.S)[1]
    assert re.findall(r"\b(\w+);", struct) == list(L.FIELDS) and re.findall(r"\b(uint\d+_t)\b", struct) == ["uint32_t"] * 6
    # the two headers in front and their declarations stay as they are
    assert _declared("prf_alignpath.h")[0] == sorted(pn.ALIGNPATH_EXPORTS) and _declared("prf_align.h")[0] == sorted(pn.ALIGN_EXPORTS)


ROWS = ((0, 12, 3),)


def _call(lib, pn, form, seq=b"ACGTACGTACGT", span=(0, 12), rows=ROWS, n_rows=None, motifs=b"ACG", length=None, dst=True, reserved=0,
          weights=TRF):
    table = np.zeros(max(1, len(rows or ())), dtype=pn.REPEAT_DTYPE)
    for at, row in enumerate(rows or ()):
        table[at] = tuple(row) + (reserved if at == len(rows) - 1 else 0,)
    out = np.full(64 * 24, 0xAB, dtype=np.uint8)
    stats = pn.ScanStats()
    stats.n_hits = 77
    tail = (*span, table.ctypes.data if rows is not None else None, len(rows or ()) if n_rows is None else n_rows, motifs,
            len(motifs or b"") if length is None else length, *weights, out.ctypes.data if dst else None, ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_motif_align_local_seq(None, arr, *tail)
    else:
        rc = lib.prf_motif_align_local(None, None, 0, *tail)
    assert (out == 0xAB).all() and stats.n_hits == 77                          # a refused call writes nothing
    return rc


LONG = (1 << 19) + 1
MANY = (1 << 24) + 1
# each case breaks one rule and, where a call can, the rules behind it: the first in the documented order is the one reported
ORDER = [
    (dict(span=(7, 3), weights=(0, 17, 0), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EINVAL", "begin 7"),
    (dict(weights=(17, 0, 0), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EINVAL", "mismatch is 0"),
    (dict(weights=(0, 17, 17), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EINVAL", "match is 0"),
    (dict(weights=(17, 16, 0), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EINVAL", "indel is 0"),
    (dict(weights=(17, 18, 19), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EUNSUPPORTED", "match = 17 is above 16 (PRF_ALIGNLOCAL_MAX_WEIGHT)"),
    (dict(weights=(16, 18, 19), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EUNSUPPORTED", "mismatch = 18 is above 16"),
    (dict(weights=(16, 1, 1 << 31), n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EUNSUPPORTED", "indel = 2147483648 is above 16"),
    (dict(n_rows=MANY, rows=None, motifs=None, dst=False), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_ROWS"),
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
    (dict(weights=(16, 16, 16)), "PRF_EINVAL", "NULL context"),               # the limit itself passes
    (dict(weights=(1, 1, 1)), "PRF_EINVAL", "NULL context"),
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
    assert text in message and message.startswith("prf_motif_align_local")


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
    assert _call(lib, pn, form, rows=(), weights=(2, 0, 7)) == pn.PRF_EINVAL    # ... and the weights
    assert _call(lib, pn, form, rows=(), weights=(2, 7, 17)) == pn.PRF_EUNSUPPORTED
    rc = lib.prf_motif_align_local_seq(None, None, 0, 4, None, 0, None, 0, 2, 7, 7, None, None)
    assert rc == pn.PRF_OK


def test_a_missing_sequence_is_refused():
    pn, lib = _lib()
    table, out = A.repeats((0, 4, 2)), np.zeros(1, dtype=pn.LOCAL_ALIGNMENT_DTYPE)
    rc = lib.prf_motif_align_local_seq(None, None, 0, 4, table.ctypes.data, 1, b"AC", 2, 2, 7, 7, out.ctypes.data, None)
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 2, [100, 50])
    ok = A.repeats((0, 10, 3))
    with pytest.raises(ValueError, match="contig 2"):
        g.motif_align_local(2, 0, None, ok, ["ACG"])
    with pytest.raises(ValueError, match="mismatch"):
        g.motif_align_local(0, 0, None, ok, ["ACG"], mismatch=0)
    with pytest.raises(ValueError, match=r"indel = 17 is more than a local alignment takes \(16\)"):
        g.motif_align_local(0, 0, None, ok, ["ACG"], indel=17)
    with pytest.raises((TypeError, ValueError)):
        g.motif_align_local(0, 0, None, ok, ["ACG"], match=2.5)
    with pytest.raises(ValueError, match="fields start, end and k"):
        g.motif_align_local(0, 0, None, [(0, 10, 3)], ["ACG"])
    with pytest.raises(ValueError, match=r"repeat 1: \[0, 51\) is not a stretch of the range's 50 positions"):
        g.motif_align_local(1, 0, None, A.repeats((0, 50, 3), (0, 51, 3)), ["ACG", "ACG"])
    with pytest.raises(ValueError, match=r"repeat 1: k = 1025 is more than an alignment takes \(1024\)"):
        g.motif_align_local(0, 0, None, A.repeats((0, 50, 3), (0, 50, 1_025)), ["ACG", "A" * 1_025])
    big = pn.Genome(None, None, 1, [1 << 20])
    with pytest.raises(ValueError, match=r"repeat 0: 524289 positions are more than an alignment takes \(524288\)"):
        big.motif_align_local(0, 0, None, A.repeats((1, (1 << 19) + 2, 3)), ["ACG"])
    with pytest.raises(ValueError, match="repeat 0: the motif has 4 letters, k is 3"):
        g.motif_align_local(0, 0, None, ok, ["ACGT"])
    g._h = big._h = None


# ---- command line ----

class _LocalGenome(_FakeGenome):
    """... and what --extend asks of it."""

    def motif_align_local(self, contig, begin, end, repeats, motifs, match=2, mismatch=7, indel=7):
        import prf_native as pn
        assert repeats["k"].max() <= pn.ALIGN_MAX_K and (repeats["end"] - repeats["start"]).max() <= pn.ALIGN_MAX_LEN
        self.calls.append(("local", len(repeats), (match, mismatch, indel)))
        return L.local(self.seq, repeats, motifs, (match, mismatch, indel), begin, end).astype(pn.LOCAL_ALIGNMENT_DTYPE)


def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_input(args, parser), args


def test_cli_parses_the_extend_options(capsys):
    import plot_periodicity_matrix as cli
    chains = ["ACGTACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2"]
    groups = ["ACGTACGT", "--groups-tsv", "g.tsv", "--min-seed", "4", "--max-gap", "2", "--max-shift", "2"]
    args = _parse(cli, chains + ["--consensus"])[1]
    assert (args.extend, args.weights, args.min_score) == (None, None, None)
    args = _parse(cli, chains + ["--consensus", "--extend", "50"])[1]
    assert (args.extend, args.weights, args.min_score) == (50, (2, 7, 7), None)
    args = _parse(cli, groups + ["--group-consensus", "--extend", "0", "--weights", "16,1,3", "--min-score", "30"])[1]
    assert (args.extend, args.weights, args.min_score) == (0, (16, 1, 3), 30)
    capsys.readouterr()
    for argv, text in ((chains + ["--extend", "50"], "--extend needs the motifs"),
                       (groups + ["--extend", "50"], "--extend needs the motifs"),
                       (["ACGT", "--extend", "5"], "--extend needs the motifs"),
                       (chains + ["--consensus", "--weights", "2,7,7"], "--weights belongs to --extend"),
                       (chains + ["--consensus", "--min-score", "5"], "--min-score belongs to --extend"),
                       (chains + ["--consensus", "--extend", "-1"], "at least 0"),
                       (chains + ["--consensus", "--extend", "5", "--weights", "2,7"], "three numbers"),
                       (chains + ["--consensus", "--extend", "5", "--weights", "2,7,x"], "three numbers"),
                       (chains + ["--consensus", "--extend", "5", "--weights", "2;7;7"], "three numbers"),
                       (chains + ["--consensus", "--extend", "5", "--weights", "0,7,7"], "match is set to 0"),
                       (groups + ["--group-consensus", "--extend", "5", "--weights", "2,7,17"], "indel is set to 17")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def _extension(seq, start, end, motif, flank, weights=TRF):
    a, b = max(0, start - flank), min(len(seq), end + flank)
    score, first, last = L.one(seq[a:b], motif, weights)[:3]
    return [str(a + first), str(a + last), str(score)] if score else [str(start), str(end), "0"]


def test_cli_lines_with_and_without_extend(tmp_path, monkeypatch):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    parent = json.load(open(os.path.join(ROOT, "tests", "golden", "alignlocal_cli_parent.json")))
    seq = K.planted(17, 2, "both")[1] + K.planted(7, 1, "ins")[1]
    files = {name: str(tmp_path / f"{name}.tsv") for name in ("plain", "aligned", "ext", "both", "kept", "split", "capped", "weights")}
    gbase = ["--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--max-shift", "4", "--min-group", "100", "--group-consensus"]
    cbase = ["--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--consensus"]
    for flag, base, name, motif_at in (("--groups-tsv", gbase, "groups", 10), ("--chains-tsv", cbase, "chains", 9)):
        # ---- without --extend the files are the parent's, byte for byte, and nothing is extended
        genome = _LocalGenome(seq)
        cli.main([seq, flag, files["plain"]] + base, context=_FakeContext(genome))
        cli.main([seq, flag, files["aligned"], "--align"] + base, context=_FakeContext(genome))
        assert open(files["plain"]).read() == parent[name] and open(files["aligned"]).read() == parent[name + "_align"]
        assert not [c for c in genome.calls if c[0] == "local"]
        # ---- three columns behind the line, in the file's coordinates
        genome = _LocalGenome(seq)
        cli.main([seq, flag, files["ext"], "--extend", "50"] + base, context=_FakeContext(genome))
        old, new = parent[name].splitlines(), open(files["ext"]).read().splitlines()
        assert len(old) == len(new) >= 2 and genome.calls[-2:] == [("local", len(old), TRF), "free"]
        for before, line in zip(old, new):
            f = before.split("\t")
            assert line.startswith(before + "\t") and line[len(before) + 1:].split("\t") == _extension(seq, int(f[1]), int(f[2]), f[motif_at], 50), before
        moved = [line for before, line in zip(old, new) if line.split("\t")[-3:-1] != before.split("\t")[1:3]]
        assert moved                                                           # the inputs: a boundary does move
        # ---- behind the columns of --align
        cli.main([seq, flag, files["both"], "--align", "--extend", "50"] + base, context=_FakeContext(_LocalGenome(seq)))
        both = open(files["both"]).read().splitlines()
        assert both == [a + "\t" + "\t".join(e.split("\t")[-3:]) for a, e in zip(parent[name + "_align"].splitlines(), new)]
        # ---- --min-score, alone and behind --min-aligned-identity
        scores = sorted(int(line.split("\t")[-1]) for line in new)
        cut = scores[len(scores) // 2]
        cli.main([seq, flag, files["kept"], "--extend", "50", "--min-score", str(cut)] + base, context=_FakeContext(_LocalGenome(seq)))
        kept = open(files["kept"]).read().splitlines()
        assert kept == [line for line in new if int(line.split("\t")[-1]) >= cut] and 0 < len(kept) and (len(kept) < len(new) or scores[0] == cut)
        cli.main([seq, flag, files["kept"], "--align", "--min-aligned-identity", "0.99", "--extend", "50", "--min-score", str(cut)] + base,
                 context=_FakeContext(_LocalGenome(seq)))
        assert open(files["kept"]).read().splitlines() == [line for line in both if float(line.split("\t")[-5]) >= 0.99 and int(line.split("\t")[-1]) >= cut]
        # ---- other weights, another flank
        genome = _LocalGenome(seq)
        cli.main([seq, flag, files["weights"], "--extend", "7", "--weights", "3,1,2"] + base, context=_FakeContext(genome))
        assert [c for c in genome.calls if c[0] == "local"] == [("local", len(old), (3, 1, 2))]
        for before, line in zip(old, open(files["weights"]).read().splitlines()):
            f = before.split("\t")
            assert line[len(before) + 1:].split("\t") == _extension(seq, int(f[1]), int(f[2]), f[motif_at], 7, (3, 1, 2))
    # ---- batches: with room for one row per call every repeat goes alone, and the lines are the same
    monkeypatch.setattr(pn, "CONSENSUS_MAX_ROWS", 1)
    genome = _LocalGenome(seq)
    cli.main([seq, "--chains-tsv", files["split"], "--extend", "50"] + cbase, context=_FakeContext(genome))
    assert [c for c in genome.calls if c[0] == "local"] == [("local", 1, TRF)] * len(old) and open(files["split"]).read().splitlines() == new
    monkeypatch.undo()
    # ---- a repeat above a limit: '.' in the three columns, dropped when the filter is given
    monkeypatch.setattr(pn, "ALIGN_MAX_K", 10)
    cli.main([seq, "--chains-tsv", files["capped"], "--extend", "50"] + cbase, context=_FakeContext(_LocalGenome(seq)))
    capped = open(files["capped"]).read().splitlines()
    wide = [int(line.split("\t")[3]) > 10 for line in old]
    assert any(wide) and not all(wide)
    assert capped == [before + "\t.\t.\t." if w else line for before, line, w in zip(old, new, wide)]
    cli.main([seq, "--chains-tsv", files["capped"], "--extend", "50", "--min-score", "0"] + cbase, context=_FakeContext(_LocalGenome(seq)))
    assert open(files["capped"]).read().splitlines() == [line for line, w in zip(new, wide) if not w]
