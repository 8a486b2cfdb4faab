"""The consensus over phased segments (include/prf_phased.h) without a GPU: the CPU model against an independent brute
force, its two identities with the ungapped model, the host step from chains and links to segments on planted gapped repeats
(through the CPU models of DESIGN 16 and 17), the C ABI and its refusals (no context is needed to be refused), the binding's
argument checks, the command line, and the per-lane text of the kernels on the host under the sanitizers."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import consensus_model as C
import periodchain_model as PC
import periodlink_model as PL
import phased_cases as K
import phased_model as M
from conftest import ROOT, load_jsonl_gz


def fixture_sequences():
    """The distinct sequences of the dot-plot fixture, in the order of their first appearance."""
    seen = {}
    for c in load_jsonl_gz("dotpair.jsonl.gz"):
        for s in (c["a"], c["b"]):
            seen.setdefault(s, None)
    return list(seen)


def brute(seq, k, segs):
    """(motif, agree, acgt, counts) of one row over its segments (start, end, phase), position by position."""
    counts = [[0, 0, 0, 0] for _ in range(k)]
    for start, end, phase in segs:
        for q in range(start, end):
            letter = seq[q].upper()
            if letter in "ACGT":
                counts[(phase + q - start) % k]["ACGT".index(letter)] += 1
    motif, agree = "", 0
    for column in counts:
        most = max(column)
        agree += most
        motif += "N" if most == 0 else [b for b, c in zip("ACGT", column) if c == most][0]
    return motif, agree, sum(map(sum, counts)), counts


def test_model_agrees_with_a_brute_force_on_every_fixture_sequence():
    seqs = fixture_sequences()
    assert len(seqs) == 276
    rng = random.Random(19)
    compared = tied = empty = bare = overlapping = 0
    for s in seqs:
        if not s:
            continue
        ks = [rng.randint(1, 64) for _ in range(5)] + [rng.choice((65, 100, 130, len(s) + 3)), rng.randint(1, 64)]
        per_row, flat = [], []
        for row, k in enumerate(ks):
            mine = []
            for _ in range(0 if row == 6 else rng.randint(1, 5)):              # the last row has no segment
                start = rng.randrange(len(s))
                mine.append((start, rng.randint(start + 1, len(s)), rng.choice((0, 1 % k, k - 1))))
            per_row.append(mine)
            flat += [(a, b, row, phase) for a, b, phase in mine]
            overlapping += any(a < d and c < b for i, (a, b, _) in enumerate(mine) for c, d, _ in mine[i + 1:])
        rng.shuffle(flat)                                                      # any order, rows interleaved
        got, motifs, counts = M.consensus(s, ks, M.segments(*flat))
        assert counts.shape == (sum(ks), 4)
        for k, mine, row, motif in zip(ks, per_row, got.tolist(), motifs):
            want = brute(s, k, mine)
            offset = row[0]
            assert (motif, row[1], row[2], row[3], row[4]) == (want[0], want[1], want[2], k, 0), (s, k, mine)
            assert counts[offset:offset + k].tolist() == want[3]
            compared += 1
            tied += any(sorted(c)[-1] == sorted(c)[-2] > 0 for c in want[3])
            empty += "N" in motif
            bare += not mine
        assert got["offset"].tolist() == np.concatenate([[0], np.cumsum(got["k"][:-1])]).tolist()
    print(compared, tied, empty, bare, overlapping)
    # 275 sequences hold a position; the fixture's reach: rows with a tie, with an empty column, without segments, with overlaps
    assert compared == 275 * 7 and bare == 275 and tied >= 800 and empty >= 600 and overlapping >= 500


def test_one_segment_of_phase_0_is_the_ungapped_consensus_and_a_phase_rotates_it():
    rng = random.Random(20)
    rows = 0
    for s in fixture_sequences()[::3]:
        if not s:
            continue
        plain = []
        for _ in range(6):
            start = rng.randrange(len(s))
            plain.append((start, rng.randint(start + 1, len(s)), rng.choice((1, 2, 3, 7, 63, 64, 65, 100, rng.randint(1, 64)))))
        want, want_motifs, want_counts = C.consensus(s, C.repeats(*plain))
        ks = [k for _, _, k in plain]
        got, motifs, counts = M.consensus(s, ks, M.segments(*[(a, b, at, 0) for at, (a, b, _) in enumerate(plain)]))
        assert M.same(got, want) and motifs == want_motifs and np.array_equal(counts, want_counts)
        for phase_of in (lambda k: 1 % k, lambda k: k - 1, lambda k: rng.randrange(k)):
            phases = [phase_of(k) for k in ks]
            turned, turned_motifs, turned_counts = M.consensus(s, ks, M.segments(*[(a, b, at, phases[at]) for at, (a, b, _) in enumerate(plain)]))
            assert M.same(turned, want)                                        # offset, agree, acgt and k do not see the phase
            for k, phase, o, motif, moved in zip(ks, phases, want["offset"].tolist(), want_motifs, turned_motifs):
                assert moved == (motif[k - phase:] + motif[:k - phase])
                assert np.array_equal(turned_counts[o:o + k], np.roll(want_counts[o:o + k], phase, axis=0))
                rows += 1
    assert rows == 91 * 6 * 3                                                  # 91 of the 92 sequences hold a position


def test_ties_empty_rows_overlaps_and_ranges():
    one = lambda seq, k, *segs: M.consensus(seq, [k], M.segments(*[(a, b, 0, p) for a, b, p in segs]))    # noqa: E731
    assert one("ACCA", 1, (0, 4, 0))[1] == ["A"] and one("TGCC", 2, (0, 4, 1))[1] == ["CC"]
    # a row without segments, and no segments at all
    got, motifs, counts = M.consensus("ACGT", [3, 2], M.segments((0, 4, 1, 0)))
    assert motifs == ["NNN", "AC"] and got.tolist() == [(0, 0, 0, 3, 0), (3, 2, 4, 2, 0)] and counts[:3].sum() == 0
    got, motifs, counts = M.consensus("ACGT", [3, 2], M.segments())
    assert motifs == ["NNN", "NN"] and got.tolist() == [(0, 0, 0, 3, 0), (3, 0, 0, 2, 0)] and counts.shape == (5, 4)
    # overlapping segments count once per segment; an insertion skipped by two segments: ACG ACG t ACG ACG
    got, motifs, _ = one("ACGACG", 3, (0, 6, 0), (3, 6, 0))
    assert motifs == ["ACG"] and got.tolist() == [(0, 9, 9, 3, 0)]
    got, motifs, _ = one("ACGACGtACGACG", 3, (0, 6, 0), (7, 13, 0))
    assert motifs == ["ACG"] and got.tolist() == [(0, 12, 12, 3, 0)]
    got, motifs, _ = one("ACGACGtACGACG", 3, (0, 13, 0))                        # ... which the ungapped columns mix
    assert got["agree"][0] < 12
    # a deletion: ACG ACG A_G ACG, the second segment begins in column 2 ... or one column earlier with the G in column 2
    got, motifs, _ = one("ACGACGAGACG", 3, (0, 7, 0), (7, 11, 2))
    assert motifs == ["ACG"] and got.tolist() == [(0, 11, 11, 3, 0)]
    # a range: segments are relative to begin, and lower case counts as upper case
    got, motifs, _ = M.consensus("TTTTacgacgacCTTTT", [3], M.segments((1, 9, 0, 1)), begin=4, end=13)
    assert motifs == ["ACG"] and got.tolist() == [(0, 7, 8, 3, 0)]


# ---- from chains and links to segments ----

def _lists(seq, period):
    import prf_native as pn
    kmax = period + 8
    chains = PC.chains(seq, 1, kmax, K.MIN_SEED[period], K.MAX_GAP).astype(pn.PCHAIN_DTYPE)
    links = PL.links(seq, 1, kmax, K.MIN_SEED[period], K.MAX_GAP, K.MAX_SHIFT).astype(pn.PLINK_DTYPE)
    return chains, links


def _rotations(motif):
    return {motif[i:] + motif[:i] for i in range(len(motif))}


@pytest.mark.parametrize("kind", ["ins", "del", "both"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("period", [7, 17, 40])
def test_group_segments_on_planted_indels(period, d, kind):
    import prf_native as pn
    motif, seq = K.planted(period, d, kind)
    edits = K.EDITS[kind](d)
    chains, links = _lists(seq, period)
    groups = pn.join_period_chains(chains, links)
    at = K.body_group(groups, period, len(seq))
    # ---- the input is what the test needs: ONE group over the body, on-period chains joined by isolated detours
    path = pn.period_paths(chains, links)[at]
    assert len(path) == 2 * len(edits) + 1 == groups["chains"][at]
    for j, c in enumerate(path):
        if j % 2 == 0:
            assert chains["k"][c] == period
        else:                                                                  # the indel's line, or its image one period up
            want = period + (edits[j // 2][2] if edits[j // 2][1] == "I" else -edits[j // 2][2])
            assert chains["k"][c] in (want, want + period) and chains["len"][c] <= chains["k"][c]
    # ---- the binding's step against the plain model
    pieces, segments = pn.group_segments(chains, links)
    model_pieces, model_segments = M.group_segments(chains, links, groups["period"].tolist())
    assert [tuple(p) for p in pieces.tolist()] == model_pieces and [tuple(s) for s in segments.tolist()] == model_segments
    mine = np.flatnonzero(pieces["group"] == at)
    assert len(mine) == 1                                                      # one piece
    piece = pieces[mine[0]]
    segs = segments[segments["row"] == mine[0]]
    assert piece["segments"] == len(segs) == len(edits) + 1 and piece["k"] == period and piece["anchor"] == groups["start"][at]
    assert piece["positions"] == (segs["end"] - segs["start"]).sum() and piece["end"] == segs["end"][-1] == groups["end"][at]
    assert (segs["end"][:-1] <= segs["start"][1:]).all()                       # ascending and disjoint
    # the inserted bases (lower case) lie in no segment; every other base of the group does, but the deleted ones' neighbours
    covered = np.zeros(len(seq), dtype=bool)
    for a, b in zip(segs["start"].tolist(), segs["end"].tolist()):
        covered[a:b] = True
    lower = np.array([c.islower() for c in seq])
    assert lower.sum() == sum(n for _, what, n in edits if what == "I") and not (covered & lower).any()
    inside = np.zeros(len(seq), dtype=bool)
    inside[int(groups["start"][at]):int(groups["end"][at])] = True
    assert (inside & ~covered & ~lower).sum() <= 2 * period * len(edits)
    # ---- the consensus: the planted motif rotated to the anchor, and strictly better than the ungapped columns
    ks = pieces["k"].tolist()
    cons, motifs, _ = M.consensus(seq, ks, segments)
    turn = (int(piece["anchor"]) - K.FLANK) % period
    assert motifs[mine[0]] == motif[turn:] + motif[:turn]
    rows, names = pn.group_consensus_rows(groups, pieces, cons.astype(pn.CONSENSUS_DTYPE), motifs)
    assert names[at] == motifs[mine[0]] and rows["pieces"][at] == 1 and rows["primitive"][at] == period
    assert rows["consensus_identity"][at] == cons["agree"][mine[0]] / piece["positions"] >= 0.97
    start, end = int(groups["start"][at]), int(groups["end"][at])
    flat, _, _ = C.consensus(seq, C.repeats((start, end, period)))
    print(period, d, kind, rows["consensus_identity"][at], flat["agree"][0] / (end - start))
    assert rows["consensus_identity"][at] > flat["agree"][0] / (end - start)
    assert rows["covered"][at] == piece["positions"] / (end - start) and 0.9 < rows["covered"][at] <= 1.0


@pytest.mark.parametrize("period", [7, 17, 40])
def test_two_indels_closer_than_a_period_cut_the_group_into_pieces(period):
    import prf_native as pn
    motif, seq = K.close_pair(period)
    chains, links = _lists(seq, period)
    groups = pn.join_period_chains(chains, links)
    at = K.body_group(groups, period, len(seq))
    pieces, segments = pn.group_segments(chains, links)
    model_pieces, model_segments = M.group_segments(chains, links, groups["period"].tolist())
    assert [tuple(p) for p in pieces.tolist()] == model_pieces and [tuple(s) for s in segments.tolist()] == model_segments
    mine = np.flatnonzero(pieces["group"] == at)
    assert len(mine) == 2
    cons, motifs, _ = M.consensus(seq, pieces["k"].tolist(), segments)
    for row in mine.tolist():
        assert motifs[row] in _rotations(motif) and (segments["phase"][segments["row"] == row] == 0).all()
    rows, names = pn.group_consensus_rows(groups, pieces, cons.astype(pn.CONSENSUS_DTYPE), motifs)
    largest = mine[np.argmax(pieces["positions"][mine])]
    assert rows["pieces"][at] == 2 and names[at] == motifs[largest] and rows["covered"][at] < 0.7


def _chains(*rows):
    import prf_native as pn
    out = np.zeros(len(rows), dtype=pn.PCHAIN_DTYPE)
    for at, (start, length, k) in enumerate(rows):
        out[at] = (start, length, length, k, 1)
    return out


def _links(chains, *pairs):
    """A link from chain x to chain y per pair, by the keys join_period_chains resolves."""
    import prf_native as pn
    out = np.zeros(len(pairs), dtype=pn.PLINK_DTYPE)
    for at, (x, y) in enumerate(pairs):
        out[at] = (chains["start"][y], chains["start"][x] + chains["len"][x] - 1, chains["k"][y], int(chains["k"][y]) - int(chains["k"][x]), 0, 0)
    return out


def test_group_segments_on_a_hand_written_path():
    import prf_native as pn
    # one path of period 10 (its line has the most matches): a detour at the head (line 11), three on-period chains of which the
    # second overlaps the first by 5 positions and the third lies inside what the second covered (dropped), an isolated insertion
    # of 2 (line 12, len 9 <= 12), an on-period chain, a detour that is too long (line 9, len 30 > 9), an on-period chain, two
    # detours in a row, an on-period chain, and a detour at the tail (line 8)
    chains = _chains((0, 6, 11), (10, 90, 10), (105, 95, 10), (150, 20, 10), (198, 9, 12), (212, 100, 10), (318, 30, 9), (350, 60, 10),
                     (415, 8, 11), (424, 8, 12), (440, 50, 10), (498, 7, 8), (600, 40, 10))
    links = _links(chains, (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 11))
    # chains on one line are not linked by period_links (a link changes the line); the join only follows what it is given
    groups = pn.join_period_chains(chains, links)
    assert groups["period"].tolist() == [10, 10] and groups["chains"].tolist() == [12, 1]
    pieces, segments = pn.group_segments(chains, links)
    # chain 1 opens piece 0 at 10; chains 2 and 3 follow it directly (nothing in between): each opens a piece of its own
    want_pieces = [(0, 10, 110, 10, 1, 100), (0, 105, 210, 10, 1, 105), (0, 150, 322, 10, 2, 140), (0, 350, 420, 10, 1, 70),
                   (0, 440, 500, 10, 1, 60), (1, 600, 650, 10, 1, 50)]
    want_segments = [(10, 110, 0, 0), (105, 210, 1, 0), (150, 180, 2, 0), (212, 322, 2, (212 - 150 - 2) % 10), (350, 420, 3, 0),
                     (440, 500, 4, 0), (600, 650, 5, 0)]
    assert [tuple(p) for p in pieces.tolist()] == want_pieces and [tuple(s) for s in segments.tolist()] == want_segments
    assert (M.group_segments(chains, links, groups["period"].tolist())) == (want_pieces, want_segments)
    # the clipping of overlapping segments inside ONE piece: two isolated detours whose on-period chains overlap, and one that
    # the piece already covers
    chains = _chains((10, 90, 10), (99, 5, 11), (104, 50, 10), (120, 3, 9), (125, 20, 10), (150, 4, 11), (158, 40, 10))
    links = _links(chains, (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6))
    pieces, segments = pn.group_segments(chains, links)
    assert [tuple(p) for p in pieces.tolist()] == [(0, 10, 208, 10, 3, 198)]
    assert [tuple(s) for s in segments.tolist()] == [(10, 110, 0, 0), (110, 164, 0, (110 - 10 - 1) % 10), (164, 208, 0, (164 - 10 - 1) % 10)]
    assert M.group_segments(chains, links, [10])[1] == [tuple(s) for s in segments.tolist()]
    # nothing in, nothing out
    pieces, segments = pn.group_segments(chains[:0], links[:0])
    assert len(pieces) == 0 and len(segments) == 0 and pieces.dtype == np.dtype(pn.PIECE_DTYPE) and segments.dtype == np.dtype(pn.SEGMENT_DTYPE)


def test_group_consensus_rows_fields():
    import prf_native as pn
    chains = _chains((10, 90, 10), (99, 5, 11), (104, 50, 10), (300, 20, 4))
    links = _links(chains, (0, 1), (1, 2))
    groups = pn.join_period_chains(chains, links)
    pieces, segments = pn.group_segments(chains, links)
    assert pieces["group"].tolist() == [0, 1] and pieces["positions"].tolist() == [154, 24]
    cons = np.array([(0, 140, 154, 10, 0), (10, 24, 24, 4, 0)], dtype=pn.CONSENSUS_DTYPE)
    rows, names = pn.group_consensus_rows(groups, pieces, cons, ["ACGTTGCAAC", "ACAC"])
    assert [name for name, _ in pn.GROUP_CONSENSUS_DTYPE] == [name for name, _ in pn.TANDEM_GROUP_DTYPE] + ["consensus_identity", "primitive", "pieces", "covered"]
    plain = pn.tandem_groups(groups, drop_covered=False)
    for name, _ in pn.TANDEM_GROUP_DTYPE:
        assert rows[name].tolist() == plain[name].tolist()
    assert names == ["ACGTTGCAAC", "ACAC"] and rows["primitive"].tolist() == [10, 2] and rows["pieces"].tolist() == [1, 1]
    assert rows["consensus_identity"].tolist() == [140 / 154, 1.0] and rows["covered"].tolist() == [154 / 154, 1.0]
    same, _ = pn.group_consensus_rows(plain, pieces, cons, ["ACGTTGCAAC", "ACAC"])          # the rows of tandem_groups do as well
    assert same.tobytes() == rows.tobytes()
    # the piece with the most positions names the group; ties go to the first
    two = np.array([(0, 10, 60, 10, 1, 50), (0, 70, 120, 10, 1, 50), (0, 130, 150, 10, 1, 20)], dtype=pn.PIECE_DTYPE)
    cons = np.array([(0, 40, 50, 10, 0), (10, 50, 50, 10, 0), (20, 20, 20, 10, 0)], dtype=pn.CONSENSUS_DTYPE)
    rows, names = pn.group_consensus_rows(groups, two, cons, ["A" * 10, "C" * 10, "G" * 10])
    assert names == ["A" * 10, ""] and rows["pieces"].tolist() == [3, 0] and rows["consensus_identity"].tolist() == [0.8, 0.0]
    assert rows["covered"][0] == 50 / 154 and rows["primitive"].tolist() == [1, 0]
    with pytest.raises(ValueError, match="phased_consensus returned"):
        pn.group_consensus_rows(groups, pieces, cons, ["A", "C", "G"])
    with pytest.raises(ValueError, match="phased_consensus returned"):
        pn.group_consensus_rows(groups, two, np.array([(0, 40, 50, 10, 0), (10, 50, 50, 9, 0), (19, 20, 20, 10, 0)], dtype=pn.CONSENSUS_DTYPE),
                                ["A" * 10, "C" * 9, "G" * 10])
    with pytest.raises(ValueError, match="whose chains and links"):
        pn.group_consensus_rows(groups[:0], two, cons, ["A" * 10, "C" * 10, "G" * 10])
    index = pn.tandem_groups(groups, with_index=True)[1]
    assert index.tolist() == [0, 1] and pn.tandem_groups(groups[:1], with_index=True)[1].tolist() == [0]


# ---- the per-lane text of the kernels, on the host ----

def test_item_text_against_a_brute_force_on_the_host(tmp_path):
    """csrc/phased_word.h is the text the kernels run; the stand-alone program checks it and the cutting of segments on random and
    hand-made ranges in every regime, at phases 0, 1, k - 1 and random ones, with slices of 1, 64, 100, k - 1 and more, under the
    sanitizers.  Its source of plane words refuses any word outside the range's, outside the item's, asked for twice or out of
    order.  Nothing is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/phased_word_check.cpp")
    exe = tmp_path / "phased_word_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "phased_word_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, rows, segments, items, words, positions = done.stdout.split()
    assert word == "ok" and int(rows) == 500 * 10 and int(segments) > 10_000 and int(items) > 50_000 and int(words) > 100_000 and int(positions) > 1_000_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_phased.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.PHASED_EXPORTS) and len(declared) == 3
    older = (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS) |
             set(pn.DOTCHAIN_EXPORTS) | set(pn.DOTLINK_EXPORTS) | set(pn.PERIODCHAIN_EXPORTS) | set(pn.PERIODLINK_EXPORTS) |
             set(pn.CONSENSUS_EXPORTS))
    assert not set(declared) & older
    header = open(os.path.join(ROOT, "include", "prf.h")).read()
    assert header.count('#include "prf_phased.h"') == 1 and header.index('#include "prf_phased.h"') < header.index("#ifdef __cplusplus\n}")
    assert header.index('#include "prf_consensus.h"') < header.index('#include "prf_phased.h"')
    assert all(hasattr(lib, name) and getattr(lib, name).argtypes for name in declared)
    assert lib.prf_abi_version() == 4
    found = re.search(r"#define PRF_PHASED_MAX_SEGMENTS \((\d+)ull << (\d+)\)", text)
    assert found and int(found[1]) << int(found[2]) == pn.PHASED_MAX_SEGMENTS == 1 << 24
    assert np.dtype(pn.SEGMENT_DTYPE).itemsize == 24 and pn.SEGMENT_DTYPE == M.SEGMENT_DTYPE and pn.PIECE_DTYPE == M.PIECE_DTYPE
    struct = re.search(r"typedef struct prf_segment \{(.*?)\} prf_segment;", text, flags=re.S)[1]
    assert re.findall(r"\b(start|end|row|phase);", struct) == ["start", "end", "row", "phase"]
    assert re.findall(r"\b(uint\d+_t)\b", struct) == ["uint64_t", "uint64_t", "uint32_t", "uint32_t"]
    # prf_consensus.h and its three declarations stay as they are
    older_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_consensus.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", older_text))) == sorted(pn.CONSENSUS_EXPORTS)


KS = (3,)
SEGS = ((0, 12, 0, 0),)


def _call(lib, pn, form, seq=b"ACGTACGTACGT", span=(0, 12), ks=KS, n_rows=None, segs=SEGS, n_segs=None, dst=True, motifs=True, capacity=64,
          counts=True, written=False):
    widths = np.zeros(max(1, len(ks or ())), dtype=np.uint32)
    widths[:len(ks or ())] = ks or ()
    table = np.zeros(max(1, len(segs or ())), dtype=pn.SEGMENT_DTYPE)
    for at, row in enumerate(segs or ()):
        table[at] = tuple(row)
    out = np.full(64 * 32, 0xAB, dtype=np.uint8)
    letters = np.full(64, 0xAB, dtype=np.uint8)
    sums = np.full(64 * 16, 0xAB, dtype=np.uint8)
    stats = pn.ScanStats()
    stats.n_hits = 77
    tail = (*span, widths.ctypes.data if ks is not None else None, len(ks or ()) if n_rows is None else n_rows,
            table.ctypes.data if segs is not None else None, len(segs or ()) if n_segs is None else n_segs,
            out.ctypes.data if dst else None, letters.ctypes.data if motifs else None, capacity, sums.ctypes.data if counts else None,
            ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_phased_consensus_seq(None, arr, *tail)
    elif form == "ex":
        rc = lib.prf_phased_consensus_ex(None, None, 0, *tail, 100)
    else:
        rc = lib.prf_phased_consensus(None, None, 0, *tail)
    assert written or ((out == 0xAB).all() and (letters == 0xAB).all() and (sums == 0xAB).all() and stats.n_hits == 77)   # a refused call writes nothing
    return rc


BIG_K = (1 << 26) + 1
FULL = ((0, 1 << 63, 0, 0),)                                                  # 2^63 positions in the one column of a row of k = 1
# each case breaks one rule and, where a call can, the rules behind it: the first in the documented order is the one reported
ORDER = [
    (dict(span=(7, 3), n_rows=(1 << 24) + 1, ks=None, segs=None, dst=False, motifs=False), "PRF_EINVAL", "begin 7"),
    (dict(n_rows=(1 << 24) + 1, n_segs=(1 << 24) + 1, ks=None, segs=None, dst=False, motifs=False), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_ROWS"),
    (dict(n_segs=(1 << 24) + 1, ks=None, n_rows=1, segs=None, dst=False, motifs=False), "PRF_EUNSUPPORTED", "PRF_PHASED_MAX_SEGMENTS"),
    (dict(ks=None, n_rows=1, segs=None, n_segs=1, dst=False, motifs=False), "PRF_EINVAL", "NULL ks"),
    (dict(ks=(0,), segs=None, n_segs=1, dst=False, motifs=False), "PRF_EINVAL", "NULL destination"),
    (dict(ks=(0,), segs=None, n_segs=1, motifs=False), "PRF_EINVAL", "NULL motifs"),
    (dict(ks=(0,), segs=None, n_segs=1), "PRF_EINVAL", "NULL segments"),
    (dict(ks=(3, 0, 0), segs=((5, 5, 0, 0),), capacity=1), "PRF_EINVAL", "row 1: k is 0"),
    (dict(ks=(3, BIG_K), segs=((0, 12, 0, 0), (5, 5, 9, 3), (0, 12, 0, 7)), capacity=1), "PRF_EINVAL", "segment 1: start 5"),
    (dict(ks=(3, BIG_K), segs=((7, 5, 9, 3),), capacity=1), "PRF_EINVAL", "segment 0: start 7"),
    (dict(ks=(3, BIG_K), segs=((0, 12, 1, 0), (0, 12, 2, 9), (0, 12, 0, 3)), capacity=1), "PRF_EINVAL", "segment 1: row 2 is not one of the 2 rows"),
    (dict(ks=(3, BIG_K), segs=((0, 12, 1, BIG_K - 1), (0, 12, 0, 3), (0, 0, 0, 0)), capacity=1), "PRF_EINVAL", "segment 1: phase 3 is not below the k = 3 of row 0"),
    (dict(ks=(BIG_K, 1), segs=((0, 12, 0, 0), (0, 1 << 32, 1, 0)), capacity=1), "PRF_EUNSUPPORTED", "row 1: a column of more than 2^32 - 1"),
    (dict(ks=(BIG_K, 1), segs=((0, 1 << 31, 1, 0), (5, 1 << 31, 1, 0), (0, 5, 1, 0), (0, 12, 0, 0)), capacity=1), "PRF_EUNSUPPORTED", "row 1: a column of more than 2^32 - 1"),
    (dict(ks=(1,), segs=FULL * 3, capacity=0), "PRF_EUNSUPPORTED", "row 0: a column"),                 # the sums saturate
    (dict(ks=(1,), segs=((0, (1 << 32) - 1, 0, 0),), capacity=0), "PRF_EINVAL", "holds 0 letters"),     # 2^32 - 1 positions in a column pass
    (dict(ks=(BIG_K,), capacity=1), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_LETTERS"),
    (dict(ks=(1 << 25, 1 << 25, 1), segs=((0, 13, 0, 0),), capacity=1 << 27), "PRF_EUNSUPPORTED", "PRF_CONSENSUS_MAX_LETTERS"),
    (dict(ks=(3, 4), segs=((0, 13, 1, 0),), capacity=6), "PRF_EINVAL", "holds 6 letters, the k of the rows add up to 7"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(segs=None, n_segs=0), "PRF_EINVAL", "NULL context"),                 # no segments: legal, and NULL will do
    (dict(segs=(), counts=False), "PRF_EINVAL", "NULL context"),
    (dict(counts=False, ks=(1 << 25, 1 << 25), segs=((0, 12, 1, (1 << 25) - 1),), capacity=1 << 26), "PRF_EINVAL", "NULL context"),   # the limits themselves pass
    (dict(ks=(62, 1), segs=((11, 12, 0, 61), (0, 12, 1, 0), (0, 12, 1, 0), (3, 9, 0, 5)), span=(0, 1 << 63)), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    message = lib.prf_last_error().decode()
    assert rc == getattr(pn, code), message
    assert text in message and message.startswith("prf_phased_consensus")


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(ks=(3, 4), segs=((0, 12, 0, 0), (0, 13, 1, 0))), "PRF_EINVAL", "segment 1: end 13 is behind the range's 12 positions"),
    (dict(segs=((0, 9, 0, 0), (2, 10, 0, 1)), span=(3, 12)), "PRF_EINVAL", "segment 1: end 10 is behind the range's 9 positions"),
    (dict(segs=((0, 13, 0, 0),), seq=b"ACGT-ACGTACG"), "PRF_EINVAL", "segment 0: end 13"),     # the segments are judged before the bytes
    (dict(seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(segs=(), seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(segs=((0, 1, 0, 0),), seq=b""), "PRF_EINVAL", "segment 0: end 1 is behind the range's 0 positions"),
    (dict(span=(2, 1 << 63), segs=((0, 10, 0, 2),)), "PRF_EINVAL", "NULL context"),           # ends are clipped
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_no_rows_is_no_work_and_no_error(form):
    pn, lib = _lib()
    assert _call(lib, pn, form, ks=None, n_rows=0, segs=None, n_segs=0, dst=False, motifs=False, counts=False) == pn.PRF_OK
    assert _call(lib, pn, form, ks=(), segs=(), capacity=0) == pn.PRF_OK
    assert _call(lib, pn, form, ks=(), segs=None, n_segs=5) == pn.PRF_OK        # segments without rows are not looked at
    assert _call(lib, pn, form, ks=(), span=(7, 3)) == pn.PRF_EINVAL            # ... but the range is still judged
    assert _call(lib, pn, form, ks=(), n_segs=(1 << 24) + 1) == pn.PRF_EUNSUPPORTED    # ... and the limits


def test_a_missing_sequence_is_refused():
    pn, lib = _lib()
    ks, seg = np.array([2], dtype=np.uint32), np.array([(0, 4, 0, 0)], dtype=pn.SEGMENT_DTYPE)
    out, letters = np.zeros(1, dtype=pn.CONSENSUS_DTYPE), np.zeros(8, dtype=np.uint8)
    rc = lib.prf_phased_consensus_seq(None, None, 0, 4, ks.ctypes.data, 1, seg.ctypes.data, 1, out.ctypes.data, letters.ctypes.data, 8, None, None)
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 2, [100, 50])
    ok = M.segments((0, 10, 0, 0))
    with pytest.raises(ValueError, match="contig 2"):
        g.phased_consensus(2, 0, None, [3], ok)
    with pytest.raises(ValueError, match="begin"):
        g.phased_consensus(0, 30, 20, [3], ok)
    with pytest.raises(ValueError, match="one k per row"):
        g.phased_consensus(0, 0, None, [[3]], ok)
    with pytest.raises(ValueError, match="one k per row"):
        g.phased_consensus(0, 0, None, [2.5], ok)
    with pytest.raises(ValueError, match="fields start, end, row and phase"):
        g.phased_consensus(0, 0, None, [3], np.zeros(3, dtype=[("start", "<u8"), ("end", "<u8"), ("k", "<u4")]))
    with pytest.raises(ValueError, match="fields start, end, row and phase"):
        g.phased_consensus(0, 0, None, [3], [(0, 10, 0, 0)])
    with pytest.raises(ValueError, match="row 1: k"):
        g.phased_consensus(0, 0, None, [3, 0], ok)
    with pytest.raises(ValueError, match=r"segment 0: \[5, 5\)"):
        g.phased_consensus(0, 0, None, [3], M.segments((5, 5, 0, 0)))
    with pytest.raises(ValueError, match=r"segment 1: \[0, 51\) is not a stretch of the range's 50 positions"):
        g.phased_consensus(1, 0, None, [3], M.segments((0, 50, 0, 0), (0, 51, 0, 0)))
    with pytest.raises(ValueError, match=r"range's 20 positions"):
        g.phased_consensus(0, 10, 30, [3], M.segments((0, 21, 0, 0)))
    with pytest.raises(ValueError, match="segment 1: row 2 is not one of the 2 rows"):
        g.phased_consensus(0, 0, None, [3, 4], M.segments((0, 10, 1, 0), (0, 10, 2, 0)))
    with pytest.raises(ValueError, match="segment 0: phase 3 is not below the k = 3 of row 0"):
        g.phased_consensus(0, 0, None, [3, 4], M.segments((0, 10, 0, 3), (0, 10, 1, 3)))
    with pytest.raises(ValueError, match="add up to"):
        g.phased_consensus(0, 0, None, [1 << 26, 1], ok)
    with pytest.raises(ValueError, match="slice_positions"):
        g.phased_consensus(0, 0, None, [3], ok, slice_positions=-1)
    g._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_input(args, parser), args


def test_cli_parses_the_group_consensus_options(capsys):
    import plot_periodicity_matrix as cli
    base = ["ACGTACGT", "--groups-tsv", "g.tsv", "--min-seed", "4", "--max-gap", "2", "--max-shift", "2"]
    args = _parse(cli, base)[1]
    assert (args.group_consensus, args.min_group_consensus_identity) == (False, None)
    args = _parse(cli, base + ["--group-consensus", "--min-group-consensus-identity", "0.8"])[1]
    assert (args.group_consensus, args.min_group_consensus_identity) == (True, 0.8)
    capsys.readouterr()
    chains = ["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "2"]
    for argv, text in ((["ACGT", "--group-consensus"], "--group-consensus belongs to --groups-tsv"),
                       (chains + ["--group-consensus"], "--group-consensus belongs to --groups-tsv"),
                       (base + ["--consensus"], "drift at an indel"),                      # stays refused: the new flag is the way in
                       (base + ["--group-consensus", "--consensus"], "drift at an indel"),
                       (base + ["--min-group-consensus-identity", "0.5"], "belongs to --group-consensus"),
                       (base + ["--group-consensus", "--min-group-consensus-identity", "1.5"], "0 .. 1"),
                       (base + ["--group-consensus", "--min-group-consensus-identity", "-0.1"], "0 .. 1")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_piece_batches_respect_the_three_limits():
    import plot_periodicity_matrix as cli
    ks, segs = [3, 5, 2, 9, 1, 1, 7], [1, 2, 1, 4, 1, 1, 3]
    assert list(cli.piece_batches(ks, segs, 100, 100, 100)) == [(0, 7)]
    assert list(cli.piece_batches(ks, segs, 3, 100, 100)) == [(0, 3), (3, 6), (6, 7)]
    assert list(cli.piece_batches(ks, segs, 100, 10, 100)) == [(0, 3), (3, 5), (5, 7)]
    assert list(cli.piece_batches(ks, segs, 100, 100, 4)) == [(0, 3), (3, 4), (4, 6), (6, 7)]
    assert list(cli.piece_batches(ks, segs, 100, 100, 3)) == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 7)]    # a piece above the limit goes alone
    assert list(cli.piece_batches([], [], 2, 8, 2)) == []
    for rows, letters, segments in ((1, 1, 1), (2, 9, 3), (3, 12, 5), (7, 28, 13)):
        parts = list(cli.piece_batches(ks, segs, rows, letters, segments))
        assert [a for a, _ in parts] + [len(ks)] == [0] + [b for _, b in parts]
        assert all(b - a <= rows and ((sum(ks[a:b]) <= letters and sum(segs[a:b]) <= segments) or b - a == 1) for a, b in parts)


class _FakeGenome:
    """What list_groups asks of a resident genome, answered by the models."""

    def __init__(self, seq, period):
        self.seq, self.period, self.calls = seq, period, []

    def period_chains(self, contig, begin, end, kmin, kmax, min_seed, max_gap, min_len, n_matches, positions):
        import prf_native as pn
        self.calls.append("chains")
        return PC.chains(self.seq, kmin, kmax, min_seed, max_gap, n_matches, min_len, begin, end, positions).astype(pn.PCHAIN_DTYPE)

    def period_links(self, contig, begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches, positions):
        import prf_native as pn
        self.calls.append("links")
        return PL.links(self.seq, kmin, kmax, min_seed, max_gap, max_shift, n_matches, begin, end, positions).astype(pn.PLINK_DTYPE)

    def phased_consensus(self, contig, begin, end, ks, segments):
        import prf_native as pn
        self.calls.append(("phased", len(ks), len(segments)))
        rows, motifs, _ = M.consensus(self.seq, ks, segments, begin, end)
        return rows.astype(pn.CONSENSUS_DTYPE), motifs

    def free(self):
        self.calls.append("free")


class _FakeContext:
    def __init__(self, genome):
        self.genome = genome

    def load(self, seqs, kmax_hint):
        return self.genome


def test_cli_lines_with_and_without_group_consensus(tmp_path, monkeypatch):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    motif, seq = K.planted(17, 2, "both")
    plain, named, kept, split = (str(tmp_path / name) for name in ("plain.tsv", "named.tsv", "kept.tsv", "split.tsv"))
    base = [seq, "--groups-tsv", plain, "--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--max-shift", "4", "--min-group", "100"]
    genome = _FakeGenome(seq, 17)
    cli.main(base, context=_FakeContext(genome))
    # without --group-consensus: the lines of group_lines, byte for byte, and the consensus is never asked for
    assert genome.calls == ["chains", "links", "free"]
    chains, links = genome.period_chains(0, 0, len(seq), 1, 25, 12, 8, 0, False, None), genome.period_links(0, 0, len(seq), 1, 25, 12, 8, 4, False, None)
    rows = pn.tandem_groups(pn.join_period_chains(chains, links))
    rows = rows[rows["end"] - rows["start"] >= 100]
    want = list(cli.group_lines("sequence", 0, seq, rows))
    assert len(want) == 1 and want[0].split("\t")[3] == "17" and open(plain).read() == "".join(want)
    genome = _FakeGenome(seq, 17)
    cli.main(base[:2] + [named] + base[3:] + ["--group-consensus"], context=_FakeContext(genome))
    assert genome.calls == ["chains", "links", ("phased", 1, 3), "free"]       # only the pieces of the groups that are left
    start = int(rows["start"][0])
    turned = motif[(start - K.FLANK) % 17:] + motif[:(start - K.FLANK) % 17]
    fields = open(named).read().split("\t")
    assert "\t".join(fields[:10]) == want[0][:-1] and fields[10] == turned and fields[12:14] == ["17", pn.canonical_motif(motif)]
    assert fields[14] == "1" and 0.97 <= float(fields[11]) < 1.0 and 0.95 < float(fields[15]) <= 1.0 and fields[15].endswith("\n")
    assert len(fields) == 16 and re.fullmatch(r"\d\.\d{4}", fields[11]) and re.fullmatch(r"\d\.\d{4}\n", fields[15])
    cli.main(base[:2] + [kept] + base[3:] + ["--group-consensus", "--min-group-consensus-identity", "0.999"], context=_FakeContext(_FakeGenome(seq, 17)))
    assert open(kept).read() == ""
    # batches: two repeats in one sequence; with room for one segment per call every piece goes alone, and the lines are the same
    both = seq + K.planted(17, 1, "ins")[1]
    whole, split = str(tmp_path / "whole.tsv"), str(tmp_path / "split.tsv")
    genome = _FakeGenome(both, 17)
    cli.main([both, "--groups-tsv", whole] + base[3:] + ["--group-consensus"], context=_FakeContext(genome))
    assert genome.calls == ["chains", "links", ("phased", 2, 5), "free"]
    monkeypatch.setattr(pn, "PHASED_MAX_SEGMENTS", 1)
    genome = _FakeGenome(both, 17)
    cli.main([both, "--groups-tsv", split] + base[3:] + ["--group-consensus"], context=_FakeContext(genome))
    assert genome.calls == ["chains", "links", ("phased", 1, 3), ("phased", 1, 2), "free"]
    assert open(whole).read() == open(split).read() and open(whole).read().count("\n") == 2 and open(named).read() in open(whole).read()
