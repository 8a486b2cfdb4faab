"""CPU: the list of junctions between the chains of the period lines of a range, and the gapped tandem repeats they join (DESIGN
17; prf_period_links, prf_native.join_period_chains, tandem_groups, plot_periodicity_matrix.py --groups-tsv).  The model
(tests/periodlink_model.py: dotlink_model's pairwise construction on periodchain_model's chains of the whole band) is pinned to an
independent brute force (every line as a string of 0 and 1, its chains by a regular expression, the candidates looked up line by
line) on the 276 distinct sequences of tests/golden/dotpair.jsonl.gz, and to dotlink_model on the rectangle s x s; the step of the
join kernel (csrc/periodlink_step.h) runs on the host against a third brute force (tests/periodlink_step_check.cpp).  The refusals
of the new entry points are decided before the context is looked at (NULL context, no GPU needed), in the documented order; the
joins and the command line run on the host as well.  Every list is compared exactly."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import dotchain_model as C
import dotlink_model as DL
import dotpair_model as P
import dotruns_model as R
import periodchain_model as M
import periodlink_cases as K
import periodlink_model as L
from conftest import ROOT, load_jsonl_gz

TRIPLES = [(3, 2, 1), (3, 2, 4), (4, 8, 8), (5, 3, 32), (8, 16, 32)]             # (min_seed, max_gap, max_shift), DESIGN 15.4's
# the links of the 276 sequences per (triple, n_matches), counted with the brute force: floors, so that no triple passes on an
# empty list (every one is above 100, so no generated sequences are needed to fill one up)
FLOORS = {((3, 2, 1), 0): 5804, ((3, 2, 1), 1): 7613, ((3, 2, 4), 0): 10318, ((3, 2, 4), 1): 12840, ((4, 8, 8), 0): 3940, ((4, 8, 8), 1): 5108,
          ((5, 3, 32), 0): 2095, ((5, 3, 32), 1): 2812, ((8, 16, 32), 0): 203, ((8, 16, 32), 1): 299}


@pytest.fixture(scope="module")
def sequences():
    golden = load_jsonl_gz("dotpair.jsonl.gz")
    found = sorted({c["a"] for c in golden} | {c["b"] for c in golden})
    assert len(found) == 276
    return found


@pytest.fixture(scope="module")
def modelled(sequences):
    """{(sequence index, triple, n_matches): (every link of the whole band, the smallest keys are unique)}, computed once."""
    out = {}
    for at, s in enumerate(sequences):
        for n_matches in (0, 1):
            chains = {}
            for triple in TRIPLES:
                if triple[:2] not in chains:
                    chains[triple[:2]] = L.band_chains(s, n_matches, *triple[:2])
                unique = []
                out[at, triple, n_matches] = L.all_links(chains[triple[:2]], *triple, unique), all(unique)
    return out


def _line_chains(text, min_seed, max_gap):
    out = []
    for m in re.finditer("1+", text):
        if m.end() - m.start() < min_seed:
            continue
        if out and m.start() - out[-1][1] - 1 <= max_gap:
            out[-1][1] = m.end() - 1
        else:
            out.append([m.start(), m.end() - 1])
    return out


def _brute(seq, n_matches, min_seed, max_gap, max_shift):
    """Every link, from the lines 1 .. n - 1 as strings: {k: [(t_s, t_e)]}; pred and succ by looking at the 2 max_shift
    neighbouring lines of a chain, the key computed from the definition's words."""
    s = seq.upper()
    n = len(s)
    ov = min(min_seed - 1, L.OVERLAP)
    lines = {}
    for k in range(1, n):
        text = "".join("1" if s[t] == s[t + k] and (n_matches or s[t] != "N") else "0" for t in range(n - k))
        lines[k] = [(a, b) for a, b in _line_chains(text, min_seed, max_gap)]

    def key(k_x, t_e, k_y, t_s):
        shift = k_y - k_x
        gi = t_s - t_e - 1
        g = min(gi, gi + shift)
        if not -ov <= g <= max_gap:
            return None
        return (max(g, 0) + abs(shift), abs(shift), max(-g, 0), shift < 0)

    def best(k, at, forward):
        options = []
        for shift in range(-max_shift, max_shift + 1):
            other = k + shift if forward else k - shift
            if shift == 0 or other not in lines:
                continue
            for t_s, t_e in lines[other]:
                found = key(k, at, other, t_s) if forward else key(other, t_e, k, at)
                if found is not None:
                    options.append((found, other, (t_s, t_e)))
        options.sort()
        assert len(options) < 2 or options[0][0] != options[1][0]
        return options[0] if options else None

    found = []
    for k, chains in lines.items():
        for t_s, t_e in chains:                                      # Y
            pred = best(k, t_s, False)
            if pred is None:
                continue
            kk, k_x, (_x_s, x_e) = pred
            if best(k_x, x_e, True)[1:] != (k, (t_s, t_e)):
                continue
            found.append((t_s, x_e, k, k - k_x, kk[0] - kk[1], kk[2]))
    return np.sort(np.array(found, dtype=L.DTYPE), order=["start", "k"])


def test_model_agrees_with_a_brute_force_on_every_fixture_sequence(sequences, modelled):
    bad, counts = [], {key: 0 for key in FLOORS}
    for at, s in enumerate(sequences):
        for n_matches in (0, 1):
            for triple in TRIPLES:
                want = _brute(s, n_matches, *triple)
                counts[triple, n_matches] += len(want)
                if not L.same(modelled[at, triple, n_matches][0], want):
                    bad.append((at, triple, n_matches))
    print(counts)
    assert not bad, f"{len(bad)} differ: {bad[:5]}"
    assert all(counts[key] >= floor for key, floor in FLOORS.items()) and min(FLOORS.values()) >= 100


def test_the_smallest_key_is_unique_and_degrees_are_at_most_one(sequences, modelled):
    for (at, triple, n_matches), (links, unique) in modelled.items():
        assert unique, (at, triple, n_matches)
        into = list(zip(links["start"].tolist(), links["k"].tolist()))
        out_of = list(zip(links["from_end"].tolist(), (links["k"].astype(np.int64) - links["shift"]).tolist()))
        assert len(set(into)) == len(into) and len(set(out_of)) == len(out_of), (at, triple)
        min_seed, max_gap, max_shift = triple
        assert (np.abs(links["shift"]) >= 1).all() and (np.abs(links["shift"]) <= max_shift).all()
        assert (links["gap"] <= max_gap).all() and (links["overlap"] <= min(min_seed - 1, L.OVERLAP)).all()
        assert not ((links["gap"] > 0) & (links["overlap"] > 0)).any()
        # the row's own arithmetic: g from the two cells and the shift
        gi = links["start"].astype(np.int64) - links["from_end"].astype(np.int64) - 1
        assert np.array_equal(np.minimum(gi, gi + links["shift"]), links["gap"].astype(np.int64) - links["overlap"])
        k_x = links["k"].astype(np.int64) - links["shift"]
        n = len(sequences[at])
        assert not len(links) or (k_x.min() >= 1 and k_x.max() <= n - 1 and int(links["k"].min()) >= 1 and int(links["k"].max()) <= n - 1)
        # t_s grows strictly along links
        assert (links["start"].astype(np.int64) > links["from_end"].astype(np.int64) - min(min_seed - 1, L.OVERLAP)).all()


def test_the_join_form_of_the_model_agrees_with_the_pairwise_one(sequences, modelled):
    """all_links_by_join, which tests/test_periodlink_gpu.py needs for a million chains, against all_links: the fixture's triples
    on every fourth sequence (the two with max_shift 32, 2 000 joins each, on every twelfth), and seeds of one and two cells, where
    the chains lie densest (the GPU test's min_seed = 1, max_gap = 0 among them), on the first 100 letters of every third: the
    pairwise matrices of a thousand chains."""
    bad, found = [], 0
    for (at, triple, n_matches), (links, _) in modelled.items():
        if at % (12 if triple[2] == 32 else 4):
            continue
        got = L.all_links_by_join(L.band_chains(sequences[at], n_matches, *triple[:2]), *triple)
        found += len(got)
        if not L.same(got, links):
            bad.append((at, triple, n_matches))
    for at, s in enumerate(sequences[::3]):
        for triple in ((1, 0, 2), (1, 1, 1), (2, 0, 3)):
            chains = L.band_chains(s[:100], at % 2, *triple[:2])
            got, want = L.all_links_by_join(chains, *triple), L.all_links(chains, *triple)
            found += len(want)
            if not L.same(got, want):
                bad.append((at, triple))
    assert not bad, f"{len(bad)} differ: {bad[:5]}"
    assert found > 20_000


def test_partitions_in_positions_and_in_k_add_up(sequences, modelled):
    rng = random.Random(17)
    for at, s in list(enumerate(sequences))[::3]:
        n = len(s)
        every = modelled[at, (3, 2, 4), 0][0]
        r, q = rng.randrange(0, n + 1), rng.randrange(1, n + 2)
        parts = [L.select(every, n, positions, kmin, kmax) for positions in ((0, r), (r, n + 7)) for kmin, kmax in ((1, q), (q + 1, None))]
        assert L.same(np.sort(np.concatenate(parts), order=["start", "k"]), every), at
        assert L.same(L.links(s, q + 1, n, 3, 2, 4, positions=(r, None)), parts[3]), at
    # one inserted base: Y's start and line decide the window; X lies on a line outside [kmin, kmax]
    seq = K.CASES["an insertion of 1"][0]
    every = K.expected("an insertion of 1", 0)
    assert [(int(x["k"]), int(x["shift"])) for x in every] == [(21, 1), (20, -1)]
    assert L.same(L.links(seq, 21, 21, K.S, K.G, K.D), every[:1]) and L.same(L.links(seq, 20, 20, K.S, K.G, K.D), every[1:])
    start = int(every["start"][0])
    assert L.same(L.links(seq, 1, 30, K.S, K.G, K.D, positions=(start, start + 1)), every[:1])
    assert len(L.links(seq, 1, 30, K.S, K.G, K.D, positions=(0, start))) == 0


def test_links_above_twice_max_shift_are_those_of_the_rectangle(sequences):
    """n_matches = 1: line k of the range is the diagonal col - row = k of s x s.  A chain on a line above max_shift has no
    candidate on the lines <= 0, and its candidates' other candidates lie above 0 if it lies above 2 max_shift: there the band's
    links are the rectangle's."""
    total = 0
    for s in sequences[::2]:
        raw = P.kept_cells(s, s, "+", 0)
        every = R.all_runs(raw)
        for triple in TRIPLES:
            min_seed, max_gap, max_shift = triple
            chains = C.all_chains(raw, min_seed, max_gap, every)
            rect = DL.all_links(chains[chains["dir"] == R.MAIN], raw.shape[1], *triple)
            delta = rect["col"].astype(np.int64) - rect["row"].astype(np.int64)
            rect = np.sort(rect[(delta >= 1) & (delta > 2 * max_shift)], order=["row", "col"])
            band = L.links(s, 2 * max_shift + 1, len(s), *triple, n_matches=True)
            assert len(band) == len(rect), (s, triple)
            assert np.array_equal(band["start"], rect["row"]) and np.array_equal(band["k"], rect["col"] - rect["row"])
            assert np.array_equal(band["from_end"], rect["from_row"])
            assert all(np.array_equal(band[f], rect[f]) for f in ("shift", "gap", "overlap"))
            total += len(band)
    assert total >= 1000


# ---- the planted junctions ----

@pytest.mark.parametrize("name", list(K.CASES))
def test_planted_junctions_hold_what_they_claim(name):
    seq, params, _claims = K.CASES[name]
    assert set(seq) <= set(b"ACGTN")
    for n_matches in (0, 1):
        links = K.expected(name, n_matches)
        K.check_claim(name, links, n_matches)
        assert L.same(links, _brute(seq.decode(), n_matches, *params)), name
    if name == "a period below min_seed":                       # the chain of line 3 runs over the insertion
        line3 = M.line_chains(seq, 0, 3, 3, params[0], params[1])
        assert len(line3) == 1 and int(line3["len"][0]) >= 55 and int(line3["seeds"][0]) == 2
    if name == "a head on line 3":
        assert int(K.expected(name, 0)["k"][0]) == 3 and params[2] == 8


def test_dense_bands_link_up_to_their_last_lines():
    near_the_end = 0
    for seq, params in K.DENSE:
        for n_matches in (0, 1):
            links = L.links(seq, 1, len(seq), *params, n_matches=n_matches)
            assert L.same(links, _brute(seq.decode(), n_matches, *params))
            near_the_end += int((np.maximum(links["k"], links["k"].astype(np.int64) - links["shift"]) >= len(seq) - 8).sum())
    assert near_the_end >= 10
    for seq in K.generated(12):
        assert L.same(L.links(seq, 1, len(seq), 4, 2, 4), _brute(seq.decode(), 0, 4, 2, 4))


# ---- join_period_chains and tandem_groups ----

def _chains(*rows):
    import prf_native
    return np.sort(np.array(list(rows), dtype=prf_native.PCHAIN_DTYPE), order=["start", "k"])


def _links(*rows):
    import prf_native
    return np.sort(np.array(list(rows), dtype=prf_native.PLINK_DTYPE), order=["start", "k"])


def _as(rows, dtype, fields):
    out = np.zeros(len(rows), dtype=dtype)
    for f in fields:
        out[f] = rows[f]
    return out


def test_join_period_chains_on_hand_made_lists():
    import prf_native as pn
    # (start, len, matches, k, seeds).  A path of three: line 20 -> (+2, gap 1) line 22 -> (-2, overlap 3) line 20; a chain alone;
    # a chain whose predecessor is missing
    chains = _chains((10, 30, 28, 20, 3), (41, 20, 20, 22, 1), (58, 40, 37, 20, 4), (5, 12, 12, 7, 1), (200, 9, 9, 30, 1))
    # (start, from_end, k, shift, gap, overlap)
    links = _links((41, 39, 22, 2, 1, 0), (58, 60, 20, -2, 0, 3), (200, 190, 30, 4, 5, 0))
    groups = pn.join_period_chains(chains, links)
    assert groups.dtype == np.dtype(pn.PGROUP_DTYPE) and len(groups) == 3
    assert groups["start"].tolist() == [5, 10, 200] and groups["k_first"].tolist() == [7, 20, 30]
    path = groups[1]
    assert (int(path["end"]), int(path["span_a"]), int(path["span_b"])) == (58 + 40 + 20, 88, 88)
    assert int(path["matches"]) == 28 + 20 + 37 - 3                          # the overlap is subtracted once
    assert (int(path["chains"]), int(path["seeds"]), int(path["indel"]), int(path["net_shift"]), int(path["gap_cells"])) == (3, 8, 4, 0, 1)
    assert (int(path["k_min"]), int(path["k_max"]), int(path["period"]), bool(path["open"])) == (20, 22, 20, False)
    alone = groups[0]
    assert (int(alone["end"]), int(alone["span_a"]), int(alone["span_b"]), int(alone["matches"]), int(alone["period"])) == (24, 12, 12, 12, 7)
    assert (int(alone["chains"]), int(alone["indel"]), bool(alone["open"])) == (1, 0, False)
    begun_outside = groups[2]
    assert bool(begun_outside["open"]) and int(begun_outside["chains"]) == 1 and int(begun_outside["indel"]) == 0
    # a path that ends on another line: span_b = span_a + k_last - k_first; the period is the line with the most matches, the
    # smaller one on a tie
    two = pn.join_period_chains(_chains((0, 30, 30, 12, 1), (31, 30, 30, 11, 1)), _links((31, 29, 11, -1, 0, 0)))
    assert len(two) == 1 and (int(two["span_a"][0]), int(two["span_b"][0]), int(two["period"][0]), int(two["net_shift"][0])) == (61, 60, 11, -1)
    assert int(two["end"][0]) == 31 + 30 + 11 and int(two["indel"][0]) == 1
    # the same path without its links: two groups more
    assert len(pn.join_period_chains(chains, links[:0])) == 5
    with pytest.raises(ValueError, match="min_len = 0"):                     # a missing successor: the chains were filtered
        pn.join_period_chains(chains[chains["len"] >= 25], links)
    empty = pn.join_period_chains(chains[:0], links[:0])
    assert len(empty) == 0 and len(pn.tandem_groups(empty)) == 0
    rows = pn.tandem_groups(groups)
    assert rows.dtype == np.dtype(pn.TANDEM_GROUP_DTYPE) and rows["period"].tolist() == [7, 20, 30]
    assert np.allclose(rows["copies"], [19 / 7, 108 / 20, 39 / 30]) and np.allclose(rows["identity"], [1.0, 82 / 88, 1.0])
    # covered: [12, 100) at period 40 by [10, 118) at period 20; not by a group of the same or a larger period
    more = np.concatenate([groups, groups[1:2], groups[1:2]])
    more[3]["start"], more[3]["end"], more[3]["period"] = 12, 100, 40
    more[4]["start"], more[4]["end"], more[4]["period"] = 12, 100, 20
    assert pn.tandem_groups(more)["period"].tolist() == [7, 20, 30, 20] and len(pn.tandem_groups(more, drop_covered=False)) == 5


def test_join_period_chains_on_the_model_of_a_repeat_with_three_indels():
    import prf_native as pn
    seq, start, end, indel = K.vntr()
    chains = _as(L.band_chains(seq, 0, K.S, K.G), pn.PCHAIN_DTYPE, M.FIELDS)
    links = _as(L.all_links(chains, K.S, K.G, K.D), pn.PLINK_DTYPE, L.FIELDS)
    groups = pn.join_period_chains(chains, links)
    assert int(groups["chains"].sum()) == len(chains)
    rows = pn.tandem_groups(groups)
    # a chance match at either end of the repeat lengthens it by a base: the unit's letters are random
    assert len(rows) == 1 and abs(int(rows["start"][0]) - start) <= 1 and abs(int(rows["end"][0]) - end) <= 1
    assert (int(rows["period"][0]), int(rows["indel"][0]), int(rows["chains"][0])) == (24, indel, 7) and rows["identity"][0] > 0.95
    assert len(pn.tandem_groups(groups, drop_covered=False)) == len(groups) > 1
    whole = groups[groups["chains"] == 7]
    assert len(whole) == 1 and int(whole["net_shift"][0]) == 0 and (int(whole["k_min"][0]), int(whole["k_max"][0])) == (22, 27) and not whole["open"][0]
    # a range of k that holds the repeat's line but not the line of its first detour: the group is cut there, its second part is open
    inside = chains[(chains["k"] >= 22) & (chains["k"] <= 24)]
    cut = pn.join_period_chains(inside, links[(links["k"] >= 22) & (links["k"] <= 24)])
    assert cut["open"].any() and int(cut["chains"].sum()) == len(inside)


# ---- the step of the kernel, on the host ----

def test_step_of_the_kernel_against_a_brute_force_on_the_host(tmp_path):
    """csrc/periodlink_step.h is the text the join kernel runs between its two wave minima; the stand-alone program checks it on
    random bands, under the sanitizers."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/periodlink_step_check.cpp")
    exe = tmp_path / "step_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "periodlink_step_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, bands, heads, links, shifts, overlaps, edges = done.stdout.split()
    assert word == "ok" and int(bands) == 140 and int(heads) > 10_000 and int(links) > 5_000 and int(shifts) == 64
    assert int(overlaps) > 1_000 and int(edges) > 1_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_periodlink.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.PERIODLINK_EXPORTS) and len(declared) == 3
    assert not set(declared) & (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS)
                                | set(pn.DOTCHAIN_EXPORTS) | set(pn.DOTLINK_EXPORTS) | set(pn.PERIODCHAIN_EXPORTS))
    assert open(os.path.join(ROOT, "include", "prf.h")).read().count('#include "prf_periodlink.h"') == 1
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4
    assert np.dtype(pn.PLINK_DTYPE).itemsize == 32 and pn.PLINK_DTYPE == L.DTYPE
    struct = re.search(r"typedef struct prf_plink \{(.*?)\} prf_plink;", text, flags=re.S)[1]
    assert re.findall(r"\b(start|from_end|k|shift|gap|overlap)\b", struct) == list(L.FIELDS)
    assert "int32_t shift" in struct


def _call(lib, pn, form, seq=b"ACGTACGTACGT", begin=0, end=12, positions=(0, 12), kmin=1, kmax=6, n_matches=0, min_seed=3, max_gap=2,
          max_shift=2, capacity=64, dst=True, n_links=True):
    buf = np.full(64, 0xAB, dtype=np.uint8).repeat(32)
    n, stats = ctypes.c_uint64(77), pn.ScanStats()
    tail = (begin, end, positions[0], positions[1], kmin, kmax, n_matches, min_seed, max_gap, max_shift, buf.ctypes.data if dst else None,
            capacity, ctypes.byref(n) if n_links else None, ctypes.byref(stats))
    if form == "one_shot":
        arr, _keep = pn._contig_array([seq])
        rc = lib.prf_period_links_seq(None, arr, *tail)
    elif form == "ex":
        rc = lib.prf_period_links_ex(None, None, 0, *tail, 4096)
    else:
        rc = lib.prf_period_links(None, None, 0, *tail)
    assert (buf == 0xAB).all() and n.value == 77                              # a refused call writes nothing
    return rc


# each case breaks one rule and every rule behind it: the first in the documented order is the one reported
LATER = dict(positions=(5, 4), kmin=0, n_matches=2, min_seed=0, max_gap=4097, max_shift=0, capacity=(1 << 24) + 1, dst=False, n_links=False)


def _later(*fixed, **more):
    return dict({k: v for k, v in LATER.items() if k not in fixed}, **more)


ORDER = [
    (dict(begin=7, end=3, **LATER), "PRF_EINVAL", "begin 7"),
    (dict(LATER), "PRF_EINVAL", "pos0"),
    (_later("positions"), "PRF_EINVAL", "kmin is 0"),
    (_later("positions", "kmin", kmin=9, kmax=4), "PRF_EINVAL", "kmin 9 is above kmax 4"),
    (_later("positions", "kmin"), "PRF_EINVAL", "n_matches is 2"),
    (_later("positions", "kmin", "n_matches"), "PRF_EINVAL", "min_seed is 0"),
    (_later("positions", "kmin", "n_matches", "min_seed"), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (_later("positions", "kmin", "n_matches", "min_seed", "max_gap"), "PRF_EINVAL", "max_shift is 0"),
    (_later("positions", "kmin", "n_matches", "min_seed", "max_gap", max_shift=33), "PRF_EUNSUPPORTED", "PRF_DOTLINK_MAX_SHIFT"),
    (_later("positions", "kmin", "n_matches", "min_seed", "max_gap", "max_shift"), "PRF_EUNSUPPORTED", "PRF_PCHAIN_MAX_ROWS"),
    (dict(dst=False, n_links=False), "PRF_EINVAL", "NULL n_links"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(dst=False, capacity=0), "PRF_EINVAL", "NULL context"),              # counting only is a valid call
    (dict(max_gap=0xFFFFFFFF), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (dict(max_shift=0xFFFFFFFF), "PRF_EUNSUPPORTED", "PRF_DOTLINK_MAX_SHIFT"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(max_gap=4096, max_shift=32, min_seed=1 << 40, capacity=1 << 24, n_matches=1), "PRF_EINVAL", "NULL context"),
    (dict(kmin=40, kmax=0xFFFFFFFF, positions=(3, 3), begin=4, end=4), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_period_links")


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(seq=b"ACGT-ACGTACG"), "PRF_ESYMBOL", "position 4"),
    (dict(seq=b"", begin=0, end=0), "PRF_EINVAL", "NULL context"),            # an empty range
    (dict(end=1 << 63, positions=(2, 1 << 63)), "PRF_EINVAL", "NULL context"),   # ends are clipped
])
def test_refusals_that_need_the_sequence(kwargs, code, text):
    pn, lib = _lib()
    assert _call(lib, pn, "one_shot", **kwargs) == getattr(pn, code)
    assert text in lib.prf_last_error().decode()


def test_a_missing_sequence_and_a_window_above_the_limit_are_refused():
    pn, lib = _lib()
    n, stats = ctypes.c_uint64(0), pn.ScanStats()
    rc = lib.prf_period_links_seq(None, None, 0, 4, 0, 4, 1, 2, 0, 3, 1, 1, None, 0, ctypes.byref(n), ctypes.byref(stats))
    assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()
    big = (pn._Contig * 1)()                                                  # 2^43 cells: judged from the length, the sequence is never read
    block = ctypes.create_string_buffer(16)
    big[0].ascii, big[0].len = ctypes.addressof(block), 1 << 30
    rc = lib.prf_period_links_seq(None, big, 0, 1 << 30, 0, 1 << 30, 1, 1 << 13, 0, 12, 8, 4, None, 0, ctypes.byref(n), ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g = pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="contig 1"):
        g.period_links(1, 0, None, 1, 6, 4, 1, 1)
    with pytest.raises(ValueError, match="periods"):
        g.period_links(0, 0, None, 0, 6, 4, 1, 1)
    with pytest.raises(ValueError, match="min_seed"):
        g.period_links(0, 0, None, 1, 6, 0, 1, 1)
    with pytest.raises(ValueError, match="max_gap"):
        g.period_links(0, 0, None, 1, 6, 4, 4097, 1)
    for max_shift in (0, 33, -1, True):
        with pytest.raises(ValueError, match="max_shift"):
            g.period_links(0, 0, None, 1, 6, 4, 1, max_shift)
    with pytest.raises(ValueError, match="positions"):
        g.period_links(0, 0, None, 1, 6, 4, 1, 1, positions=(5, 4))
    g._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_input(args, parser), args


def test_cli_parses_the_groups_options(tmp_path, capsys):
    import plot_periodicity_matrix as cli
    base = ["ACGTACGT", "--groups-tsv", "g.tsv", "--min-seed", "4", "--max-gap", "2", "--max-shift", "3"]
    (chrom, seq, begin, end), args = _parse(cli, base)
    assert (chrom, seq, begin, end) == ("sequence", "ACGTACGT", 0, 8)
    assert (args.groups_tsv, args.min_seed, args.max_gap, args.max_shift, args.min_group, args.min_identity, args.keep_covered, args.n_matches,
            args.chain_window, args.chains_tsv) == ("g.tsv", 4, 2, 3, 0, 0.0, False, False, 1 << 22, None)
    args = _parse(cli, base + ["--min-group", "30", "--min-identity", "0.9", "--keep-covered", "--n-matches", "--chain-window", "1000"])[1]
    assert (args.min_group, args.min_identity, args.keep_covered, args.n_matches, args.chain_window) == (30, 0.9, True, True, 1000)
    # nothing changes for a command line without the new options
    (_, seq, _, _), args = _parse(cli, ["ACGTACGT", "--max-motif-size", "4"])
    assert seq == "ACGTACGT" and args.groups_tsv is None and args.max_shift is None and args.output_path == "periodicity_matrix.png"
    args = _parse(cli, ["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "1"])[1]
    assert args.chains_tsv == "c.tsv" and args.groups_tsv is None
    # above 5 000 positions the list needs no --window
    long_fa = tmp_path / "x.fa"
    long_fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    (chrom, seq, begin, end), _ = _parse(cli, [str(long_fa), "-i", "chrA:100-7100", "--groups-tsv", "g.tsv", "--min-seed", "12", "--max-gap", "8",
                                                "--max-shift", "32"])
    assert (chrom, len(seq), begin, end) == ("chrA", 8000, 100, 7100)
    capsys.readouterr()
    short = ["ACGT", "--groups-tsv", "g.tsv"]
    full = short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "1"]
    for argv, text in ((short, "--max-shift"), (short + ["--min-seed", "4", "--max-gap", "1"], "--max-shift"),
                       (short + ["--max-gap", "4", "--max-shift", "1"], "--min-seed"),
                       (["ACGT", "--max-shift", "5"], "--groups-tsv"), (["ACGT", "--min-group", "5"], "--groups-tsv"),
                       (["ACGT", "--keep-covered"], "--groups-tsv"), (["ACGT", "--min-seed", "5"], "--chains-tsv or --groups-tsv"),
                       (["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "1", "--max-shift", "1"], "--groups-tsv"),
                       (full + ["--chains-tsv", "c.tsv"], "one of them"), (full + ["--min-chain", "3"], "--min-chain goes with --chains-tsv"),
                       (full + ["--keep-multiples"], "--keep-covered"),
                       (short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "0"], "1 .. 32"),
                       (short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "33"], "1 .. 32"),
                       (short + ["--min-seed", "0", "--max-gap", "1", "--max-shift", "1"], "at least 1"),
                       (short + ["--min-seed", "3", "--max-gap", "4097", "--max-shift", "1"], "0 .. 4096"),
                       (full + ["--min-group", "-2"], "at least 0"), (full + ["--min-identity", "1.5"], "0 .. 1"),
                       (full + ["--chain-window", "0"], "at least 1"), (full + ["--window", "64"], "belong to the profile")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_group_lines_are_in_genomic_coordinates():
    import plot_periodicity_matrix as cli
    import prf_native as pn
    seq = "ttttttttttacgacgacgacgatacgtttt"
    rows = np.zeros(1, dtype=pn.TANDEM_GROUP_DTYPE)
    rows[0] = (2, 16, 3, 14 / 3, 0.9091, 2, 3, 4)
    assert list(cli.group_lines("chr1", 8, seq, rows)) == ["chr1\t10\t24\t3\t4.667\t0.9091\t2\t3\t4\tACG\n"]


class _StubGenome:
    def __init__(self, ctx, seq):
        self.ctx, self.seq = ctx, seq

    def period_chains(self, contig, begin, end, kmin, kmax, min_seed, max_gap, min_len=0, n_matches=False, positions=None):
        import prf_native
        self.ctx.calls.append(("chains", begin, end, kmin, kmax, min_seed, max_gap, min_len, n_matches, positions))
        got = M.select(L.band_chains(self.seq, n_matches, min_seed, max_gap, begin, end), end - begin, positions, kmin, kmax, min_len)
        return _as(got, prf_native.PCHAIN_DTYPE, M.FIELDS)

    def period_links(self, contig, begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches=False, positions=None):
        import prf_native
        self.ctx.calls.append(("links", begin, end, kmin, kmax, min_seed, max_gap, max_shift, n_matches, positions))
        return _as(L.links(self.seq, kmin, kmax, min_seed, max_gap, max_shift, n_matches, begin, end, positions), prf_native.PLINK_DTYPE, L.FIELDS)

    def free(self):
        self.ctx.calls.append(("free",))


class _StubContext:
    """Serves period_chains and period_links from the models, so that the command line's path runs without a GPU."""

    def __init__(self):
        self.calls = []

    def load(self, seqs, kmax_hint):
        return _StubGenome(self, seqs[0])


def test_cli_writes_the_groups_of_stubbed_lists(tmp_path, capsys):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    seq, start, end, indel = K.vntr()
    rng = random.Random(8)
    chrom = "".join(rng.choice("ACGT") for _ in range(100)) + seq.decode() + "".join(rng.choice("ACGT") for _ in range(50))
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + chrom + "\n")
    tsv, ctx = tmp_path / "groups.tsv", _StubContext()
    common = [str(fa), "-i", f"chrT:40-{len(chrom)}", "--max-motif-size", "40", "--groups-tsv", str(tsv), "--min-seed", str(K.S), "--max-gap", str(K.G),
              "--chain-window", "150"]
    cli.main(common + ["--max-shift", str(K.D), "--min-group", "100"], context=ctx)
    n = len(chrom) - 40
    windows = [(at, min(at + 150, n)) for at in range(0, n, 150)]
    assert ctx.calls == [call for w in windows for call in (("chains", 40, len(chrom), 1, 40, K.S, K.G, 0, False, w),
                                                            ("links", 40, len(chrom), 1, 40, K.S, K.G, K.D, False, w))] + [("free",)]
    lines = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert len(lines) == 1 and len(lines[0]) == 10
    name, a0, a1, period, copies, identity, n_indel, chains, seeds, motif = lines[0]
    assert (name, period, n_indel, chains) == ("chrT", "24", str(indel), "7")
    assert abs(int(a0) - (100 + start)) <= 1 and abs(int(a1) - (100 + end)) <= 1
    assert motif == chrom[int(a0):int(a0) + 24] and copies == f"{(int(a1) - int(a0)) / 24:.3f}" and 0.95 < float(identity) <= 1.0
    assert not list(tmp_path.glob("*.png")) and "1 repeats" in capsys.readouterr().out          # no image
    # the same lines as tandem_groups of the model of the whole interval
    chains_ = _as(M.select(L.band_chains(chrom, 0, K.S, K.G, 40, None), n, None, 1, 40), pn.PCHAIN_DTYPE, M.FIELDS)
    links_ = _as(L.links(chrom, 1, 40, K.S, K.G, K.D, begin=40), pn.PLINK_DTYPE, L.FIELDS)
    rows = pn.tandem_groups(pn.join_period_chains(chains_, links_))
    rows = rows[rows["end"] - rows["start"] >= 100]
    assert list(cli.group_lines("chrT", 40, chrom, rows)) == [line + "\n" for line in tsv.read_text().splitlines()]
    cli.main(common + ["--max-shift", "1", "--min-group", "100"], context=ctx)                  # the indels of 2 and 3 are out of reach
    assert [line.split("\t")[6:8] for line in tsv.read_text().splitlines()] == [["2", "3"]]          # the piece with the insertion of 1
    cli.main(common + ["--max-shift", str(K.D), "--min-group", "100", "--min-identity", "0.999"], context=ctx)     # filtered on the host
    assert tsv.read_text() == ""
    wider = common + ["--max-motif-size", "80", "--max-shift", str(K.D), "--min-group", "100"]  # with the images at 48 and 72 ..
    cli.main(wider, context=ctx)
    assert len(tsv.read_text().splitlines()) == 1
    cli.main(wider + ["--keep-covered"], context=ctx)
    assert len(tsv.read_text().splitlines()) > 1
