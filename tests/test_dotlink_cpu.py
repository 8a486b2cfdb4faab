"""CPU: the list of junctions between the chains of the dot plot of two ranges, and the gapped repeats they join (DESIGN 15;
prf_dotpair_links, prf_native.join_chains, plot_dot_plot.py --groups-tsv).  The model (tests/dotlink_model.py: the definition on
dotchain_model.all_chains, with pairwise matrices) is pinned to an independent brute force (every line as a string of 0 and 1,
its chains by a regular expression, the candidates looked up line by line) on every case of tests/golden/dotpair.jsonl.gz; the
walks of the join kernel (csrc/dotlink_walk.h) run on the host against a third brute force (tests/dotlink_walk_check.cpp).  The
refusals of the new entry points are decided before the context is looked at (NULL context, no GPU needed), in the documented
order; join_chains, group_identity and the command line run on the host as well.  Every list is compared exactly."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import dotchain_model as C
import dotlink_model as L
import dotpair_model as P
import dotruns_model as R
from conftest import ROOT, load_jsonl_gz

TRIPLES = [(3, 2, 1), (3, 2, 4), (4, 8, 8), (5, 3, 32), (8, 16, 32)]             # (min_seed, max_gap, max_shift)
# the links of the 159 cases, those with overlap > 0 and those with s < 0: what the model and the brute force agree on
COUNTS = {(3, 2, 1): (6312, 2355, 3109), (3, 2, 4): (12693, 5222, 6302), (4, 8, 8): (4572, 1992, 2288), (5, 3, 32): (2182, 1230, 1104),
          (8, 16, 32): (259, 135, 132)}


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("dotpair.jsonl.gz")


@pytest.fixture(scope="module")
def modelled(golden):
    """{(case index, min_seed, max_gap, max_shift): (every link of the case, sorted; the smallest keys are unique)}, computed once."""
    out = {}
    for k, c in enumerate(golden):
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        every = R.all_runs(raw)
        chains = {}
        for min_seed, max_gap, max_shift in TRIPLES:
            if (min_seed, max_gap) not in chains:
                chains[min_seed, max_gap] = C.all_chains(raw, min_seed, max_gap, every)
            unique = []
            links = L.all_links(chains[min_seed, max_gap], raw.shape[1], min_seed, max_gap, max_shift, unique)
            out[k, min_seed, max_gap, max_shift] = L.select(links, *raw.shape), all(unique)
    return out


def _line_chains(text, min_seed, max_gap):
    """[(first cell, last cell)] of the chains of one line given as a string of 0 and 1."""
    out = []
    for m in re.finditer("1+", text):
        if m.end() - m.start() < min_seed:
            continue
        if out and m.start() - out[-1][1] - 1 <= max_gap:
            out[-1][1] = m.end() - 1
        else:
            out.append([m.start(), m.end() - 1])
    return out


def _brute(raw, min_seed, max_gap, max_shift):
    """Every link, from the lines as strings: per direction {delta: [(i_s, i_e)]}; pred and succ by looking at the 2 max_shift
    neighbouring lines of a chain, the key computed from the definition's words."""
    na, nb = raw.shape
    ov = min(min_seed - 1, L.OVERLAP)
    found = []
    for d in (R.MAIN, R.ANTI):
        cells = raw if d == R.MAIN else raw[:, ::-1]               # (i, c): an anti line is a main line of the flipped matrix
        lines = {}
        for delta in range(-(na - 1), nb):
            i0 = max(0, -delta)
            text = "".join("1" if x else "0" for x in np.diagonal(cells, delta))
            lines[delta] = [(i0 + s, i0 + e) for s, e in _line_chains(text, min_seed, max_gap)]

        def key(x_delta, x_end, y_delta, y_start):
            s = y_delta - x_delta
            gi = y_start - x_end - 1
            g = min(gi, gi + s)
            if not -ov <= g <= max_gap:
                return None
            return (max(g, 0) + abs(s), abs(s), max(-g, 0), s < 0)

        def best(delta, at, forward):
            """The smallest (key, line, chain) among the chains that start behind (forward) or end in front of the cell `at` of line delta."""
            options = []
            for s in range(-max_shift, max_shift + 1):
                other = delta + s if forward else delta - s
                if s == 0 or other not in lines:
                    continue
                for i_s, i_e in lines[other]:
                    k = key(delta, at, other, i_s) if forward else key(other, i_e, delta, at)
                    if k is not None:
                        options.append((k, other, (i_s, i_e)))
            options.sort()
            assert len(options) < 2 or options[0][0] != options[1][0]
            return options[0] if options else None

        for delta, chains in lines.items():
            for i_s, i_e in chains:                                  # Y
                pred = best(delta, i_s, False)
                if pred is None:
                    continue
                k, x_delta, (x_s, x_e) = pred
                succ = best(x_delta, x_e, True)
                if succ[1:] != (delta, (i_s, i_e)):
                    continue
                c_s, c_e = i_s + delta, x_e + x_delta
                found.append((i_s, c_s if d == R.MAIN else nb - 1 - c_s, x_e, c_e if d == R.MAIN else nb - 1 - c_e, d,
                              delta - x_delta, k[0] - k[1], k[2]))
    return np.sort(np.array(found, dtype=L.DTYPE), order=["row", "col", "dir"])


def test_model_agrees_with_a_brute_force_on_every_fixture_case(golden, modelled):
    assert len(golden) == 159
    bad, counts = [], {t: [0, 0, 0] for t in TRIPLES}
    for k, c in enumerate(golden):
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        for triple in TRIPLES:
            got = modelled[(k, *triple)][0]
            if not L.same(got, _brute(raw, *triple)):
                bad.append((c["tag"], triple))
            counts[triple][0] += len(got)
            counts[triple][1] += int((got["overlap"] > 0).sum())
            counts[triple][2] += int((got["shift"] < 0).sum())
    print(counts)
    assert not bad, f"{len(bad)} differ: {bad[:5]}"
    for triple in TRIPLES[:4]:                                   # no vacuous pass: a condition, not a measurement
        assert counts[triple][0] >= 1000 and counts[triple][1] >= 100 and counts[triple][2] >= 100, (triple, counts[triple])
    assert {t: tuple(v) for t, v in counts.items()} == COUNTS


def test_the_smallest_key_is_unique_and_degrees_are_at_most_one(golden, modelled):
    for k, c in enumerate(golden):
        nb = len(c["b"])
        for triple in TRIPLES:
            links, unique = modelled[(k, *triple)]
            assert unique, (c["tag"], triple)
            into = list(zip(links["row"].tolist(), links["col"].tolist(), links["dir"].tolist()))
            out_of = list(zip(links["from_row"].tolist(), links["from_col"].tolist(), links["dir"].tolist()))
            assert len(set(into)) == len(into) and len(set(out_of)) == len(out_of), (c["tag"], triple)
            min_seed, max_gap, max_shift = triple
            assert (np.abs(links["shift"]) >= 1).all() and (np.abs(links["shift"]) <= max_shift).all()
            assert (links["gap"] <= max_gap).all() and (links["overlap"] <= min(min_seed - 1, L.OVERLAP)).all()
            assert not ((links["gap"] > 0) & (links["overlap"] > 0)).any()
            # the row's own arithmetic: g from the two cells
            sign = np.where(links["dir"] == R.MAIN, 1, -1)
            gi = links["row"].astype(np.int64) - links["from_row"].astype(np.int64) - 1
            gc = sign * (links["col"].astype(np.int64) - links["from_col"].astype(np.int64)) - 1
            assert np.array_equal(gc - gi, links["shift"]) and np.array_equal(np.minimum(gi, gc), links["gap"].astype(np.int64) - links["overlap"])
            assert not len(links) or nb > int(links["col"].max())


def test_model_windows_add_up_to_the_whole_list(golden, modelled):
    rng = random.Random(15)
    for k, c in list(enumerate(golden))[::3]:
        na, nb = len(c["a"]), len(c["b"])
        raw = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        every = L.all_links(C.all_chains(raw, 3, 2), nb, 3, 2, 4)
        r, q = rng.randrange(0, na + 1), rng.randrange(0, nb + 1)
        parts = [L.select(every, na, nb, rows, cols) for rows in ((0, r), (r, na + 7)) for cols in ((0, q), (q, None))]
        assert L.same(np.sort(np.concatenate(parts), order=["row", "col", "dir"]), modelled[k, 3, 2, 4][0]), c["tag"]
    # one inserted base in B: the copy is two chains, one line apart, and one link; Y's first cell decides the window
    a = "ACGGTCATTGCAGGCTTAACCGATATCGGA"
    b = a[:15] + "A" + a[15:]                                    # a[14] = 'T', a[15] = 'T': the inserted A lengthens neither run
    only = L.links(a, b, "+", 8, 0, 1, directions="main")
    assert only.tolist() == [(15, 16, 14, 14, R.MAIN, 1, 0, 0)]
    assert L.links(a, b, "+", 8, 0, 1, rows=(15, 16), cols=(16, 17)).tolist() == only.tolist()
    assert len(L.links(a, b, "+", 8, 0, 1, rows=(0, 15))) == 0
    assert L.links(b, a, "+", 8, 0, 1, directions="main").tolist() == [(16, 15, 14, 14, R.MAIN, -1, 0, 0)]     # a deletion: s < 0


# ---- join_chains ----

def _chains(*rows):
    import prf_native
    return np.sort(np.array(list(rows), dtype=prf_native.DOTCHAIN_DTYPE), order=["row", "col", "dir"])


def _links(*rows):
    import prf_native
    return np.sort(np.array(list(rows), dtype=prf_native.DOTLINK_DTYPE), order=["row", "col", "dir"])


def test_join_chains_on_hand_made_lists():
    import prf_native as pn
    # a path of three main chains: 0 -> (+2, gap 1) -> (-1, overlap 3); an anti chain alone; a main chain whose predecessor is missing
    chains = _chains((10, 20, 30, 28, 1, 3), (41, 53, 20, 20, 1, 1), (58, 69, 40, 37, 1, 4), (5, 90, 12, 12, 2, 1), (200, 7, 9, 9, 1, 1))
    links = _links((41, 53, 39, 49, 1, 2, 1, 0), (58, 69, 60, 72, 1, -1, 0, 3), (200, 7, 190, 1, 1, 4, 5, 0))
    groups = pn.join_chains(chains, links, 300)
    assert groups.dtype == np.dtype(pn.DOTGROUP_DTYPE) and len(groups) == 3
    assert [groups[f].tolist() for f in ("row", "col", "dir")] == [[5, 10, 200], [90, 20, 7], [2, 1, 1]]
    path = groups[1]
    assert (int(path["end_row"]), int(path["end_col"]), int(path["span_a"]), int(path["span_b"])) == (97, 108, 88, 89)
    assert int(path["matches"]) == 28 + 20 + 37 - 3                         # the overlap is subtracted once
    assert (int(path["chains"]), int(path["seeds"]), int(path["indel"]), int(path["gap_cells"]), bool(path["open"])) == (3, 8, 3, 1, False)
    alone = groups[0]
    assert (int(alone["end_row"]), int(alone["end_col"]), int(alone["span_a"]), int(alone["span_b"]), int(alone["matches"])) == (16, 79, 12, 12, 12)
    assert (int(alone["chains"]), int(alone["indel"]), bool(alone["open"])) == (1, 0, False)
    begun_outside = groups[2]
    assert bool(begun_outside["open"]) and int(begun_outside["chains"]) == 1 and int(begun_outside["indel"]) == 0
    assert int(begun_outside["matches"]) == 9 and int(begun_outside["gap_cells"]) == 0
    assert np.allclose(pn.group_identity(groups), [1.0, 82 / 89, 1.0]) and pn.group_identity(groups).dtype == np.float64
    # the same path without its links: three groups more
    assert len(pn.join_chains(chains, links[:0], 300)) == 5
    # a missing successor: the chains were filtered
    with pytest.raises(ValueError, match="min_len = 0"):
        pn.join_chains(chains[chains["len"] >= 25], links, 300)
    empty = pn.join_chains(chains[:0], links[:0], 300)
    assert len(empty) == 0 and len(pn.group_identity(empty)) == 0


def test_join_chains_on_the_model_of_a_copy_with_three_indels():
    import prf_native as pn
    rng = random.Random(3)
    noise = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    u = noise(200)
    v = u[:50] + "G" + u[50:100] + u[103:150] + "TT" + u[150:]                # +1 at 50, -3 at 100, +2 at 150
    a, b = noise(30) + u + noise(20), noise(45) + v + noise(35)
    chains = C.chains(a, b, "+", 12, 2, directions="main")
    links = L.links(a, b, "+", 12, 2, 4, directions="main")
    assert len(links) == 3 and sorted(links["shift"].tolist()) == [-3, 1, 2]
    as_chains = np.zeros(len(chains), dtype=pn.DOTCHAIN_DTYPE)
    for f in C.FIELDS:
        as_chains[f] = chains[f]
    as_links = np.zeros(len(links), dtype=pn.DOTLINK_DTYPE)
    for f in L.FIELDS:
        as_links[f] = links[f]
    groups = pn.join_chains(as_chains, as_links, len(b))
    copy = groups[groups["chains"] == 4]
    assert len(copy) == 1 and int(copy["indel"][0]) == 6 and not copy["open"][0]
    assert abs(int(copy["row"][0]) - 30) <= 3 and abs(int(copy["end_row"][0]) - 229) <= 3
    assert 190 <= int(copy["matches"][0]) <= 200 + 6 and int(copy["span_b"][0]) - int(copy["span_a"][0]) == 0
    assert int(groups["chains"].sum()) == len(chains)


# ---- the walks of the kernel, on the host ----

def test_walks_of_the_kernel_against_a_brute_force_on_the_host(tmp_path):
    """csrc/dotlink_walk.h is the text the join kernel runs; the stand-alone program checks it on random lines, under the sanitizers."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/dotlink_walk_check.cpp")
    exe = tmp_path / "walk_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "dotlink_walk_check.cpp")], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    word, lines, stretches, tails, heads = done.stdout.split()
    assert word == "ok" and int(lines) == 4000 and int(stretches) == 160_000 and int(tails) > 10_000 and int(heads) > 10_000


# ---- the C ABI ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def test_entry_points_are_declared_bound_and_exported():
    pn, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prf_dotlink.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(prf_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(pn.DOTLINK_EXPORTS) and len(declared) == 3
    assert not set(declared) & (set(pn.EXPORTS) | set(pn.PERIOD_EXPORTS) | set(pn.DOTPLOT_EXPORTS) | set(pn.DOTPAIR_EXPORTS) | set(pn.DOTRUNS_EXPORTS)
                                | set(pn.DOTCHAIN_EXPORTS))
    assert open(os.path.join(ROOT, "include", "prf.h")).read().count('#include "prf_dotlink.h"') == 1
    assert all(hasattr(lib, name) for name in declared)
    assert lib.prf_abi_version() == 4
    for name, value in (("PRF_DOTLINK_MAX_SHIFT", pn.DOTLINK_MAX_SHIFT), ("PRF_DOTLINK_OVERLAP", pn.DOTLINK_OVERLAP)):
        found = re.search(rf"#define {name} (\d+)u", text)
        assert found and int(found[1]) == value, name
    assert (pn.DOTLINK_MAX_SHIFT, pn.DOTLINK_OVERLAP) == (L.MAX_SHIFT, L.OVERLAP) == (32, 16)
    assert np.dtype(pn.DOTLINK_DTYPE).itemsize == 48 and pn.DOTLINK_DTYPE == L.DTYPE
    struct = re.search(r"typedef struct prf_dotlink \{(.*?)\} prf_dotlink;", text, flags=re.S)[1]
    assert re.findall(r"\b(row|col|from_row|from_col|dir|shift|gap|overlap)\b", struct) == list(L.FIELDS)
    assert "int32_t  shift" in struct or "int32_t shift" in struct


def _call(lib, pn, form, seq_a=b"ACGTACGTAC", seq_b=b"ACGTACGTACGT", a=(0, 10), b=(0, 12), strand=0, rows=(0, 10), cols=(0, 12),
          directions=3, min_seed=3, max_gap=2, max_shift=2, capacity=64, dst=True, n_links=True):
    buf = np.full(64, 0xAB, dtype=np.uint8).repeat(48)
    n, stats = ctypes.c_uint64(77), pn.ScanStats()
    tail = (strand, rows[0], rows[1], cols[0], cols[1], directions, min_seed, max_gap, max_shift, buf.ctypes.data if dst else None, capacity,
            ctypes.byref(n) if n_links else None, ctypes.byref(stats))
    if form == "one_shot":
        arr_a, _keep_a = pn._contig_array([seq_a])
        arr_b, _keep_b = pn._contig_array([seq_b])
        rc = lib.prf_dotpair_links_seq(None, arr_a, *a, arr_b, *b, *tail)
    elif form == "ex":
        rc = lib.prf_dotpair_links_ex(None, None, 0, *a, 1, *b, *tail, 4096)
    else:
        rc = lib.prf_dotpair_links(None, None, 0, *a, 1, *b, *tail)
    assert (buf == 0xAB).all() and n.value == 77                              # a refused call writes nothing
    return rc


# each case breaks one rule and every rule behind it: the first in the documented order is the one reported
LATER = dict(rows=(5, 4), cols=(9, 2), strand=2, directions=4, min_seed=0, max_gap=4097, max_shift=0, capacity=(1 << 24) + 1, dst=False,
             n_links=False)


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
    (_later("rows", "cols", "strand", "directions", "min_seed", "max_gap"), "PRF_EINVAL", "max_shift is 0"),
    (dict(_later("rows", "cols", "strand", "directions", "min_seed", "max_gap"), max_shift=33), "PRF_EUNSUPPORTED", "PRF_DOTLINK_MAX_SHIFT"),
    (_later("rows", "cols", "strand", "directions", "min_seed", "max_gap", "max_shift"), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_ROWS"),
    (dict(dst=False, n_links=False), "PRF_EINVAL", "NULL n_links"),
    (dict(dst=False), "PRF_EINVAL", "NULL destination"),
    (dict(dst=False, capacity=0), "PRF_EINVAL", "NULL context"),              # counting only is a valid call
    (dict(strand=0xFFFFFFFF), "PRF_EINVAL", "strand"),
    (dict(max_gap=0xFFFFFFFF), "PRF_EUNSUPPORTED", "PRF_DOTCHAIN_MAX_GAP"),
    (dict(max_shift=0xFFFFFFFF), "PRF_EUNSUPPORTED", "PRF_DOTLINK_MAX_SHIFT"),
    (dict(), "PRF_EINVAL", "NULL context"),                                   # valid arguments
    (dict(max_gap=4096, max_shift=32, min_seed=1 << 40, capacity=1 << 24), "PRF_EINVAL", "NULL context"),
    (dict(strand=1, directions=1, max_gap=0, max_shift=1), "PRF_EINVAL", "NULL context"),
    (dict(directions=2, rows=(3, 3), a=(4, 4)), "PRF_EINVAL", "NULL context"),
]


@pytest.mark.parametrize("kwargs,code,text", ORDER)
@pytest.mark.parametrize("form", ["genome", "ex", "one_shot"])
def test_refusals_in_the_documented_order(form, kwargs, code, text):
    pn, lib = _lib()
    rc = _call(lib, pn, form, **kwargs)
    assert rc == getattr(pn, code)
    message = lib.prf_last_error().decode()
    assert text in message and message.startswith("prf_dotpair_links")


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
        rc = lib.prf_dotpair_links_seq(None, first, 0, 4, second, 0, 4, 0, 0, 4, 0, 4, 3, 2, 1, 1, None, 0, ctypes.byref(n), ctypes.byref(stats))
        assert rc == pn.PRF_EINVAL and "NULL sequence" in lib.prf_last_error().decode()
    big = (pn._Contig * 1)()                                                  # 2^44 cells: judged from the lengths, the sequences are never read
    block = ctypes.create_string_buffer(16)
    big[0].ascii, big[0].len = ctypes.addressof(block), 1 << 22
    rc = lib.prf_dotpair_links_seq(None, big, 0, 1 << 22, big, 0, 1 << 22, 1, 0, 1 << 22, 0, 1 << 22, 3, 64, 8, 4, None, 0, ctypes.byref(n),
                                   ctypes.byref(stats))
    assert rc == pn.PRF_EUNSUPPORTED and "PRF_DOT_MAX_CELLS" in lib.prf_last_error().decode()


def test_binding_checks_its_arguments_before_the_library():
    pn, _lib_ = _lib()
    g, other = pn.Genome(None, None, 2, [100, 50]), pn.Genome(None, None, 1, [100])
    with pytest.raises(ValueError, match="contig 2"):
        g.dotpair_links((0, 0, None), (2, 0, None), min_seed=4, max_gap=2, max_shift=1)
    with pytest.raises(ValueError, match="strand"):
        g.dotpair_links((0, 0, None), (1, 0, None), strand="x")
    with pytest.raises(ValueError, match="directions"):
        g.dotpair_links((0, 0, None), (1, 0, None), directions="up")
    with pytest.raises(ValueError, match="min_seed"):
        g.dotpair_links((0, 0, None), (1, 0, None), min_seed=0)
    with pytest.raises(ValueError, match="max_gap"):
        g.dotpair_links((0, 0, None), (1, 0, None), min_seed=4, max_gap=4097)
    for max_shift in (0, 33, -1, True):
        with pytest.raises(ValueError, match="max_shift"):
            g.dotpair_links((0, 0, None), (1, 0, None), min_seed=4, max_gap=1, max_shift=max_shift)
    with pytest.raises(ValueError, match="cols"):
        g.dotpair_links((0, 0, None), (1, 0, None), cols=(5, 4))
    with pytest.raises(ValueError, match="same resident genome"):
        pn._links(None, (g, 0), (0, None), (other, 0), (0, None), "+", "both", 3, 1, 1, None, None, False, 0)
    with pytest.raises(ValueError, match="both be sequences or both"):
        pn._links(None, (g, 0), (0, None), "ACGT", (0, None), "+", "both", 3, 1, 1, None, None, False, 0)
    g._h = other._h = None


# ---- command line ----

def _parse(cli, argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    return cli.resolve_inputs(args, parser), cli.resolve_versus(args, parser), args


def test_cli_parses_the_groups_options(tmp_path, capsys):
    import plot_dot_plot as cli
    base = ["ACGTACGT", "--groups-tsv", "g.tsv", "--min-seed", "4", "--max-gap", "2", "--max-shift", "3"]
    args = _parse(cli, base)[2]
    assert (args.groups_tsv, args.min_seed, args.max_gap, args.max_shift, args.min_group, args.min_identity, args.run_directions) == (
        "g.tsv", 4, 2, 3, None, None, "both")
    assert cli.no_image(args) and args.chains_tsv is None and args.runs_tsv is None
    args = _parse(cli, base + ["--min-group", "30", "--min-identity", "0.9", "--run-directions", "anti"])[2]
    assert (args.min_group, args.min_identity, args.run_directions) == (30, 0.9, "anti")
    assert not cli.no_image(_parse(cli, base + ["-o", "x.png"])[2])
    both = _parse(cli, base + ["--chains-tsv", "c.tsv", "--min-chain", "5"])[2]                 # the two lists share their options
    assert (both.chains_tsv, both.groups_tsv, both.min_chain) == ("c.tsv", "g.tsv", 5)
    # nothing changes for a command line without the new options
    out, _, args = _parse(cli, ["ACGTACGT", "-d", str(tmp_path)])
    assert out == [("sequence", 0, "ACGTACGT", str(tmp_path / "dot_plot.png"))] and args.groups_tsv is None and not cli.no_image(args)
    assert cli.no_image(_parse(cli, ["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "1"])[2])
    long_fa = tmp_path / "x.fa"
    long_fa.write_text(">chrA\n" + "ACGTTGCA" * 1000 + "\n")
    out, versus, _ = _parse(cli, ["-R", str(long_fa), "chrA:100-7100", "--versus", "chrA:500-6500", "--groups-tsv", "g.tsv", "--min-seed", "12",
                                  "--max-gap", "8", "--max-shift", "32"])
    assert len(out[0][2]) == 7000 and versus[:2] == ("chrA", 500) and len(versus[2]) == 6000
    assert "BOTH mirror images" in " ".join(cli.build_parser().format_help().split())
    capsys.readouterr()
    short = ["ACGT", "--groups-tsv", "g.tsv"]
    for argv, text in ((short, "--max-shift"), (short + ["--min-seed", "4", "--max-gap", "1"], "--max-shift"),
                       (short + ["--max-gap", "4", "--max-shift", "1"], "--min-seed"),
                       (["ACGT", "--max-shift", "5"], "--groups-tsv"), (["ACGT", "--min-group", "5"], "--groups-tsv"),
                       (["ACGT", "--min-seed", "5"], "--chains-tsv or --groups-tsv"),
                       (short + ["--min-seed", "4", "--max-gap", "1", "--max-shift", "1", "--min-chain", "3"], "--min-chain goes with --chains-tsv"),
                       (["ACGT", "--chains-tsv", "c.tsv", "--min-seed", "4", "--max-gap", "1", "--max-shift", "1"], "--groups-tsv"),
                       (short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "0"], "between 1 and 32"),
                       (short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "33"], "between 1 and 32"),
                       (short + ["--min-seed", "0", "--max-gap", "1", "--max-shift", "1"], "at least 1"),
                       (short + ["--min-seed", "3", "--max-gap", "4097", "--max-shift", "1"], "between 0 and 4096"),
                       (short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "1", "--min-group", "-2"], "at least 0"),
                       (short + ["--min-seed", "3", "--max-gap", "1", "--max-shift", "1", "--min-identity", "1.5"], "between 0 and 1"),
                       (["ACGT", "TTGA", "--groups-tsv", "g.tsv", "--min-seed", "3", "--max-gap", "1", "--max-shift", "1"], "takes one input"),
                       (["-R", str(long_fa), "chrA:0-7000", "--groups-tsv", "g.tsv", "--min-seed", "30", "--max-gap", "1", "--max-shift", "2", "-o",
                         "x.png"], "--block")):
        with pytest.raises(SystemExit):
            _parse(cli, argv)
        assert text in capsys.readouterr().err, argv


def test_group_lines_are_in_genomic_coordinates():
    import plot_dot_plot as cli
    import prf_native
    groups = np.zeros(2, dtype=prf_native.DOTGROUP_DTYPE)
    groups[0] = (5, 9, 104, 110, 100, 102, 95, 3, 1, 3, 7, 2, False)
    groups[1] = (0, 50, 19, 30, 20, 21, 20, 0, 2, 2, 2, 1, True)
    assert list(cli.group_lines("chr1", 100, "chrX", 1000, "-", groups)) == [
        "chr1\t105\t205\tchrX\t1009\t1111\t-\tmain\t100\t102\t95\t3\t7\t2\t3\t0\t0.9314\n",
        "chr1\t100\t120\tchrX\t1030\t1051\t-\tanti\t20\t21\t20\t2\t2\t1\t0\t1\t0.9524\n"]


class _StubContext:
    """Serves dotpair_chains and dotpair_links from the models, so that the command line's path runs without a GPU."""

    def __init__(self):
        self.calls = []

    def dotpair_chains(self, seq_a, seq_b, strand="+", directions="both", min_seed=16, max_gap=0, min_len=0):
        import prf_native
        self.calls.append(("chains", len(seq_a), len(seq_b), strand, directions, min_seed, max_gap, min_len))
        got = C.chains(seq_a, seq_b, strand, min_seed, max_gap, min_len, directions=directions)
        out = np.zeros(len(got), dtype=prf_native.DOTCHAIN_DTYPE)
        for f in C.FIELDS:
            out[f] = got[f]
        return out

    def dotpair_links(self, seq_a, seq_b, strand="+", directions="both", min_seed=16, max_gap=0, max_shift=1):
        import prf_native
        self.calls.append(("links", len(seq_a), len(seq_b), strand, directions, min_seed, max_gap, max_shift))
        got = L.links(seq_a, seq_b, strand, min_seed, max_gap, max_shift, directions=directions)
        out = np.zeros(len(got), dtype=prf_native.DOTLINK_DTYPE)
        for f in L.FIELDS:
            out[f] = got[f]
        return out


def test_cli_writes_the_groups_of_stubbed_lists(tmp_path, capsys):
    import plot_dot_plot as cli
    rng = random.Random(21)
    noise = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    u = noise(90)
    v = u[:30] + "GG" + u[30:60] + u[61:]                       # two bases inserted behind 30, one deleted at 60
    chrom = noise(290) + u + noise(120)
    other = noise(70) + P.revcomp(v.encode()).decode() + noise(69)
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + chrom + "\n")
    tsv, ctx = tmp_path / "groups.tsv", _StubContext()
    common = ["-R", str(fa), "chrT:250-450", "--versus", "other:50-200", "--strand", "both", "--groups-tsv", str(tsv), "-d", str(tmp_path),
              "--min-seed", "12", "--max-gap", "1"]
    cli.main(common + ["--max-shift", "2", "--min-group", "60"], context=ctx)
    assert ctx.calls == [("chains", 200, 150, "+", "both", 12, 1, 0), ("links", 200, 150, "+", "both", 12, 1, 2),
                         ("chains", 200, 150, "-", "both", 12, 1, 0), ("links", 200, 150, "-", "both", 12, 1, 2)]
    lines = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert len(lines) == 1 and len(lines[0]) == 17
    name, a0, a1, x_name, b0, b1, strand, direction, span_a, span_b, matches, chains, seeds, indel, gap_cells, is_open, identity = lines[0]
    assert (name, x_name, strand, direction, chains, indel, is_open) == ("chrT", "other", "-", "anti", "3", "3", "0")
    assert abs(int(a0) - 290) <= 3 and abs(int(a1) - 380) <= 3 and abs(int(b0) - 70) <= 3 and abs(int(b1) - 161) <= 3
    assert int(span_a) == int(a1) - int(a0) and int(span_b) == int(b1) - int(b0) == int(span_a) + 1
    assert 85 <= int(matches) <= int(span_a) and identity == f"{int(matches) / int(span_b):.4f}"
    assert not list(tmp_path.glob("*.png")) and "dot plot(s) written" not in capsys.readouterr().out     # no -o: no image
    cli.main(common + ["--max-shift", "1", "--min-group", "50"], context=ctx)                    # the junction of two lines is out of reach
    assert [line.split("\t")[11] for line in tsv.read_text().splitlines()] == ["2"] and ctx.calls[-1][-1] == 1
    cli.main(common + ["--max-shift", "2", "--min-group", "60", "--min-identity", "0.999"], context=ctx)     # filtered on the host
    assert tsv.read_text() == ""
    # without --versus: both mirror images and the trivial diagonal
    seq = chrom[285:385] + "ACGTTC" + v
    cli.main([seq, "--groups-tsv", str(tsv), "--min-seed", "12", "--max-gap", "1", "--max-shift", "2", "--min-group", "60", "--run-directions", "main",
              "-d", str(tmp_path)], context=ctx)
    lines = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert ctx.calls[-2:] == [("chains", len(seq), len(seq), "+", "main", 12, 1, 0), ("links", len(seq), len(seq), "+", "main", 12, 1, 2)]
    assert len(lines) == 3 and sorted(line[11] for line in lines) == ["1", "3", "3"]
    assert [line[1:3] + line[4:6] for line in lines if line[11] == "1"] == [["0", str(len(seq)), "0", str(len(seq))]]


# ---- the planted junctions of the GPU tests ----

def test_planted_junctions_hold_what_they_claim():
    """tests/dotlink_cases.py on the model: every band has the one link its case names, or none (the plus strand; the minus
    strand's bands are the same letters complemented)."""
    import dotlink_cases as K
    rows, columns, where = K.build()
    assert len(rows) == K.ROWS and set(rows) <= set(b"ACGTN") and set(columns["+"]) <= set(b"ACGTN")      # the 3-plane kernels
    for (name, d), band in where["+"].items():
        chains, links = K.expected(rows, columns["+"], band, "+", K.CASES[name][2])
        K.check_claim(name, links, d)
        assert len(chains) >= 2, name
    long_one = K.expected(rows, columns["+"], where["+"]["a predecessor of more than F cells", R.MAIN], "+", (K.S, K.G, K.D))[0]
    assert int(long_one["len"].max()) > K.FOLLOW
