"""GPU (-m gpu): the list of junctions between the chains of the dot plot of two ranges (prf_dotpair_links, csrc/dotlink.hip,
DESIGN 15) and the gapped repeats prf_native.join_chains folds them into.  Every list is compared EXACTLY with the model
(tests/dotlink_model.py, pinned to a brute force by tests/test_dotlink_cpu.py).

Shapes: the fixture's cases (at most 200 x 200); planted junctions (tests/dotlink_cases.py) in a genome of ACGT and N (the
3-plane kernels), each a copied piece with an insertion, a deletion, changed bases or a homopolymer run at the breakpoint, as main
and anti lines on both strands, looked at through windows of 3 x 3 cells around the successor's start; two sequences of 333 and
517 letters with IUPAC letters (the 8-plane kernels) whose copies with indels lie in the corners of their rectangle, at a
min_seed at which chance supplies rival tails and rival heads by the hundred."""
import ctypes
import random

import numpy as np
import pytest

import dotchain_model as C
import dotlink_cases as K
import dotlink_model as L
import dotpair_model as P
import dotruns_model as R
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu

TRIPLES = [(3, 2, 1), (3, 2, 4), (4, 8, 8), (5, 3, 32), (8, 16, 32)]             # (min_seed, max_gap, max_shift): the fixture


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    cases = load_jsonl_gz("dotpair.jsonl.gz")
    for c in cases:                                            # the raw cells, their runs and their chains once, for the five triples
        c["raw"] = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        c["every"] = R.all_runs(c["raw"])
        c["chains"] = {}
    return cases


def _same(got, want, what=None):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in L.FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, got[f][:8], want[f][:8])


def _random(n, seed, alphabet=b"ACGT"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---- 1. the fixture ----

@pytest.mark.parametrize("min_seed,max_gap,max_shift", TRIPLES)
def test_every_fixture_case_through_the_one_shot_call(ctx, golden, min_seed, max_gap, max_shift):
    bad, found, overlapping, negative = [], 0, 0, 0
    assert len(golden) == 159
    for c in golden:
        na, nb = c["raw"].shape
        if (min_seed, max_gap) not in c["chains"]:
            c["chains"][min_seed, max_gap] = C.all_chains(c["raw"], min_seed, max_gap, c["every"])
        chains = c["chains"][min_seed, max_gap]
        got, st = ctx.dotpair_links(c["a"], c["b"], c["strand"], "both", min_seed, max_gap, max_shift, with_stats=True)
        want = L.select(L.all_links(chains, nb, min_seed, max_gap, max_shift), na, nb)
        if not L.same(got, want):
            bad.append(c["tag"])
        found, overlapping, negative = found + len(want), overlapping + int((want["overlap"] > 0).sum()), negative + int((want["shift"] < 0).sum())
        assert st.path == 9 and st.positions == na + nb and st.n_hits == len(got)
        assert st.n_candidates == len(chains)                  # the chain heads of the window, which is the whole rectangle
        assert (st.scan_ms > 0 and st.n_launches >= 1) or not (na and nb)
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"
    floor = (1000, 100, 100) if max_gap != 16 else (100, 50, 50)                # no vacuous pass
    assert found >= floor[0] and overlapping >= floor[1] and negative >= floor[2]


# ---- 2. where the kernels can go wrong: planted junctions ----

@pytest.fixture(scope="module")
def junctions(ctx):
    """The genome of tests/dotlink_cases.py (contig 0: the rows; contigs 1 and 2: the columns for the plus and the minus strand)
    and, per strand and band, the model's chains and links of the rows x the band's columns."""
    rows, columns, where = K.build()
    want = {}
    for strand in "+-":
        for (name, d), band in where[strand].items():
            want[strand, name, d] = K.expected(rows, columns[strand], band, strand, K.CASES[name][2])
            K.check_claim(name, want[strand, name, d][1], d)
    g = ctx.load([rows, columns["+"], columns["-"]], 64)
    yield g, where, want
    g.free()


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("d", [R.MAIN, R.ANTI])
def test_planted_junctions_through_windows_around_the_successor(junctions, strand, d):
    g, where, want = junctions
    a, b = (0, 0, None), (1 if strand == "+" else 2, 0, None)
    links_seen = 0
    for name, (_i, _ops, (min_seed, max_gap, max_shift), claim) in K.CASES.items():
        band = where[strand][name, d]
        chains, links = want[strand, name, d]
        # the band's columns over all rows: the model's list of the band, whatever lies in the other bands
        got, st = g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, cols=(band[0] - 3, band[1] + 3), with_stats=True)
        _same(got, links, (strand, d, name))
        assert st.n_candidates == len(chains) and st.n_hits == len(links) and st.path == 9
        other = "anti" if d == R.MAIN else "main"
        assert len(g.dotpair_links(a, b, strand, other, min_seed, max_gap, max_shift, cols=(band[0] - 3, band[1] + 3))) == 0
        # a window of 3 x 3 cells around every chain's start: the link into that chain, if it has one, and no other
        for row, col in zip(chains["row"].tolist(), chains["col"].tolist()):
            mine = links[(links["row"] == row) & (links["col"] == col)]
            got, st = g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, rows=(max(0, row - 1), row + 2), cols=(col - 1, col + 2),
                                      with_stats=True)
            _same(got, mine, (strand, d, name, row, col))
            near = (chains["row"] + 1 >= row) & (chains["row"] < row + 2) & (chains["col"] + 1 >= col) & (chains["col"] < col + 2)
            assert st.n_candidates == int(near.sum()) >= 1
            links_seen += len(mine)
        for link in links:                                     # a link is present only where the successor's first cell lies
            row, col = int(link["row"]), int(link["col"])
            assert len(g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, rows=(row, row + 1), cols=(col, col + 1))) == 1
            for rows, cols in (((row + 1, row + 4), (col - 3, col + 4)), ((max(0, row - 3), row), (col - 3, col + 4)),
                               ((row, row + 1), (col + 1, col + 4)), ((row, row + 1), (col - 3, col))):
                assert len(g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, rows=rows, cols=cols)) == 0, (name, rows, cols)
            around = (int(link["from_row"]), int(link["from_col"]))                               # ... not where the predecessor ends
            if abs(around[0] - row) > 1 or abs(around[1] - col) > 1:
                assert len(g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, rows=(around[0], around[0] + 1),
                                           cols=(around[1], around[1] + 1))) == 0
    assert links_seen == sum(1 for case in K.CASES.values() if case[3] is not None)


def test_the_long_predecessor_and_all_64_lanes(junctions):
    import prf_native
    g, where, want = junctions
    chains, links = want["+", "a predecessor of more than F cells", R.MAIN]
    x = chains[chains["row"] == 7]
    assert len(x) == 1 and int(x["len"][0]) > prf_native.DOTCHAIN_FOLLOW == K.FOLLOW and len(links) == 1
    assert int(links["from_row"][0]) == 7 + int(x["len"][0]) - 1 and int(links["row"][0]) > K.FOLLOW
    for name, shift in (("a shift of 32", 32), ("a shift of -32", -32)):
        for d in (R.MAIN, R.ANTI):
            assert want["-", name, d][1]["shift"].tolist() == [shift]                             # lanes 0 and 63 of the wave


@pytest.mark.parametrize("strand", ["+", "-"])
def test_strips_cut_into_one_launch_per_tile_row(junctions, strand):
    g, where, want = junctions
    a, b = (0, 0, None), (1 if strand == "+" else 2, 0, None)
    for d in (R.MAIN, R.ANTI):
        for name in ("a junction across a tile row", "a predecessor of more than F cells"):
            min_seed, max_gap, max_shift = K.CASES[name][2]
            band = where[strand][name, d]
            chains, links = want[strand, name, d]
            assert len(links) == 1
            row, col = int(links["row"][0]), int(links["col"][0])
            rows, cols = (max(0, row - 200), row + 70), (col - 1, col + 2)                        # a strip of 3 columns over 5 tile rows
            keep = (links["row"] >= rows[0]) & (links["row"] < rows[1]) & (links["col"] >= cols[0]) & (links["col"] < cols[1])
            whole, st1 = g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, rows=rows, cols=cols, with_stats=True)
            _same(whole, links[keep], (name, d))
            cut, st = g.dotpair_links(a, b, strand, "both", min_seed, max_gap, max_shift, rows=rows, cols=cols, with_stats=True,
                                      launch_cells=64 * (cols[1] - cols[0]))                      # one tile of rows per launch
            _same(cut, links[keep], (name, d, "cut"))
            assert st.n_launches - st1.n_launches == -(-(rows[1] - rows[0]) // 64) - 1 and st.n_candidates == st1.n_candidates >= 1


def _with_indels(piece, seed, tr=bytes):
    """tr(piece) with a base inserted or removed every 30 to 50 letters and a base changed now and then."""
    rng = random.Random(seed)
    out, at = bytearray(), 0
    while at < len(piece):
        step = rng.randrange(30, 51)
        part = bytearray(piece[at:at + step])
        if len(part) > 20 and part[11] in b"ACGT":
            part[11] = b"ACGT"[(b"ACGT".index(part[11]) + 1) % 4]
        out += part
        at += step
        if rng.random() < 0.5:
            out += bytes([rng.choice(b"ACGT")]) * rng.randrange(1, 3)
        else:
            at += rng.randrange(1, 4)
    return tr(bytes(out))


def _corner_sequences(strand):
    """Two sequences of 333 and 517 letters (the rows, the columns) with copies that hold indels in the corners of their
    rectangle: from (0, 0), from row 0, from column 0, up to (na, nb), an anti copy from (0, nb - 1) and one down to column 0;
    an N block and an R / Y stretch inside a copy."""
    tr = P.comp if strand == "-" else bytes
    a, b = bytearray(_random(333, 23)), bytearray(_random(517, 24))
    a[95:101], a[110:116] = b"NNNNNN", b"RRYYRY"                # inside a[80:170]
    a[0:60] = a[333 - 60:][::-1]                                # with b's tail below: an anti copy from (0, nb - 1)
    b[0:len(_with_indels(a[0:70], 1))] = _with_indels(a[0:70], 1, tr)             # from (0, 0)
    piece = _with_indels(a[80:170], 2, tr)                                        # through the N block and the R / Y stretch
    b[150:150 + len(piece)] = piece
    piece = _with_indels(a[333 - 80:], 3, tr)                                     # up to (na, nb)
    b[517 - len(piece):] = piece
    piece = _with_indels(tr(bytes(b[0:45]))[::-1], 4)                             # an anti copy that ends at column 0
    a[230:230 + len(piece)] = piece
    return bytes(a[:333]), bytes(b[:517])


@pytest.mark.parametrize("strand", ["+", "-"])
def test_junctions_at_the_corners_with_rival_tails_and_rival_heads(ctx, strand):
    """The rows are the LAST contig (a look ahead behind the planes' last word) and the columns contig 0 from b_begin = 0 (an anti
    line's look backwards reaches in front of the planes); then the other way round.  IUPAC letters: the 8-plane kernels.  At
    min_seed 3 chance supplies what a planted case could only show once: chains with several candidates (a nearer rival
    tail on another line) and chains whose best predecessor prefers another head."""
    a, b = _corner_sequences(strand)
    g = ctx.load([b, a], 64)
    try:
        for rows_of, cols_of, sa, sb in (((1, 0, None), (0, 0, None), a, b), ((0, 0, None), (1, 0, None), b, a)):
            raw = P.kept_cells(sa, sb, strand, 0)
            every = R.all_runs(raw)
            na, nb = raw.shape
            for min_seed, max_gap, max_shift in ((3, 2, 4), (3, 1, 1), (4, 3, 32), (5, 64, 8), (6, 4096, 32), (9, 0, 3)):
                chains = C.all_chains(raw, min_seed, max_gap, every)
                want = L.select(L.all_links(chains, nb, min_seed, max_gap, max_shift), na, nb)
                _same(g.dotpair_links(rows_of, cols_of, strand, "both", min_seed, max_gap, max_shift), want,
                      (strand, rows_of[0], min_seed, max_gap, max_shift))
                if (min_seed, max_gap, max_shift) != (3, 2, 4):
                    continue
                rivals = jilted = 0
                linked = {(r, c, d) for r, c, d in zip(want["row"].tolist(), want["col"].tolist(), want["dir"].tolist())}
                for d in (R.MAIN, R.ANTI):
                    at, key, _s, _g = L.key_matrix(chains, nb, d, min_seed, max_gap, max_shift)
                    n_candidates = (key < L.NONE).sum(axis=0)
                    heads = chains[at]
                    for y in np.flatnonzero(n_candidates >= 1)[:60]:
                        start = (int(heads["row"][y]), int(heads["col"][y]), d)
                        rivals += int(n_candidates[y] >= 2)
                        jilted += start not in linked
                        got = g.dotpair_links(rows_of, cols_of, strand, "both", min_seed, max_gap, max_shift, rows=(start[0], start[0] + 1),
                                              cols=(start[1], start[1] + 1))
                        got = got[got["dir"] == d]
                        assert len(got) == (start in linked), start
                        if len(got):
                            x = int(key[:, y].argmin())                        # the nearest tail, and no other
                            n = int(heads["len"][x]) - 1
                            assert int(got["from_row"][0]) == int(heads["row"][x]) + n
                            assert int(got["from_col"][0]) == int(heads["col"][x]) + (n if d == R.MAIN else -n)
                assert rivals >= 10 and jilted >= 10, (rivals, jilted)
            # the copies with indels, joined: groups that start or end in the corners
            chains = g.dotpair_chains(rows_of, cols_of, strand, "both", 6, 2)
            links = g.dotpair_links(rows_of, cols_of, strand, "both", 6, 2, 3)
            import prf_native
            groups = prf_native.join_chains(chains, links, nb)
            assert int(groups["chains"].sum()) == len(chains) and len(groups) == len(chains) - len(links) and not groups["open"].any()
            joined = groups[(groups["chains"] >= 2) & (groups["matches"] >= 40)]
            assert len(joined) >= 3, groups[groups["chains"] >= 2]
    finally:
        g.free()


# ---- 3. capacity, windows, determinism, join_chains, neighbours ----

def _call(g, a, b, strand, directions, min_seed, max_gap, max_shift, capacity, dst, rows=(0, 1 << 62), cols=(0, 1 << 62)):
    import prf_native
    n, st = ctypes.c_uint64(0), prf_native.ScanStats()
    rc = g.ctx.lib.prf_dotpair_links(g.ctx._h, g._h, a[0], a[1], a[2], b[0], b[1], b[2], strand, rows[0], rows[1], cols[0], cols[1],
                                     directions, min_seed, max_gap, max_shift, None if dst is None else dst.ctypes.data, capacity,
                                     ctypes.byref(n), ctypes.byref(st))
    assert rc == prf_native.PRF_OK, g.ctx.lib.prf_last_error()
    return n.value, st


@pytest.fixture(scope="module")
def two_randoms(ctx):
    """Two contigs of 700 and 900 random letters, the second with pieces of the first that hold indels."""
    a = bytearray(_random(700, 51))
    b = bytearray(_random(900, 52))
    for at, (lo, hi), seed in ((40, (100, 300), 5), (420, (350, 640), 6)):
        piece = _with_indels(bytes(a[lo:hi]), seed)
        b[at:at + len(piece)] = piece
    seqs = [bytes(a), bytes(b[:900])]
    g = ctx.load(seqs, 64)
    raw = P.kept_cells(seqs[0], seqs[1], "+", 0)
    yield g, seqs, raw, R.all_runs(raw)
    g.free()


def test_capacity_counts_fills_or_leaves_the_destination_alone(two_randoms):
    import prf_native
    g, seqs, raw, every = two_randoms
    a, b = (0, 0, 1 << 40), (1, 0, 1 << 40)
    want = L.select(L.all_links(C.all_chains(raw, 4, 3, every), raw.shape[1], 4, 3, 8), *raw.shape)
    n = len(want)
    assert n > 300 and int((want["overlap"] > 0).sum()) > 30
    assert _call(g, a, b, 0, 3, 4, 3, 8, 0, None)[0] == n                      # counting only
    dst = np.full(n + 8, 0xEE, dtype=np.uint8).repeat(48).view(prf_native.DOTLINK_DTYPE)
    sentinel = dst.copy()
    count, st = _call(g, a, b, 0, 3, 4, 3, 8, n - 1, dst)
    assert count == n and st.n_hits == n and np.array_equal(dst.view(np.uint8), sentinel.view(np.uint8))      # untouched
    assert _call(g, a, b, 0, 3, 4, 3, 8, n, dst)[0] == n                       # exactly enough: filled
    _same(dst[:n], want)
    assert np.array_equal(dst[n:].view(np.uint8), sentinel[n:].view(np.uint8))
    rc = g.ctx.lib.prf_dotpair_links(g.ctx._h, g._h, 1, 0, 10, 3, 0, 10, 0, 0, 10, 0, 10, 3, 2, 1, 1, None, 0, ctypes.byref(ctypes.c_uint64(0)), None)
    assert rc == prf_native.PRF_EINVAL and "contig 3" in g.ctx.lib.prf_last_error().decode()


def test_windows_add_up_and_two_calls_give_equal_arrays(two_randoms):
    g, seqs, raw, every = two_randoms
    a, b = (0, 0, None), (1, 0, None)
    whole = g.dotpair_links(a, b, "+", "both", 3, 2, 4)
    _same(whole, L.select(L.all_links(C.all_chains(raw, 3, 2, every), raw.shape[1], 3, 2, 4), *raw.shape))
    assert len(whole) > 1_000 and np.array_equal(whole, g.dotpair_links(a, b, "+", "both", 3, 2, 4))          # determinism
    for row_cuts, col_cuts in (((0, 131, 9_999), (0, 257, None)), ((0, 64, 300, 700), (0, None))):             # 2 x 2 and 3 x 1
        parts = [g.dotpair_links(a, b, "+", "both", 3, 2, 4, rows=(r0, r1), cols=(c0, c1))
                 for r0, r1 in zip(row_cuts, row_cuts[1:]) for c0, c1 in zip(col_cuts, col_cuts[1:])]
        assert all(len(p) for p in parts)
        _same(np.sort(np.concatenate(parts), order=["row", "col", "dir"]), whole, row_cuts)                  # each once, unclipped
    for directions in ("main", "anti"):
        _same(g.dotpair_links(a, b, "+", directions, 3, 2, 4), whole[whole["dir"] == R.DIRECTIONS[directions][0]], directions)


def _as(dtype, rows):
    out = np.zeros(len(rows), dtype=dtype)
    for f in rows.dtype.names:
        out[f] = rows[f]
    return out


def test_join_chains_on_a_planted_copy_with_three_indels(ctx):
    import prf_native
    u = _random(240, 61)
    v = u[:60] + b"G" + u[60:120] + u[123:180] + b"TT" + u[180:]               # +1 at 60, -3 at 120, +2 at 180
    a = _random(29, 62) + b"A" + u + b"A" + _random(19, 63)                   # A against C in front of and behind the copy:
    b = _random(44, 64) + b"C" + v + b"C" + _random(34, 65)                   # chance lengthens neither end
    for strand, cols in (("+", b), ("-", P.comp(b))):
        chains = ctx.dotpair_chains(a, cols, strand, "main", 14, 2)
        links = ctx.dotpair_links(a, cols, strand, "main", 14, 2, 4)
        assert len(links) == 3 and sorted(links["shift"].tolist()) == [-3, 1, 2]
        _same(links, L.links(a, cols, strand, 14, 2, 4, directions="main"))
        groups = prf_native.join_chains(chains, links, len(cols))
        modelled = prf_native.join_chains(_as(prf_native.DOTCHAIN_DTYPE, C.chains(a, cols, strand, 14, 2, directions="main")),
                                          _as(prf_native.DOTLINK_DTYPE, L.links(a, cols, strand, 14, 2, 4, directions="main")), len(cols))
        assert np.array_equal(groups, modelled)
        copy = groups[groups["chains"] == 4]
        assert len(copy) == 1 and len(groups) == len(chains) - 3
        only = copy[0]
        # the copy begins and ends where it was planted; every base of u that v holds matches once, overlaps are counted once
        assert (int(only["row"]), int(only["col"]), int(only["end_row"]), int(only["end_col"])) == (30, 45, 269, 284)
        assert (int(only["span_a"]), int(only["span_b"]), int(only["indel"]), bool(only["open"])) == (240, 240, 6, False)
        assert int(only["matches"]) == 237 and int(only["gap_cells"]) == 0
        assert prf_native.group_identity(copy)[0] == 237 / 240
        # the same through a window that holds the last three chains only: the group is open
        rows = (100, 400)
        part = prf_native.join_chains(ctx.dotpair_chains(a, cols, strand, "main", 14, 2, rows=rows),
                                      ctx.dotpair_links(a, cols, strand, "main", 14, 2, 4, rows=rows), len(cols))
        assert part["open"].tolist().count(True) == 1 and int(part[part["open"]]["chains"][0]) == 2
        with pytest.raises(ValueError, match="min_len = 0"):
            prf_native.join_chains(ctx.dotpair_chains(a, cols, strand, "main", 14, 2, 70), links, len(cols))


def test_scans_runs_and_chains_are_not_disturbed(ctx):
    import torch
    import prf_native
    tile = prf_native.tile_positions()
    seq = bytearray(_random(3 * tile + 500, 13))
    for at in range(1000, len(seq) - 200, 9_973):
        seq[at:at + 60] = b"CAG" * 20
    seq = bytes(seq)
    seqs = [seq, _random(900, 14)]
    g = ctx.load(seqs, 50)
    cap = 100_000
    buf = torch.empty((cap + 1, 3), dtype=torch.int64, device="cuda")
    try:
        g.select([(0, tile, 3 * tile)])
        ctx.set_row_sink(buf.data_ptr(), cap)
        before, _ = g.scan(1, 50, 3, 9)
        sink_before = buf.cpu().numpy().copy()
        runs_before = g.dotpair_runs((0, 900, 1_300), (1, 0, None), "-", "both", 3)
        chains_before = g.dotpair_chains((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2)
        links = g.dotpair_links((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2, 4)             # whatever is selected
        _same(links, L.links(seq, seqs[1], "-", 3, 2, 4, (900, 1_300), (0, None)))
        assert len(links) > 100
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.dotpair_runs((0, 900, 1_300), (1, 0, None), "-", "both", 3), runs_before)
        assert np.array_equal(g.dotpair_chains((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2), chains_before)
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_the_groups_of_two_intervals(ctx, tmp_path):
    import plot_dot_plot as cli
    import prf_native
    u = _random(240, 41)
    v = u[:80] + b"C" + u[80:160] + u[162:]                                   # one base inserted, two removed
    n = len(v)
    # A in front of and behind the copy on both sides: A is not its own complement, chance lengthens neither end
    chrom = (_random(2_999, 14) + b"A" + u + b"A" + _random(5_199, 15)).decode()
    other = (_random(399, 16) + b"A" + P.revcomp(v) + b"A" + _random(249, 17)).decode()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    tsv = tmp_path / "groups.tsv"
    base = ["-R", str(fa), "chrT:100-8000", "--versus", "other:300-700", "--strand", "both", "--groups-tsv", str(tsv), "--min-seed", "20",
            "--max-gap", "2", "-d", str(tmp_path)]
    cli.main(base + ["--max-shift", "2", "--min-group", "100"], context=ctx)     # 7 900 positions: no --block needed without an image
    sa, sb = chrom[100:8000], other[300:700]
    groups = prf_native.join_chains(_as(prf_native.DOTCHAIN_DTYPE, C.chains(sa, sb, "-", 20, 2)), _as(prf_native.DOTLINK_DTYPE, L.links(sa, sb, "-", 20, 2, 2)),
                                    len(sb))
    groups = groups[np.maximum(groups["span_a"], groups["span_b"]) >= 100]
    assert len(groups) == 1 and (int(groups["chains"][0]), int(groups["indel"][0]), int(groups["dir"][0])) == (3, 3, R.ANTI)
    matches = int(groups["matches"][0])
    assert 236 <= matches <= 240
    assert tsv.read_text() == f"chrT\t3000\t3240\tother\t400\t{400 + n}\t-\tanti\t240\t{n}\t{matches}\t3\t3\t3\t0\t0\t{matches / 240:.4f}\n"
    assert tsv.read_text() == "".join(cli.group_lines("chrT", 100, "other", 300, "-", groups))
    assert not list(tmp_path.glob("*.png"))
    cli.main(base + ["--max-shift", "1", "--min-group", "100"], context=ctx)     # the deletion of two is out of reach
    assert [line.split("\t")[11] for line in tsv.read_text().splitlines()] == ["2"]
    cli.main(base + ["--max-shift", "2", "--min-group", "100", "--min-identity", "0.999"], context=ctx)
    assert tsv.read_text() == ""
