"""GPU (-m gpu): scans, hand-offs and every product on contigs that hold global position 2^31, global position 2^32, or lie wholly
beyond 2^32 (tests/far_cases.py; tests/test_far_positions_cpu.py proves the inputs without a GPU).  Every comparison is exact.

Two far genomes of five contigs, each built once: A generated on the device (three planes, the plain fused path), B loaded (its
fillers one shared buffer of N, its small contigs crafted, eight planes, fused and generic tiles).  The same three small contigs
alone are the near genomes.  A scan of the far genome must give the oracle's rows of the small contigs and -- restricted to them --
the near genome's rows; a hand-off must decode to the fetched rows; a product of a range must equal its CPU model and be the same
bytes as on the near genome.

What runs where (each on a range across 2^31, on one across 2^32 and wholly beyond 2^32):
  fused and generic scan       test_whole_scan_of_the_generated_genome (A: contigs 1, 3, 4 against the oracle, the fillers' ends just
                               below the boundaries), test_scan_of_the_loaded_genome_splits_into_fused_and_generic_tiles (B)
  selection, shares            test_the_small_contigs_selected_are_the_near_genome, test_shares_of_the_whole_genome_concatenate
  the four hand-offs           test_hand_offs_of_the_selected_scan (24-byte rows with the count record, the wire rows synchronous and
                               pipelined, the row sink on both paths: rows of contigs 1, 3 and 4, tile fields on both sides of 2^15 and 2^16)
  literal lane                 test_literal_lane_on_the_loaded_genome
  the ten products             test_product_equals_its_model_and_the_near_genome[<genome> <kind> <2^31 | 2^32 | beyond> ...]:
                               period = period_bits, period_counts; dotplot = dotplot_bits, dotplot_counts; period_chains;
                               dotpair = dotpair_bits, dotpair_counts, dotpair_runs; dotpair_chains; dotpair_links (its (3, 2) cases
                               run dotpair_chains too)
Every kind runs at every place with a begin on a word of the planes and with one 37 bits into a word (far_cases._cases).
Where the inputs bend what one would wish: of the crafted items only the tandem repeat can hold the boundary itself (period 7 in
contig 1, period 33 in contig 3), inside the enclosing copy; the N block, U and the single R lie within 2 300 positions of it, in
every range that straddles it.  period_bits and period_counts take periods up to the genome's kmax_hint (64 and 50
here), so the k-slice boundary at 2 100 lines is crossed by period_chains, which takes any period; a letter outside ACGTN sends
its tile and both neighbours to the generic kernels, so in B the tiles at the boundaries are generic ones and the fused kernel
runs there in A; the literal lane (motifs up to 8) has rows on both sides of 2^32 and across 2^31 only; at 12 cells a seed is no
chance, so the (12, 8) chains and links run on the strand that holds the copy and the other strand runs at (3, 2).

Measured on an MI355X (pytest --durations=0, three runs): genome A with its whole scan fetched (4.3 G positions, 7.6 M rows) is
set up in 0.32 to 1.10 s, genome B with its near twin (one 2.1 GB host buffer of N, 4.3 GB copied) in 0.39 to 0.73 s, torn down in
1.0 s; the slowest test is the whole scan of A with its forced generic twin and three oracle runs, 1.82 to 2.28 s; a pair-product
case takes about 1 s, nearly all of it the CPU model; the module's 96 tests take 32 s."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import far_cases as F

pytestmark = pytest.mark.gpu

T, EDGE = F.T, F.EDGE
SMALL = [(c, 0, n) for c, n in zip(F.FAR_OF, F.SMALL_LENS)]        # the selection of the three small contigs of a far genome


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    assert prf_native.tile_positions() == T
    c = prf_native.Context(0)
    yield c
    c.close()


def _bases_are(g, lens, hint):
    """A change of the layout rule fails here instead of moving the contigs off the boundaries."""
    assert g.contig_bases().tolist() == F.expected_bases(lens, hint)


@pytest.fixture(scope="module")
def far_a(ctx):
    g = ctx.standin(F.FAR_LENS, F.A_SEEDS, F.HINT_A)
    try:
        _bases_are(g, F.FAR_LENS, F.HINT_A)
        yield g
    finally:
        g.free()


@pytest.fixture(scope="module")
def near_a(ctx):
    g = ctx.standin(list(F.SMALL_LENS), [F.A_SEEDS[c] for c in F.FAR_OF], F.HINT_A)
    try:
        _bases_are(g, F.SMALL_LENS, F.HINT_A)
        yield g
    finally:
        g.free()


@pytest.fixture(scope="module")
def far_b(ctx):
    c1, c3, c4 = F.b_contigs()
    filler = np.full(max(F.FAR_LENS[0], F.FAR_LENS[2]), ord("N"), dtype=np.uint8)      # one buffer, passed twice
    g = ctx.load([(filler.ctypes.data, F.FAR_LENS[0]), c1, (filler.ctypes.data, F.FAR_LENS[2]), c3, c4], F.HINT_B)
    del filler                                                                          # (the load has returned: the bytes are packed)
    try:
        _bases_are(g, F.FAR_LENS, F.HINT_B)
        yield g
    finally:
        g.free()


@pytest.fixture(scope="module")
def near_b(ctx):
    g = ctx.load(list(F.b_contigs()), F.HINT_B)
    try:
        _bases_are(g, F.SMALL_LENS, F.HINT_B)
        yield g
    finally:
        g.free()


@pytest.fixture(scope="module")
def whole_a(far_a):
    """The rows of the whole scan of genome A, fetched once and left unchanged."""
    rows, st = far_a.scan(*F.SCAN)
    assert st.path == 1 and st.sorted_on_device == 1 and st.positions == sum(F.FAR_LENS) and int(st.n_hits) == len(rows)
    rows.setflags(write=False)
    return rows


def _strictly_sorted(rows):
    c, s, e, k = (rows[f].astype(np.int64) for f in ("contig", "start", "end", "k"))
    up = lambda x: x[1:] > x[:-1]              # noqa: E731
    eq = lambda x: x[1:] == x[:-1]             # noqa: E731
    return bool((up(c) | (eq(c) & (up(s) | (eq(s) & (up(e) | (eq(e) & up(k))))))).all())


def _as_far(near_rows):
    """Rows of a near genome with the contig numbers of the far one."""
    out = np.array(near_rows, dtype=near_rows.dtype)
    out["contig"] = np.asarray(F.FAR_OF, dtype=np.uint32)[near_rows["contig"]]
    return out


def _by_position(rows):
    import multi_gpu
    rows = np.asarray(rows, dtype=multi_gpu.ROW_DTYPE)
    return rows[np.lexsort((rows["k"], rows["end"], rows["start"], rows["contig"]))]


# ---- scans on A ----

def test_whole_scan_of_the_generated_genome(far_a, whole_a):
    import prf_native
    from oracle import prf_oracle
    rows = whole_a
    contig = rows["contig"].astype(np.int64)
    assert bool((contig[1:] >= contig[:-1]).all()) and set(np.unique(contig).tolist()) == {0, 1, 2, 3, 4}
    assert _strictly_sorted(rows)
    small = rows[np.isin(rows["contig"], F.FAR_OF)]
    want = _as_far(F.oracle_rows(F.a_contigs(), F.SCAN))
    assert len(want) > 600 and all(int((want["contig"] == c).sum()) > 50 for c in F.FAR_OF)
    assert np.array_equal(small, want)
    for c in (1, 3):                                                  # rows on both sides of the boundary
        mine = want[want["contig"] == c]
        assert (mine["end"] < EDGE).any() and (mine["start"] > EDGE).any()
    # the fillers, just below 2^31 and 2^32: the oracle on a window at the contig's end
    win, margin = 400_000, 1_000
    starts, ends, ks = (rows[f].astype(np.int64) for f in ("start", "end", "k"))
    for c in (0, 2):
        n = F.FAR_LENS[c]
        off = n - win
        chunk = F.a_window(c, off, win)
        want = [(s + off, e + off, k) for s, e, _m, k in prf_oracle.detect_rows(chunk, *F.SCAN) if s >= margin]
        sel = (contig == c) & (starts >= off + margin)
        assert list(zip(starts[sel].tolist(), ends[sel].tolist(), ks[sel].tolist())) == want and len(want) > 100, c
        assert F.FAR_BASES[c] + off > F.FAR_BASES[c + 1] - 2 * win
    generic, st = far_a.scan(*F.SCAN, flags=prf_native.SCAN_FORCE_GENERIC)
    assert st.path == 0 and np.array_equal(generic, rows)


def test_the_small_contigs_selected_are_the_near_genome(far_a, near_a):
    near, st_near = near_a.scan(*F.SCAN)
    assert st_near.path == 1 and st_near.positions == 470_001 == sum(F.SMALL_LENS)
    far_a.select(SMALL)
    try:
        rows, st = far_a.scan(*F.SCAN)
        assert st.path == 1 and st.sorted_on_device == 1 and st.positions == 470_001
        assert np.array_equal(rows, _as_far(near)) and len(rows) > 600
    finally:
        far_a.select(None)


@pytest.mark.parametrize("world", [2, 5])
def test_shares_of_the_whole_genome_concatenate(far_a, whole_a, world):
    import multi_gpu
    shares = multi_gpu.plan_parts(F.FAR_LENS, world, T, [far_a.tile_classes(c) for c in range(5)])
    assert len(shares) == world and all(shares)
    got, covered = [], 0
    try:
        for parts in shares:
            far_a.select(parts)
            rows, st = far_a.scan(*F.SCAN)
            assert st.path == 1 and st.positions == sum(e - b for _c, b, e in parts)
            covered += st.positions
            got.append(rows)
    finally:
        far_a.select(None)
    assert covered == sum(F.FAR_LENS)
    # cuts inside a contig, and (world 5) a share that begins beyond 2^31
    firsts = [F.FAR_BASES[parts[0][0]] + parts[0][1] for parts in shares]
    assert any(parts[0][1] > 0 for parts in shares) and (world < 5 or max(firsts) >= 2 ** 31)
    assert np.array_equal(np.concatenate(got), whole_a)


def _check_words(words, want, cap, side, g):
    """Device words decode to the rows and are the host encoder's words."""
    import multi_gpu
    bases = g.contig_bases()
    assert np.array_equal(multi_gpu.unpack_rows(words, cap, side, bases, T), want)
    assert np.array_equal(words, multi_gpu.pack_rows(want, cap, side, bases, T))
    tiles = words[:len(want)] >> np.uint64(41)
    # tile fields below 2^15 (in front of 2^31), from 2^15 on, and from 2^16 on (beyond 2^32)
    assert int(tiles.min()) < 2 ** 15 and bool(((tiles >= 2 ** 15) & (tiles < 2 ** 16)).any()) and int(tiles.max()) >= 2 ** 16


def test_hand_offs_of_the_selected_scan(ctx, far_a):
    import multi_gpu
    import prf_native
    far_a.select(SMALL)
    try:
        rows, st = far_a.scan(*F.SCAN)
        n = len(rows)
        assert st.sorted_on_device == 1 and n > 600 and (rows["contig"] == 4).sum() > 50
        assert int((rows["end"] - rows["start"]).max()) < 65_535                      # no long rows: the side list stays empty
        cap, side = n + 7, 1
        # the 24-byte rows with the count record
        buf = torch.full((cap + 1, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.last_hits_to_device(buf.data_ptr(), cap, count_row=True) == n
        host = buf.cpu().numpy()
        assert host[cap].tolist() == [n, 0, 0] and (host[n:cap] == -1).all()
        assert np.array_equal(np.ascontiguousarray(host[:n]).view(rows.dtype).reshape(-1), rows)
        # the 8-byte wire rows of the same scan
        words_buf = torch.zeros(cap + 1 + 3 * side, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert ctx.last_hits_packed_to_device(far_a, words_buf.data_ptr(), cap, side) == n
        torch.cuda.synchronize()
        _check_words(words_buf.cpu().numpy().view(np.uint64), rows, cap, side, far_a)
        # the pipelined packed scan
        words_buf.zero_()
        torch.cuda.synchronize()
        seq = far_a.scan_async_packed(*F.SCAN, words_buf.data_ptr(), cap, side)
        sta = ctx.scan_wait(seq)
        torch.cuda.synchronize()
        assert int(sta.n_hits) == n and sta.sorted_on_device == 1 and sta.positions == 470_001
        words = words_buf.cpu().numpy().view(np.uint64)
        _check_words(words, rows, cap, side, far_a)
        decoded = multi_gpu.unpack_rows(words, cap, side, far_a.contig_bases(), T)
        assert (decoded["contig"] == 4).any() and (decoded["contig"] == 3).any() and (decoded["contig"] == 1).any()
        # the row sink, on both kernel paths
        for flags in (prf_native.SCAN_DEFAULT, prf_native.SCAN_FORCE_GENERIC):
            buf.fill_(-1)
            torch.cuda.synchronize()
            ctx.set_row_sink(buf.data_ptr(), cap)
            try:
                again, st2 = far_a.scan(*F.SCAN, flags=flags)
            finally:
                ctx.set_row_sink(None, 0)
            assert st2.path == (1 if flags == prf_native.SCAN_DEFAULT else 0) and np.array_equal(again, rows)
            host = buf.cpu().numpy()
            assert host[cap].tolist() == [n, 0, 0] and (host[n:cap] == -1).all()
            assert np.array_equal(_by_position(np.ascontiguousarray(host[:n]).view(rows.dtype).reshape(-1)), rows)
    finally:
        ctx.set_row_sink(None, 0)
        far_a.select(None)


# ---- scans on B ----

def _b_rows(settings):
    return _as_far(F.oracle_rows(F.b_contigs(), settings))


def test_scan_of_the_loaded_genome_splits_into_fused_and_generic_tiles(far_b, near_b):
    import prf_native
    want = _b_rows(F.SCAN)
    assert all(int((want["contig"] == c).sum()) >= 20 for c in F.FAR_OF)
    assert any(int(r["start"]) < EDGE < int(r["end"]) for r in want[want["contig"] == 1])          # the period-7 repeat across 2^31
    rows, st = far_b.scan(*F.SCAN)
    assert st.path == 1 and st.sorted_on_device == 0 and st.positions == sum(F.FAR_LENS)
    assert np.array_equal(rows, want)
    generic, stg = far_b.scan(*F.SCAN, flags=prf_native.SCAN_FORCE_GENERIC)
    assert stg.path == 0 and np.array_equal(generic, want)
    for c in (0, 2):
        assert (far_b.tile_classes(c) == 2).all() and len(far_b.tile_classes(c)) == -(-F.FAR_LENS[c] // T)
    small = np.concatenate([far_b.tile_classes(c) for c in F.FAR_OF])
    assert all(3 in far_b.tile_classes(c) for c in F.FAR_OF) and bool((small < 2).any())           # generic tiles and fused ones
    assert far_b.tile_classes(1)[3] < 2 and far_b.tile_classes(3)[0] < 2                           # (two tiles away from such a letter)
    assert far_b.tile_classes(1)[EDGE // T] == 3 or far_b.tile_classes(1)[EDGE // T - 1] == 3     # a generic tile next to 2^31
    near, stn = near_b.scan(*F.SCAN)
    assert stn.path == 1 and np.array_equal(_as_far(near), want)


def test_literal_lane_on_the_loaded_genome(far_b):
    want = _b_rows(F.LITERAL)
    assert len(want) > 30_000 and set(np.unique(want["contig"]).tolist()) == set(F.FAR_OF)
    rows, st = far_b.scan(*F.LITERAL)
    assert st.path == 2 and int(st.n_hits) == len(want)
    assert not np.isin(rows["contig"], (0, 2)).any()                                              # nothing but N: no rows
    assert np.array_equal(_by_position(rows), _by_position(want))
    for c in (1, 3):                                                                              # rows up to, behind and (2^31) across the boundary
        mine = rows[rows["contig"] == c]
        assert (mine["end"] <= EDGE).any() and (mine["start"] >= EDGE).any()
        assert c == 3 or ((mine["start"] < EDGE) & (mine["end"] > EDGE)).any()


# ---- products: B with eight planes, A with three ----

@pytest.mark.parametrize("case", F.CASES, ids=[c.name for c in F.CASES])
def test_product_equals_its_model_and_the_near_genome(case, request):
    genome = case.genome.lower()
    far, near = request.getfixturevalue(f"far_{genome}"), request.getfixturevalue(f"near_{genome}")
    seqs = F.near_contigs(case.genome)
    want = F.models(case)                                              # (asserts the floors of the case on the way)
    got_far, got_near = F.calls(far, case, True, seqs), F.calls(near, case, False, seqs)
    assert [label for label, _ in got_far] == [label for label, _ in want] == [label for label, _ in got_near]
    for (label, x), (_, y), (_, z) in zip(got_far, got_near, want):
        assert F.same(x, z), (case.name, label, "far genome against the model")
        # (a list's rows carry padding that numpy leaves unset: its fields are compared, a matrix byte by byte)
        assert x.dtype == y.dtype and x.shape == y.shape, (case.name, label)
        assert F.same(x, y) if x.dtype.names else x.tobytes() == y.tobytes(), (case.name, label, "far genome against the near one")
    if case.opt.get("self"):                                           # a range against itself is the self plot
        by_label = dict(got_far)
        assert np.array_equal(by_label["bits t=3"], by_label["the self plot t=3"])


def test_a_scan_after_the_products_returns_the_same_rows(far_b):
    """The products share the context's stream and scratch memory with the scans: run last, after every product call."""
    c, a = F.CASES[0], [c for c in F.CASES if c.genome == "B" and c.kind == "links"][0]
    seqs = F.b_contigs()
    F.calls(far_b, c, True, seqs), F.calls(far_b, a, True, seqs)
    rows, st = far_b.scan(*F.SCAN)
    assert st.path == 1 and np.array_equal(rows, _b_rows(F.SCAN))
    rows, st = far_b.scan(*F.LITERAL)
    assert st.path == 2 and np.array_equal(_by_position(rows), _by_position(_b_rows(F.LITERAL)))
