"""GPU (-m gpu): the data path of a multi-GPU step at its edges -- prf_genome_select, one synchronous scan that sizes the buffers,
prf_scan_genome_async_packed twice in flight, prf_stream_wait_for, multi_gpu.unpack_rows -- which bench.py runs at N > 1.

A  shares of one genome through the pipelined packed path, empty shares included;
B  spans on either side of the wire row's span field, a side list that is exactly full and one that is too small;
C  rows at tile offsets 65 535 and 0 behind a non-zero contig base, and the widest motif the wire holds;
D  every refusal of the pipelined call leaves both slots free; the rows of a scan collected from the second slot;
E  a pipelined scan that overflows the buffers its sizing scan left (slabs, row array) leaves the all-ones count word;
F  the timing ring wraps, and a scan's two parts add up to its whole.

Every expected row set comes from the oracle (tests/pipelined_edges_cases.py; tests/test_wire_format_cpu.py asserts on the CPU
what the cases are built around)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import pipelined_edges_cases as cases

pytestmark = pytest.mark.gpu

TILE = cases.TILE
POISON = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    assert prf_native.tile_positions() == TILE
    c = prf_native.Context(0)
    yield c
    c.close()


def fresh_buffer(cap, side):
    """Zeroed device words for cap rows, the count word and `side` long rows (the library's stream does not wait for the fill)."""
    buf = torch.zeros(cap + 1 + 3 * side, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return buf


def host_words(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64)


def by_position(rows):
    import multi_gpu
    rows = np.asarray(rows, dtype=multi_gpu.ROW_DTYPE)                 # (a scan without rows returns an empty list)
    return rows[np.lexsort((rows["k"], rows["end"], rows["start"], rows["contig"]))]


def check_scan(got, stats, want):
    """The rows a synchronous scan fetched against the oracle's."""
    assert int(stats.n_hits) == len(want)
    assert np.array_equal(by_position(got), want)


def check_words(words, want, cap, side, g, sorted_on_device=True, equal_words=True):
    """Device words against the oracle's rows: they decode to them and (equal_words) are the host encoder's words, the side list in
    any order, with nothing written beyond the rows and the long rows."""
    import multi_gpu
    bases = g.contig_bases()
    got = multi_gpu.unpack_rows(words, cap, side, bases, TILE)
    assert np.array_equal(got if sorted_on_device else by_position(got), want)
    if not (equal_words and sorted_on_device):
        return
    ref = multi_gpu.pack_rows(want, cap, side, bases, TILE)
    assert np.array_equal(words[:cap + 1], ref[:cap + 1])
    assert sorted(map(tuple, words[cap + 1:].reshape(-1, 3).tolist())) == sorted(map(tuple, ref[cap + 1:].reshape(-1, 3).tolist()))


def n_side_of(words, cap):
    return int(words[cap]) >> 40


def code_of(call, *args):
    """The status code a refused call gives."""
    import prf_native
    with pytest.raises(prf_native.PrfError) as info:
        call(*args)
    return info.value.code


def slots_are_free(ctx, g, settings, n_rows):
    """Two pipelined scans of a genome whose buffers are sized: a slot left taken would refuse one of them."""
    seqs = []
    try:
        seqs.append(g.scan_async(*settings))
        seqs.append(g.scan_async(*settings))
    finally:
        stats = [ctx.scan_wait(s) for s in seqs]
    assert [int(st.n_hits) for st in stats] == [n_rows] * 2
    return stats


def packed_pair(ctx, g, settings, cap, side):
    """What a multi-GPU step does: two packed scans in flight, each buffer handed to a stream of the caller's.  Returns the two
    buffers' words and the scans' stats."""
    bufs = [fresh_buffer(cap, side) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    seqs, stats = [], []
    try:
        for buf, stream in zip(bufs, streams):
            seqs.append(g.scan_async_packed(*settings, buf.data_ptr(), cap, side))
            ctx.stream_wait_for(stream.cuda_stream)
    finally:
        stats = [ctx.scan_wait(s) for s in seqs]
    for stream in streams:
        stream.synchronize()                      # the hand-off: what the stream has waited for holds the words
    return [host_words(b) for b in bufs], stats


def packed_once(ctx, g, settings, cap, side, wait_fails_with=None):
    """One packed scan, collected.  wait_fails_with: prf_scan_wait must fail with PRF_EUNSUPPORTED and this word in its message."""
    import prf_native
    buf = fresh_buffer(cap, side)
    seq = g.scan_async_packed(*settings, buf.data_ptr(), cap, side)
    if wait_fails_with is None:
        stats = ctx.scan_wait(seq)
    else:
        with pytest.raises(prf_native.PrfError) as info:
            ctx.scan_wait(seq)
        assert info.value.code == prf_native.PRF_EUNSUPPORTED and wait_fails_with in info.value.message, info.value.message
        stats = None
    return host_words(buf), stats


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 13])
def test_shares_through_the_pipelined_packed_path(ctx, world):
    import multi_gpu
    import prf_native
    seqs, whole = cases.share_genome()
    lens, settings, side = cases.SHARE_LENS, cases.SHARE_SETTINGS, 2
    g = ctx.load(list(seqs), cases.SHARE_HINT)
    try:
        rows, st = g.scan(*settings)                                    # (sizes the buffers for the whole genome)
        check_scan(rows, st, whole)
        classes = [g.tile_classes(c) for c in range(len(lens))]
        shares = multi_gpu.plan_parts(lens, world, TILE, classes)
        assert len(shares) == world and (world != 13 or any(not parts for parts in shares))
        got, covered, with_long = [], 0, 0
        for parts in shares:
            want = cases.rows_of_parts(whole, parts)
            positions = sum(e - b for _c, b, e in parts)
            # (Genome.select([]) means the whole genome: a share without tiles is a part without positions)
            g.select(parts if parts else [(0, 0, 0)])
            rows, st = g.scan(*settings)
            assert st.positions == positions and st.path == 1
            check_scan(rows, st, want)
            if not parts:
                assert len(want) == 0
                assert code_of(g.scan_async, *settings) == prf_native.PRF_EUNSUPPORTED                # nothing to launch
                buf = fresh_buffer(4, side)
                assert code_of(g.scan_async_packed, *settings, buf.data_ptr(), 4, side) == prf_native.PRF_EUNSUPPORTED
                assert not host_words(buf).any()
                g.select(None)
                slots_are_free(ctx, g, settings, len(whole))                                            # no slot was taken
                continue
            cap = len(want) + 5
            (w0, w1), stats = packed_pair(ctx, g, settings, cap, side)
            for words, sta in zip((w0, w1), stats):
                assert int(sta.n_hits) == len(want) and sta.positions == positions
                check_words(words, want, cap, side, g, sorted_on_device=bool(sta.sorted_on_device))
            decoded = by_position(multi_gpu.unpack_rows(w1, cap, side, g.contig_bases(), TILE))
            assert all(any(c == int(r["contig"]) and b <= int(r["start"]) < e for c, b, e in parts) for r in decoded)
            with_long += n_side_of(w0, cap)
            assert n_side_of(w0, cap) == n_side_of(w1, cap) == int(np.count_nonzero(want["end"] - want["start"] >= 65_535))
            covered += positions
            got.append(decoded)
        assert covered == sum(lens) and with_long == 1                 # exactly one share carries the long row in its side list
        assert np.array_equal(np.concatenate(got), whole)              # the shares are in genome order: the concatenation is sorted
        g.select(None)
        rows, st = g.scan(*settings)
        assert st.positions == sum(lens)
        check_scan(rows, st, whole)
    finally:
        g.free()


# ---- B ------------------------------------------------------------------------------------------------------------------------
def test_spans_on_either_side_of_the_span_field(ctx):
    import multi_gpu
    import prf_native
    seqs, want = cases.span_genome()
    settings = cases.SPAN_SETTINGS
    n = len(want)
    assert n == 4
    g = ctx.load(list(seqs), 3)
    try:
        rows, st = g.scan(*settings)
        check_scan(rows, st, want)
        bases = g.contig_bases()
        for cap in (n + 3, n):                                          # (a buffer that is exactly full decodes too)
            # the synchronous hand-off, the side list exactly full
            buf = fresh_buffer(cap, 2)
            assert ctx.last_hits_packed_to_device(g, buf.data_ptr(), cap, 2) == n
            words = host_words(buf)
            check_words(words, want, cap, 2, g)
            assert n_side_of(words, cap) == 2                           # spans 65 535 and 65 536; 65 534 stays in the word
            assert ((words[:n] >> np.uint64(9)) & np.uint64(0xFFFF)).tolist() == [65_533, 65_534, 65_535, 65_535]
            # the pipelined one
            words, sta = packed_once(ctx, g, settings, cap, 2)
            assert int(sta.n_hits) == n
            check_words(words, want, cap, 2, g)
            assert n_side_of(words, cap) == 2
        cap = n + 3
        # a side list that is too small: refused synchronously, poisoned behind a pipelined scan
        buf = fresh_buffer(cap, 1)
        assert code_of(ctx.last_hits_packed_to_device, g, buf.data_ptr(), cap, 1) == prf_native.PRF_EINVAL
        words, sta = packed_once(ctx, g, settings, cap, 1)
        assert int(sta.n_hits) == n and int(words[cap]) == POISON
        with pytest.raises(ValueError):
            multi_gpu.unpack_rows(words, cap, 1, bases, TILE)
        # the pack that follows a poisoned one starts with an empty side list
        words, sta = packed_once(ctx, g, settings, cap, 2)
        check_words(words, want, cap, 2, g)
        assert n_side_of(words, cap) == 2
        # one row too few in the buffer
        words, sta = packed_once(ctx, g, settings, n - 1, 2)
        assert int(sta.n_hits) == n and int(words[n - 1]) == POISON
        with pytest.raises(ValueError):
            multi_gpu.unpack_rows(words, n - 1, 2, bases, TILE)
        buf = fresh_buffer(n - 1, 2)
        assert code_of(ctx.last_hits_packed_to_device, g, buf.data_ptr(), n - 1, 2) == prf_native.PRF_EINVAL
        words, sta = packed_once(ctx, g, settings, cap, 2)
        check_words(words, want, cap, 2, g)
    finally:
        g.free()


# ---- C ------------------------------------------------------------------------------------------------------------------------
def test_rows_at_the_ends_of_the_position_field(ctx):
    seqs, want = cases.field_genome()
    settings, side = cases.FIELD_SETTINGS, 1
    g = ctx.load(list(seqs), 50)
    try:
        bases = g.contig_bases()
        assert all(int(b) % TILE == 0 for b in bases) and int(bases[1]) > 0
        rows, st = g.scan(*settings)
        check_scan(rows, st, want)
        cap = len(want) + 2
        buf = fresh_buffer(cap, side)
        assert ctx.last_hits_packed_to_device(g, buf.data_ptr(), cap, side) == len(want)
        words = host_words(buf)
        check_words(words, want, cap, side, g, sorted_on_device=bool(st.sorted_on_device))
        for c, at in cases.FIELD_PLANTS:                                 # the planted rows' words, field by field
            gpos = int(bases[c]) + at
            word = (gpos // TILE << 41) | (gpos % TILE << 25) | (24 << 9) | 3
            assert word in words[:len(want)].tolist(), (c, at)
        assert {(int(bases[c]) + at) % TILE for c, at in cases.FIELD_PLANTS} >= {0, 65_535}
        (w0, w1), stats = packed_pair(ctx, g, settings, cap, side)
        for w, sta in zip((w0, w1), stats):
            check_words(w, want, cap, side, g, sorted_on_device=bool(sta.sorted_on_device))
    finally:
        g.free()


def test_the_widest_motif_the_wire_holds(ctx):
    import multi_gpu
    import prf_native
    wide = cases.wide_motif(511)
    want = cases.oracle_rows([wide], (505, 511, 2, 9))
    assert 511 in want["k"].tolist()
    g = ctx.load([wide], 511)
    try:
        rows, st = g.scan(505, 511, 2, 9)
        assert st.path == 0                                              # the generic path
        check_scan(rows, st, want)
        cap = len(want) + 1
        buf = fresh_buffer(cap, 1)
        assert ctx.last_hits_packed_to_device(g, buf.data_ptr(), cap, 1) == len(want)
        words = host_words(buf)
        check_words(words, want, cap, 1, g, sorted_on_device=False)      # (the generic path leaves its rows unsorted on the device)
        ref = multi_gpu.pack_rows(want, cap, 1, g.contig_bases(), TILE)
        assert sorted(words[:len(want)].tolist()) == sorted(ref[:len(want)].tolist()) and np.array_equal(words[len(want):], ref[len(want):])
        assert 511 in (words[:len(want)] & np.uint64(511)).tolist()
    finally:
        g.free()
    wider = cases.wide_motif(512)
    want = cases.oracle_rows([wider], (505, 512, 2, 9))
    small = ctx.load([b"ACGT" * 10 + b"A" * 30 + b"C"], 50)
    g = ctx.load([wider], 512)
    try:
        rows, st = g.scan(505, 512, 2, 9)
        check_scan(rows, st, want)
        buf = fresh_buffer(len(want) + 1, 1)
        assert code_of(ctx.last_hits_packed_to_device, g, buf.data_ptr(), len(want) + 1, 1) == prf_native.PRF_EUNSUPPORTED
        assert code_of(g.scan_async_packed, 505, 512, 2, 9, buf.data_ptr(), len(want) + 1, 1) == prf_native.PRF_EUNSUPPORTED
        assert not host_words(buf).any()
        rows, st = small.scan(1, 50, 3, 9)
        check_scan(rows, st, cases.oracle_rows([b"ACGT" * 10 + b"A" * 30 + b"C"], (1, 50, 3, 9)))
        slots_are_free(ctx, small, (1, 50, 3, 9), len(rows))             # no slot was taken
    finally:
        g.free()
        small.free()


# ---- D ------------------------------------------------------------------------------------------------------------------------
REFUSAL_SEQ = b"ACGT" * 10 + b"A" * 300 + b"C" + b"GT" * 200 + b"ACGTTGCA" + b"CAG" * 50 + b"T"
REFUSAL_OTHER = b"TTGACCA" + b"AC" * 100 + b"GGT" + b"ACG" * 40 + b"T" + b"C" * 20 + b"A"
REFUSAL_SETTINGS = (1, 50, 3, 9)


def test_refusals_of_the_pipelined_call_leave_the_slots_free():
    import prf_native
    settings = REFUSAL_SETTINGS
    want = cases.oracle_rows([REFUSAL_SEQ], settings)
    assert len(want) >= 3
    c, other = prf_native.Context(0), prf_native.Context(0)
    g = foreign = iupac = None
    try:
        g = c.load([REFUSAL_SEQ], 50)
        foreign = other.load([REFUSAL_SEQ], 50)
        iupac = c.load([REFUSAL_SEQ + b"R" + REFUSAL_SEQ], 50)
        buf = fresh_buffer(len(want) + 1, 2)
        packed = (buf.data_ptr(), len(want) + 1, 2)

        def free():
            slots_are_free(c, g, settings, len(want))
            assert not host_words(buf).any()                                          # and no refused call wrote words

        # the context was never sized
        assert code_of(g.scan_async, *settings) == prf_native.PRF_EUNSUPPORTED
        assert code_of(g.scan_async_packed, *settings, *packed) == prf_native.PRF_EUNSUPPORTED
        rows, st = g.scan(*settings)
        check_scan(rows, st, want)
        free()
        # a row sink is set
        sink = torch.zeros((len(want) + 1, 3), dtype=torch.int64, device="cuda")
        c.set_row_sink(sink.data_ptr(), len(want))
        try:
            assert code_of(g.scan_async, *settings) == prf_native.PRF_EUNSUPPORTED
            assert code_of(g.scan_async_packed, *settings, *packed) == prf_native.PRF_EUNSUPPORTED
        finally:
            c.set_row_sink(None, 0)
        free()
        # min_repeats is 1 (the literal lane serves it)
        assert code_of(g.scan_async, 1, 50, 1, 9) == prf_native.PRF_EUNSUPPORTED
        assert code_of(g.scan_async_packed, 1, 50, 1, 9, *packed) == prf_native.PRF_EUNSUPPORTED
        free()
        # max_motif_size above the hint the genome was packed with, and above what the wire holds
        assert code_of(g.scan_async, 1, 51, 3, 9) == prf_native.PRF_EUNSUPPORTED
        assert code_of(g.scan_async_packed, 1, 51, 3, 9, *packed) == prf_native.PRF_EUNSUPPORTED
        assert code_of(g.scan_async_packed, 1, 512, 3, 9, *packed) == prf_native.PRF_EUNSUPPORTED
        free()
        # the genome belongs to another context
        import ctypes
        seq = ctypes.c_uint64(0)
        with pytest.raises(prf_native.PrfError) as info:
            prf_native._check(c.lib, c.lib.prf_scan_genome_async(c._h, foreign._h, *settings, ctypes.byref(seq)))
        assert info.value.code == prf_native.PRF_EINVAL and seq.value == 0
        with pytest.raises(prf_native.PrfError) as info:
            prf_native._check(c.lib, c.lib.prf_scan_genome_async_packed(c._h, foreign._h, *settings, ctypes.c_void_p(packed[0]), packed[1],
                                                                        packed[2], ctypes.byref(seq)))
        assert info.value.code == prf_native.PRF_EINVAL and seq.value == 0
        free()
        # the selection is empty
        g.select([(0, 0, 0)])
        try:
            assert code_of(g.scan_async, *settings) == prf_native.PRF_EUNSUPPORTED
            assert code_of(g.scan_async_packed, *settings, *packed) == prf_native.PRF_EUNSUPPORTED
        finally:
            g.select(None)
        free()
        # a letter outside ACGTN: a second pass follows the fused scan
        rows, st = iupac.scan(*settings)
        check_scan(rows, st, cases.oracle_rows([REFUSAL_SEQ + b"R" + REFUSAL_SEQ], settings))
        assert code_of(iupac.scan_async, *settings) == prf_native.PRF_EUNSUPPORTED
        assert code_of(iupac.scan_async_packed, *settings, *packed) == prf_native.PRF_EUNSUPPORTED
        free()
        # prf_scan_wait: a serial number that is not in flight, and the same one twice
        stats = slots_are_free(c, g, settings, len(want))
        assert code_of(c.scan_wait, stats[1].seq + 1000) == prf_native.PRF_EINVAL
        assert code_of(c.scan_wait, stats[1].seq) == prf_native.PRF_EINVAL
        assert code_of(c.scan_wait, stats[0].seq) == prf_native.PRF_EINVAL
        sq = g.scan_async(*settings)
        try:
            assert code_of(c.scan_wait, sq + 1) == prf_native.PRF_EINVAL              # (one in flight: still not this one)
        finally:
            assert int(c.scan_wait(sq).n_hits) == len(want)
        assert code_of(c.scan_wait, sq) == prf_native.PRF_EINVAL
        free()
        rows, st = g.scan(*settings)
        check_scan(rows, st, want)
    finally:
        for x in (g, foreign, iupac):
            if x is not None:
                x.free()
        c.close()
        other.close()


def test_rows_of_a_scan_collected_from_the_second_slot():
    """prf_last_hits_to_device after pipelined scans hands over the rows of the scan collected last, from the slot it ran in.  Two
    genomes with different rows take the slots in turn, two scans in flight: on a fresh context the 1st, 3rd and 5th scan run in the
    first slot, the 2nd and 4th in the second.  The rows are asked for after the 4th (second slot) and after the 5th -- an odd
    count -- (first slot)."""
    import prf_native
    settings = REFUSAL_SETTINGS
    seqs = (REFUSAL_SEQ, REFUSAL_OTHER)
    want = [cases.oracle_rows([s], settings) for s in seqs]
    assert len(want[0]) >= 3 and len(want[1]) >= 3 and len(want[0]) != len(want[1])
    c = prf_native.Context(0)
    gs = []
    try:
        gs = [c.load([s], 50) for s in seqs]
        for g, w in zip(gs, want):
            rows, st = g.scan(*settings)
            check_scan(rows, st, w)
        cap = max(len(w) for w in want) + 3

        def handed_over(n_expected):
            buf = torch.full((cap + 1, 3), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            assert c.last_hits_to_device(buf.data_ptr(), cap, count_row=True) == n_expected
            host = buf.cpu().numpy()
            assert host[cap].tolist() == [n_expected, 0, 0] and (host[n_expected:cap] == -1).all()
            return by_position(np.ascontiguousarray(host[:n_expected]).view(want[0].dtype).reshape(-1))

        pending = []
        try:
            pending.append(gs[0].scan_async(*settings))                             # 1st: first slot
            pending.append(gs[1].scan_async(*settings))                             # 2nd: second slot
            assert int(c.scan_wait(pending.pop(0)).n_hits) == len(want[0])
            pending.append(gs[0].scan_async(*settings))                             # 3rd: first slot
            assert int(c.scan_wait(pending.pop(0)).n_hits) == len(want[1])
            pending.append(gs[1].scan_async(*settings))                             # 4th: second slot
            assert int(c.scan_wait(pending.pop(0)).n_hits) == len(want[0])
            assert int(c.scan_wait(pending.pop(0)).n_hits) == len(want[1])          # collected last: the 4th
            assert np.array_equal(handed_over(len(want[1])), want[1])
            pending.append(gs[0].scan_async(*settings))                             # 5th: first slot
            assert int(c.scan_wait(pending.pop(0)).n_hits) == len(want[0])
            assert np.array_equal(handed_over(len(want[0])), want[0])
        finally:
            for s in pending:
                c.scan_wait(s)
    finally:
        for g in gs:
            g.free()
        c.close()


# ---- E ------------------------------------------------------------------------------------------------------------------------
def overflow_then_recover(c, dense_genome, want, side, names):
    """A packed scan behind a sizing scan of something else: the all-ones word and a wait that names the buffer; then the
    synchronous scan (which grows the buffer) equals the oracle, and a pipelined scan decodes to the same rows."""
    import multi_gpu
    settings = cases.OVF_SETTINGS
    cap = len(want) + 5
    words, _ = packed_once(c, dense_genome, settings, cap, side, wait_fails_with=names)
    assert int(words[cap]) == POISON
    with pytest.raises(ValueError):
        multi_gpu.unpack_rows(words, cap, side, dense_genome.contig_bases(), TILE)
    rows, st = dense_genome.scan(*settings)
    assert st.path == 1
    check_scan(rows, st, want)
    words, sta = packed_once(c, dense_genome, settings, cap, side)
    assert int(sta.n_hits) == len(want) and int(words[cap]) == len(want)
    check_words(words, want, cap, side, dense_genome, sorted_on_device=bool(sta.sorted_on_device))


def test_a_pipelined_scan_that_overflows_the_slabs_poisons_its_words():
    import prf_native
    sizing, dense, want = cases.slab_case()
    c = prf_native.Context(0)
    gs = []
    try:
        gs = [c.load([sizing], 6), c.load([dense], 6)]
        _, st = gs[0].scan(*cases.OVF_SETTINGS, fetch=False)
        assert st.path == 1
        overflow_then_recover(c, gs[1], want, 2, "slabs")
    finally:
        for g in gs:
            g.free()
        c.close()


def test_a_pipelined_scan_that_overflows_the_row_array_poisons_its_words():
    """The row array holds positions / 32 + 65 536 rows, so the case needs more than 65 536 rows at more than one per 32
    positions: 436 906 rows on 10 485 744 positions, against 393 215.  The pack kernel reads none of the rows the array does not
    hold."""
    import prf_native
    slabs, sizing, dense, want = cases.row_array_case()
    c = prf_native.Context(0)
    gs = []
    try:
        gs = [c.load([slabs], 6), c.load([sizing], 6), c.load([dense], 6)]
        _, st = gs[0].scan(*cases.OVF_SETTINGS, fetch=False)                         # the slabs grow to 2 731 rows per tile and more
        assert st.path == 1 and int(st.n_hits) == cases.ROWS_SLAB_N
        _, st = gs[1].scan(*cases.OVF_SETTINGS, fetch=False)                         # the row array: 393 215 rows
        assert st.path == 1 and int(st.n_hits) < 393_215 < len(want)
        overflow_then_recover(c, gs[2], want, 2, "row array")
    finally:
        for g in gs:
            g.free()
        c.close()


# ---- F ------------------------------------------------------------------------------------------------------------------------
# The largest |scan + gather - total| over the 128 scans of the ring, in ms, as measured once on an MI355X (totals of 0.0259 to
# 0.0343 ms): the three times are whole nanoseconds that add up exactly, each handed over as a float -- the figure is one unit in
# the last place of a float at 0.03 ms (2^-29).  The test allows twice that.
SPLIT_SUM_LARGEST_SEEN_MS = 1.862645149230957e-09


def test_the_timing_ring_wraps_and_the_parts_add_up(ctx):
    import prf_native
    import synth
    assert prf_native.TIMING_RING == 128
    g = ctx.load([synth.standin2(70_000, 11).tobytes()], 50)
    try:
        seqs = []
        for _ in range(prf_native.TIMING_RING + 2):
            none, st = g.scan(1, 50, 3, 9, flags=prf_native.SCAN_DEFER_TIMING, fetch=False)
            assert none is None and st.path == 1
            seqs.append(int(st.seq))
        first, last = seqs[0], seqs[-1]
        assert seqs == list(range(first, first + prf_native.TIMING_RING + 2))
        assert code_of(ctx.scan_timings, first, 1) == prf_native.PRF_EINVAL          # its events record a later scan by now
        assert code_of(ctx.scan_timings, first + 1, 1) == prf_native.PRF_EINVAL
        assert code_of(ctx.scan_timings_split, first, 1) == prf_native.PRF_EINVAL
        assert code_of(ctx.scan_timings, last, 2) == prf_native.PRF_EINVAL           # not issued yet
        total = ctx.scan_timings(last - 127, 128)
        assert len(total) == 128 and all(0 < t < 50 for t in total)
        scan, gather = ctx.scan_timings_split(last - 127, 128)
        assert len(scan) == len(gather) == 128 and all(s > 0 and x > 0 for s, x in zip(scan, gather))
        assert ctx.scan_timings(last - 127, 128) == total                            # the events are read, not consumed
        worst = max(abs(s + x - t) for s, x, t in zip(scan, gather, total))
        print(f"largest |scan + gather - total| of 128 scans: {worst!r} ms (totals {min(total)!r} .. {max(total)!r} ms)")
        assert worst <= 2 * SPLIT_SUM_LARGEST_SEEN_MS
    finally:
        g.free()
