"""GPU (-m gpu): two pipelined scans whose rows leave as 8-byte wire words (prf_scan_genome_async_packed), each handed to a
stream of the caller's by an event (prf_stream_wait_for) -- what bench.py does at N > 1: the slots of the two scans in flight,
the pack enqueued behind a running scan, the refusal of a third scan, and the slots free again afterwards.

The input is the two contigs of test_gpu_parity.py whose longest rows do not fit the 16 bits of a wire row's span, so the side
list of long rows is written by both packs."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

pytestmark = pytest.mark.gpu

LONG_RUN = [b"ACGT" * 10 + b"A" * 70_000 + b"C", b"GT" * 40_000 + b"ACGTTGCA"]
SETTINGS = (1, 50, 3, 9)
SIDE = 4


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


def as_tuples(rows):
    return [(int(r["contig"]), int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]


def test_two_packed_scans_in_flight(ctx):
    import multi_gpu
    import prf_native
    from oracle import prf_oracle
    g = ctx.load(LONG_RUN, 50)
    try:
        rows, _ = g.scan(*SETTINGS)                                   # sizes the buffers the pipelined scans use
        assert as_tuples(rows) == [(c, s, e, k) for c, seq in enumerate(LONG_RUN) for s, e, _ml, k in prf_oracle.detect_rows(seq, *SETTINGS)]
        assert (0, 40, 70_040, 1) in as_tuples(rows) and (1, 0, 80_000, 2) in as_tuples(rows)
        cap = len(rows) + 5
        bufs = [torch.zeros(cap + 1 + 3 * SIDE, dtype=torch.int64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()                                      # (the library's stream does not wait for the fill)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        seqs = []
        for buf, stream in zip(bufs, streams):
            seqs.append(g.scan_async_packed(*SETTINGS, buf.data_ptr(), cap, SIDE))
            ctx.stream_wait_for(stream.cuda_stream)
        with pytest.raises(prf_native.PrfError):
            g.scan_async_packed(*SETTINGS, bufs[2].data_ptr(), cap, SIDE)     # two are in flight
        stats = [ctx.scan_wait(s) for s in seqs]
        torch.cuda.synchronize()
        assert [int(st.n_hits) for st in stats] == [len(rows)] * 2
        for buf in bufs[:2]:
            words = buf.cpu().numpy()
            assert np.array_equal(multi_gpu.unpack_rows(words, cap, SIDE, g.contig_bases(), prf_native.tile_positions()), rows)
            assert int(words.view(np.uint64)[cap]) >> 40 == 2         # n_side: the two rows longer than 65 534 positions
        again, _ = g.scan(*SETTINGS)                                  # no slot was left taken
        assert np.array_equal(again, rows)
    finally:
        g.free()
