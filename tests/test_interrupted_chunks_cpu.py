"""CPU: the chunked walk of interrupted repeats (tests/interrupted_chunks_model.py).  The landings of a walk are the
boundaries in order, the walk cut into chunks of landing positions gives the rows of the whole walk, and the new entry point's
ABI and refusals (no GPU needed)."""
import ctypes
import random

import pytest

import interrupted_chunks_model as C
import interrupted_model as M
from conftest import load_jsonl_gz


def _claim_cases():
    """400 cases: lengths 30-5000, four alphabets, planted repeats, k 1-8 (k <= m included), r 2/3/5, span 1/9/20, m 1-3."""
    rng = random.Random(20261016)
    for _ in range(400):
        n = rng.choice([30, 100, 1000, 5000])
        alpha = rng.choice([b"ACGT", b"AC", b"ACGTN", b"AAAC"])
        s = bytes(rng.choice(alpha) for _ in range(n))
        if rng.random() < 0.3:
            unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 6)))
            at = rng.randrange(n)
            s = s[:at] + unit * rng.randint(3, 30) + s[at:]
        yield s, rng.randint(1, 8), rng.choice([2, 3, 5]), rng.choice([1, 9, 20]), rng.choice([1, 2, 3])


def test_landings_are_the_boundaries_in_order():
    absorbed = 0
    for s, k, r, span, m in _claim_cases():
        w = M.walk(s, k, r, span, m)
        b = C.boundaries(s, k)
        assert w.landings == b[:len(w.landings)], (len(s), k, r, span, m)
        absorbed += len(w.landings) < len(b)
        # a memo walk jumps between the same landings
        assert M.walk(s, k, r, span, m, stride=4, slots=1 << 10).landings == w.landings
    assert absorbed > 20          # the walk ended before the last boundary (claim 3) in a fair share of the cases


def test_one_episode_per_boundary_lists_the_walks_candidates():
    for i, (s, k, r, span, m) in enumerate(_claim_cases()):
        if i % 4:
            continue
        want = M.walk(s, k, r, span, m).cands
        got = []
        for b in [0] + C.boundaries(s, k):      # a piece per landing: [b, b + 1) holds exactly the episode that lands on b
            if 0 < b < 2:
                continue                         # (a boundary is at least 2)
            p = C.walk_range(s, k, r, span, m, b, b + 1)
            assert p.has_work and p.episodes == 1
            got += p.cands
            if p.at_end:
                break
        assert got == want, (len(s), k, r, span, m)


@pytest.fixture(scope="module")
def golden_interrupted():
    return load_jsonl_gz("interrupted.jsonl.gz")


@pytest.mark.parametrize("chunk,memo", [(7, (0, 0, None)), (64, (8, 1 << 10, None)), (1000, (2, 3, 2)), (2, (0, 0, None))])
def test_chunked_model_matches_every_fixture(golden_interrupted, chunk, memo):
    cases = golden_interrupted if chunk != 2 else golden_interrupted[::8]
    bad, many = [], 0
    for c in cases:
        st = c["settings"]
        ctr = {}
        rows = C.detect_chunked(c["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"],
                                st["max_interruptions"], chunk, *memo, counters=ctr)
        many += ctr["lanes"] > st["max_motif_size"] - st["min_motif_size"] + 1
        if [[a, b, motif] for a, b, _k, _mask, motif in rows] != c["rows"]:
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} of {len(cases)} cases differ ({bad[:5]})"
    # the fixtures' sequences (0-600 positions, median 93) really were cut; 1000 holds each of them in one chunk
    assert many == 0 if chunk == 1000 else many > len(cases) // 2


def test_chunk_zero_and_one_large_chunk_are_the_whole_walk():
    rng = random.Random(5)
    seq = bytes(rng.choice(b"ACGT") for _ in range(3_000))
    want = M.detect(seq, 1, 6, 3, 9, 1)
    ctr = {}
    assert C.detect_chunked(seq, 1, 6, 3, 9, 1, 0, counters=ctr) == want
    assert ctr["lanes"] == 6 and ctr["dropped_lanes"] == 0
    ctr = {}
    assert C.detect_chunked(seq, 1, 6, 3, 9, 1, 1 << 20, 8, 1 << 10, counters=ctr) == want
    assert ctr["lanes"] == 6 and ctr["idle_lanes"] == 0
    assert C.lane_count([seq, b"NN" + seq[:100] + b"N", b""], 1, 6, 64) == 6 * (47 + 2 + 1)


def test_a_chunk_without_a_boundary_has_no_work():
    # k = 3 on a long perfect run: match everywhere inside it, so no boundary for several chunks
    rng = random.Random(6)
    left = bytes(rng.choice(b"ACGT") for _ in range(200))
    right = bytes(rng.choice(b"ACGT") for _ in range(200))
    seq = left + b"CAG" * 200 + right
    assert not [b for b in C.boundaries(seq, 3) if 264 <= b < 700]
    for chunk in (16, 50, 128):
        ctr = {}
        got = C.detect_chunked(seq, 3, 3, 3, 9, 1, chunk, counters=ctr)
        assert got == M.detect(seq, 3, 3, 3, 9, 1) and any(b - a >= 600 for a, b, *_ in got)
        assert ctr["idle_lanes"] >= 400 // chunk
    idle = C.walk_range(seq, 3, 3, 9, 1, 320, 384)
    assert not idle.has_work and not idle.cands and not idle.at_end


def test_chunks_behind_the_end_of_the_walk_are_dropped():
    # random ACGT, r 3, span 9, m 1.  k 6: the reference walk is one episode (the varying phase absorbs the mismatches until the end
    # of the sequence), so chunk 0 ends the walk and the 14 lanes behind it are dropped.  k 4: the walk ends in an episode that
    # lands in the middle of the sequence, and the chunks behind it list candidates of landings the walk never reaches.
    rng = random.Random(7)
    seq = bytes(rng.choice(b"ACGT") for _ in range(60_000))
    whole = M.walk(seq, 6, 3, 9, 1, stride=8, slots=1 << 16)
    assert whole.landings == [] and len(C.boundaries(seq, 6)) > 10_000
    ctr = {}
    assert C.walk_chunked(seq, 6, 3, 9, 1, 4096, stride=8, slots=1 << 12, counters=ctr) == whole.cands
    assert ctr["lanes"] == 15 and ctr["dropped_lanes"] == 14 and ctr["idle_lanes"] == 0
    whole = M.walk(seq, 4, 3, 9, 1, stride=8, slots=1 << 16)
    last = whole.landings[-1] // 4096
    assert 0 < last < 13
    ctr = {}
    assert C.walk_chunked(seq, 4, 3, 9, 1, 4096, stride=8, slots=1 << 12, counters=ctr) == whole.cands
    assert ctr["dropped_lanes"] == 14 - last and ctr["dropped_candidates"] > 100
    ctr = {}
    assert C.detect_chunked(seq, 1, 6, 3, 9, 1, 10_000, 8, 1 << 12, counters=ctr) == M.detect(seq, 1, 6, 3, 9, 1, 8, 1 << 16)
    assert ctr["lanes"] == 36 and ctr["dropped_lanes"] >= 15      # k = 1 <= m never leaves its first run; k 5 and 6 as above


def test_memo_settings_do_not_change_the_pieces():
    rng = random.Random(8)
    seq = bytes(rng.choice(b"ACGT") for _ in range(8_000))
    for k in (2, 3, 5):
        for c in range(4):
            plain = C.walk_range(seq, k, 3, 9, 1, c * 2000, (c + 1) * 2000)
            memo = C.walk_range(seq, k, 3, 9, 1, c * 2000, (c + 1) * 2000, stride=8, slots=1 << 9)
            tiny = C.walk_range(seq, k, 3, 9, 1, c * 2000, (c + 1) * 2000, stride=1, slots=5, episodes=3)
            assert plain.cands == memo.cands == tiny.cands and plain.landings == memo.landings == tiny.landings
            assert plain.at_end == memo.at_end == tiny.at_end
            assert memo.steps <= plain.steps
            assert all(c * 2000 <= p < (c + 1) * 2000 for p in plain.landings)


# ---- the C ABI of prf_scan_interrupted_chunked (refusals are decided before the context is touched) ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _call(lib, pn, kmin, kmax, r, span, m, chunk, seqs=(b"ACGTACGT",), ctx=None):
    arr, _keep = pn._contig_array(list(seqs))
    hits, stats = pn._IHits(), pn.ScanStats()
    ctr = (ctypes.c_uint64 * 6)()
    return lib.prf_scan_interrupted_chunked(ctx, arr, len(seqs), kmin, kmax, r, span, m, 8, 1 << 10, chunk, ctypes.byref(hits),
                                            ctypes.byref(stats), ctr)


def test_entry_point_is_exported_and_the_abi_version_stays():
    pn, lib = _lib()
    assert hasattr(lib, "prf_scan_interrupted_chunked")
    assert "prf_scan_interrupted_chunked" in pn.EXPORTS
    assert lib.prf_abi_version() == 4
    assert pn.INT_CHUNK >= 1 << 20 and pn.INT_CHUNK_MIN >= 2


@pytest.mark.parametrize("args,code", [
    ((2, 6, 3, 9, 1, 1), "PRF_EINVAL"),            # a chunk below the minimum
    ((2, 6, 3, 9, 0, 4096), "PRF_EINVAL"),         # max_interruptions == 0 is the perfect path's
    ((2, 6, 1, 9, 1, 4096), "PRF_EUNSUPPORTED"),   # min_repeats == 1
    ((2, 65, 3, 9, 1, 4096), "PRF_EUNSUPPORTED"),  # kmax > 64
    ((2, 6, 3, 9, 1, 4096), "PRF_EINVAL"),         # valid parameters, NULL context
    ((2, 6, 3, 9, 1, 0), "PRF_EINVAL"),            # chunk 0 is valid too: NULL context
])
def test_refusals(args, code):
    pn, lib = _lib()
    assert _call(lib, pn, *args) == getattr(pn, code)
    assert lib.prf_last_error()


def test_chunk_below_minimum_is_named_in_the_error():
    pn, lib = _lib()
    assert _call(lib, pn, 2, 6, 3, 9, 1, pn.INT_CHUNK_MIN - 1) == pn.PRF_EINVAL
    assert b"chunk" in lib.prf_last_error()


def test_cli_has_the_chunk_option(tmp_path, capsys):
    import perfect_repeat_finder as prf
    fa = tmp_path / "x.fa"
    fa.write_text(">a\nACGTACGTACGTACGT\n")
    with pytest.raises(SystemExit):
        prf.main(["--max-interruptions", "1", "--interrupted-chunk", "-5", str(fa)])
    assert "--interrupted-chunk" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        prf.main(["--max-interruptions", "1", "--interrupted-chunk", "64", "-i", "a:0-10", str(fa)])
    assert "--interval" in capsys.readouterr().err
