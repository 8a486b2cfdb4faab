"""GPU (-m gpu): the chunked walk of interrupted repeats (prf_scan_interrupted_chunked, csrc/scan_interrupted.hip) against the
reference's RepeatTracker fixtures, the one-lane engine (chunk 0) and the CPU models (tests/interrupted_model.py,
tests/interrupted_chunks_model.py)."""
import random
import time
from collections import defaultdict

import pytest

import interrupted_chunks_model as C
import interrupted_model as M
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu

# The chr22-sized stand-in (k 1-6, r 3, span 9, m 1), one call: measured 14.6 s with chunk 2^20 and 11.4 s with chunk 2^18 on an
# MI355X; the limit is about three times the former.  The one-lane engine did not finish it within 200 s.
LARGE_LIMIT_S = 45.0
LARGE_ROWS = 143_877          # the CPU model's row count for this exact input (1 434 s)
# SHA-256 of the CPU model's rows for this exact input (interrupted_model.detect, stride 8, 2^22 slots; 1 017 s on a CPU)
# as _rows_digest() lays them out.  Never taken from a GPU's output.
LARGE_SHA256 = "e7d2d5911e727b2998eb3f0b271d84057fe58de9da113d82a900562d169a9dc5"


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


def _gpu_rows(ctx, seqs, kmin, kmax, r, span, m, **kw):
    """[[ (start, end, k, nmask), ... ] per sequence]."""
    out = ctx.scan_interrupted([s if isinstance(s, bytes) else s.encode() for s in seqs], kmin, kmax, r, span, m, **kw)
    per = [[] for _ in seqs]
    for row in out[0]:
        per[int(row["contig"])].append((int(row["start"]), int(row["end"]), int(row["k"]), int(row["nmask"])))
    return (per,) + tuple(out[1:])


def _model(seq, kmin, kmax, r, span, m):
    return [(a, b, k, mask) for a, b, k, mask, _motif in M.detect(seq, kmin, kmax, r, span, m, stride=8, slots=1 << 20)]


def _random_with_repeats(n, seed):
    rng = random.Random(seed)
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for _ in range(n // 2000):                 # planted interrupted repeats
        unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 6)))
        rep = bytearray(unit * rng.randint(3, 20))
        for _ in range(rng.randint(0, 3)):
            rep[rng.randrange(len(rep))] = rng.choice(b"ACGT")
        p = rng.randrange(n - len(rep))
        s[p:p + len(rep)] = rep
    return bytes(s)


def _rows_digest(rows):
    """SHA-256 of the rows as little-endian 64-bit (contig, start, end, k, nmask), row after row."""
    import hashlib
    import numpy as np
    a = np.stack([rows[f].astype("<u8") for f in ("contig", "start", "end", "k", "nmask")], axis=1)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("chunk", [32, 7])
def test_every_fixture_batched_in_chunks(ctx, chunk):
    """The 18 calls of tests/test_interrupted_gpu.py with chunks far shorter than most sequences (median 93 positions)."""
    cases = load_jsonl_gz("interrupted.jsonl.gz")
    groups = defaultdict(list)
    for c in cases:
        st = c["settings"]
        groups[(st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], st["max_interruptions"])].append(c)
    assert len(groups) <= 24
    bad, cut = [], 0
    for settings, group in groups.items():
        seqs = [c["seq"] for c in group]
        per, stats, ctr = _gpu_rows(ctx, seqs, *settings, chunk=chunk, counters=True)
        assert stats.path == 3 and stats.sorted_on_device == 1
        assert ctr["lanes"] == C.lane_count(seqs, settings[0], settings[1], chunk)
        cut += sum(len(M.trim(s)[0]) > chunk for s in seqs)
        for c, rows in zip(group, per):
            got = [[a, b, M.motif_text(c["seq"].upper().encode(), a, k, mask)] for a, b, k, mask in rows]
            if got != c["rows"]:
                bad.append((c["tag"], settings))
    assert not bad, f"{len(bad)} of {len(cases)} fixture cases differ: {bad[:5]}"
    assert cut > len(cases) // 2


CHUNKS = (4096, 10_000, 1 << 21)       # a power of two, one that is not, one larger than every sequence below


@pytest.mark.parametrize("n,kmin,kmax,m,seed", [
    (100_000, 1, 6, 1, 1),
    (300_000, 2, 6, 2, 3),
    (1_000_000, 1, 6, 1, 4),
])
def test_synthetic_equals_one_lane_and_model(ctx, n, kmin, kmax, m, seed):
    seq = _random_with_repeats(n, seed)
    (base,), _stats, c0 = _gpu_rows(ctx, [seq], kmin, kmax, 3, 9, m, chunk=0, counters=True)
    assert base == _model(seq, kmin, kmax, 3, 9, m) and len(base) > n // 5000
    assert c0["lanes"] == kmax - kmin + 1 and c0["dropped_lanes"] == 0
    for chunk in CHUNKS:
        (got,), _stats, ctr = _gpu_rows(ctx, [seq], kmin, kmax, 3, 9, m, chunk=chunk, counters=True)
        assert got == base, chunk
        assert ctr["lanes"] == C.lane_count([seq], kmin, kmax, chunk)
        assert ctr["hits"] > 0
        if chunk > n:
            assert ctr["lanes"] == kmax - kmin + 1 and ctr["dropped_lanes"] == 0
            assert ctr["steps"] == c0["steps"]
            if kmin > m:                                  # (a k <= m lane skips the memo lookups of its endless run)
                assert {x: ctr[x] for x in c0} == c0      # one chunk: the walk of the one-lane engine, counters included
        elif kmin <= m:
            assert ctr["dropped_lanes"] >= ctr["lanes"] // (kmax - kmin + 1) - 1      # k <= m: chunk 0 ends the walk


def test_lanes_and_dropped_lanes_are_the_models(ctx):
    # random ACGT: k 1 <= m and k 5, 6 are one episode (chunk 0 ends the walk), k 4 ends in the middle of the sequence
    rng = random.Random(7)
    seq = bytes(rng.choice(b"ACGT") for _ in range(60_000))
    for chunk in (4096, 10_000):
        want_ctr = {}
        want = [(a, b, k, mask) for a, b, k, mask, _m in C.detect_chunked(seq, 1, 6, 3, 9, 1, chunk, 8, 1 << 12, counters=want_ctr)]
        (got,), _stats, ctr = _gpu_rows(ctx, [seq], 1, 6, 3, 9, 1, chunk=chunk, counters=True)
        assert got == want
        assert ctr["lanes"] == want_ctr["lanes"] and ctr["dropped_lanes"] == want_ctr["dropped_lanes"] > 0


def test_absorbing_run_standin_with_n_blocks_and_batches(ctx):
    import synth
    standin = synth.chr_standin(length=200_000, seed=5, n_head=20_000, n_tail=3_000).tobytes()
    standin = standin[:90_000] + b"N" * 5_000 + standin[95_000:]      # an N block inside: N == N is a match for this tracker
    absorbing = b"NNNN" + _random_with_repeats(100_000, 6) + b"nn"
    for seq, kmin, kmax, m in ((standin, 1, 6, 1), (standin, 2, 6, 2), (absorbing, 1, 2, 2)):
        want = _model(seq, kmin, kmax, 3, 9, m)
        (base,), _stats = _gpu_rows(ctx, [seq], kmin, kmax, 3, 9, m, chunk=0)
        assert base == want
        for chunk in CHUNKS + (1000,):
            (got,), _stats, ctr = _gpu_rows(ctx, [seq], kmin, kmax, 3, 9, m, chunk=chunk, counters=True)
            assert got == want, (chunk, kmin, kmax, m)
            assert ctr["lanes"] == C.lane_count([seq], kmin, kmax, chunk)
            if kmin <= m and chunk < 100_000:
                assert ctr["dropped_lanes"] > 0
    # k <= m: the run starting at the first match never ends -- one row to the end of the trimmed sequence, motif all N
    (got,), _stats, ctr = _gpu_rows(ctx, [absorbing], 1, 1, 3, 9, 1, chunk=4096, counters=True)
    assert got[-1][1] == len(absorbing) - 2 and got[-1][3] == 1
    assert ctr["lanes"] == 25 and ctr["dropped_lanes"] == 24
    # several sequences of very different lengths in one call, empty and all-N ones among them
    seqs = [standin[:50_000], b"", absorbing[:30_000], b"NNNN", standin[100_000:100_300].lower(), b"ACGTT"]
    base, _stats = _gpu_rows(ctx, seqs, 1, 6, 3, 9, 1, chunk=0)
    for chunk in (64, 1000, 1 << 20):
        got, _stats, ctr = _gpu_rows(ctx, seqs, 1, 6, 3, 9, 1, chunk=chunk, counters=True)
        assert got == base, chunk
        assert ctr["lanes"] == C.lane_count(seqs, 1, 6, chunk)
    assert base[0] == _model(seqs[0], 1, 6, 3, 9, 1)


def test_memo_does_not_change_rows_when_chunked(ctx):
    seq = _random_with_repeats(20_000, 7)
    seqs = [seq, seq[:7_000], b"", b"NNNN", seq[3_000:15_000].lower()]
    base, _s, c0 = _gpu_rows(ctx, seqs, 1, 6, 3, 9, 1, memo_stride=0, memo_slots=0, counters=True, chunk=0)
    for chunk in (500, 4096):
        for stride, slots in ((0, 0), (8, 1 << 20), (1, 7), (64, 1 << 10)):
            got, _s, c1 = _gpu_rows(ctx, seqs, 1, 6, 3, 9, 1, memo_stride=stride, memo_slots=slots, counters=True, chunk=chunk)
            assert got == base, (chunk, stride, slots)
            assert (c1["hits"] > 0) == (stride > 0)
    assert c0["hits"] == 0
    assert base[0] == _model(seq, 1, 6, 3, 9, 1)


def test_cli_chunk_option_writes_the_same_bed(ctx, tmp_path, monkeypatch):
    import perfect_repeat_finder as prf
    a = _random_with_repeats(30_000, 8)
    b = b"nnnACGTACCTACGTACGTAcgtacgtacgtTTTTTTTTTTTTTGGGGGGGGGGGG" + _random_with_repeats(5_000, 9) + b"NN"
    beds = {}
    for chunk in ("0", "777", "4096", None):
        d = tmp_path / f"c{chunk}"
        d.mkdir()
        fa = d / "two.fa"
        with open(fa, "wb") as f:
            f.write(b">first desc\n" + a[:15_000] + b"\n" + a[15_000:] + b"\n>second\n" + b + b"\n")
        monkeypatch.chdir(d)
        prf.main(["--max-interruptions", "1", "-min", "1", "-max", "6"] + (["--interrupted-chunk", chunk] if chunk else []) + [str(fa)])
        beds[chunk] = open(d / "two.bed").read()
    want = []
    for name, seq in (("first", a), ("second", b)):
        want += [f"{name}\t{s}\t{e}\t{motif}\n" for s, e, _k, _mask, motif in M.detect(seq, 1, 6, 3, 9, 1, stride=8, slots=1 << 20)]
    assert beds["0"] == "".join(want) and len(want) > 5
    assert beds["777"] == beds["0"] and beds["4096"] == beds["0"] and beds[None] == beds["0"]


def test_chr22_sized_standin_finishes(ctx):
    """The reference's only benchmark of this mode, on the stand-in tools/interrupted_timing.py builds by default: the row count
    and the digest of the rows (contig, start, end, k, nmask) the CPU model found, the same rows for two chunk sizes,
    each call within LARGE_LIMIT_S.

    Measured on an MI355X: see DESIGN 9.5."""
    import numpy as np
    import synth
    length = synth.CHR22_LEN
    seq = synth.chr_standin(length=length, seed=22, n_head=min(10_510_000, length // 5), n_tail=min(10_000, length // 100)).tobytes()
    import prf_native
    seen = []
    for chunk in (prf_native.INT_CHUNK, 1 << 18):
        t = time.perf_counter()
        rows, stats, ctr = ctx.scan_interrupted([seq], 1, 6, 3, 9, 1, chunk=chunk, counters=True)
        wall = time.perf_counter() - t
        print(f"chunk {chunk}: {wall:.2f} s (device {stats.scan_ms / 1e3:.2f} s: walk {stats.phase1_ms / 1e3:.2f}, emission + sort "
              f"{stats.phase2_ms / 1e3:.2f}), {len(rows)} rows, {ctr['lanes']} lanes, {ctr['dropped_lanes']} dropped")
        assert len(rows) == LARGE_ROWS
        assert _rows_digest(rows) == LARGE_SHA256, f"chunk {chunk}: the rows differ from the CPU model's"
        assert wall < LARGE_LIMIT_S, f"chunk {chunk}: {wall:.1f} s"
        assert ctr["lanes"] == C.n_chunks(length - min(10_510_000, length // 5) - min(10_000, length // 100), chunk) * 6
        seen.append(rows)
    assert np.array_equal(seen[0], seen[1])
