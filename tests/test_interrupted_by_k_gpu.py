"""GPU (-m gpu): a budget of varying phases per motif size (prf_scan_interrupted_by_k, csrc/scan_interrupted.hip) against
the reference's RepeatTracker fixture (tests/golden/interrupted_by_k.jsonl.gz), the CPU models (tests/interrupted_model.py,
tests/interrupted_chunks_model.py) and the entry points with one budget for all motif sizes."""
import random
from collections import defaultdict

import pytest

import interrupted_by_k_model as K
import interrupted_chunks_model as C
import interrupted_model as M
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu

STAIRS = {1: 0, 2: 0, 3: 1, 4: 1, 5: 2, 6: 2, 7: 0, 8: 3}
ABSORB_2 = {**STAIRS, 2: 2}                  # the same with k = 2 <= m_2: the only motif size whose runs never end


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


def _gpu_rows(ctx, seqs, kmin, kmax, r, span, by_k, **kw):
    """[[ (start, end, k, nmask), ... ] per sequence], stats, counters."""
    out = ctx.scan_interrupted([s if isinstance(s, bytes) else s.encode() for s in seqs], kmin, kmax, r, span, 0,
                               max_interruptions_by_k=by_k, counters=True, **kw)
    per = [[] for _ in seqs]
    for row in out[0]:
        per[int(row["contig"])].append((int(row["start"]), int(row["end"]), int(row["k"]), int(row["nmask"])))
    return per, out[1], out[2]


def _random_with_repeats(n, seed):
    rng = random.Random(seed)
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for _ in range(n // 2000):                 # planted interrupted repeats
        unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 8)))
        rep = bytearray(unit * rng.randint(3, 20))
        for _ in range(rng.randint(0, 3)):
            rep[rng.randrange(len(rep))] = rng.choice(b"ACGT")
        p = rng.randrange(n - len(rep))
        s[p:p + len(rep)] = rep
    return bytes(s)


@pytest.fixture(scope="module")
def golden_groups():
    """The fixture's cases by (kmin, kmax, r, span, vector): one call each."""
    groups = defaultdict(list)
    for c in load_jsonl_gz("interrupted_by_k.jsonl.gz"):
        st = c["settings"]
        groups[(st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], tuple(st["max_interruptions_by_k"]))].append(c)
    assert len(groups) <= 40
    return groups


@pytest.mark.parametrize("chunk", [0, 7, 32, None])
def test_every_fixture_case(ctx, golden_groups, chunk):
    """One call per (settings, vector) through the one-lane engine (chunk 0), chunks of 7 and 32 positions and the default chunk:
    the rows and the varying phases (the N of the motif text) are the reference's."""
    import prf_native
    chunk = prf_native.INT_CHUNK if chunk is None else chunk
    bad, n_cases = [], 0
    for (kmin, kmax, r, span, vec), group in golden_groups.items():
        seqs = [c["seq"] for c in group]
        per, stats, ctr = _gpu_rows(ctx, seqs, kmin, kmax, r, span, list(vec), chunk=chunk)
        assert stats.path == 3 and stats.sorted_on_device == 1
        assert ctr["lanes"] == C.lane_count(seqs, kmin, kmax, chunk)
        n_cases += len(group)
        for c, rows in zip(group, per):
            got = [[a, b, M.motif_text(c["seq"].upper().encode(), a, k, mask)] for a, b, k, mask in rows]
            if got != c["rows"]:
                bad.append((c["tag"], len(c["seq"]), vec))
    assert not bad, f"{len(bad)} of {n_cases} fixture cases differ: {bad[:5]}"
    assert n_cases == 808


# ---- the model at 100 kb ----

class _Model:
    """The walks of three sequences of very different lengths, one per (sequence, k, budget), each made once: the candidate list of
    a (sequence, k) does not depend on the other motif sizes, so the rows of any vector over these budgets are one emission away."""

    def __init__(self):
        # the tail plants a perfect repeat of k = 1, 2 and 7 in the last chunk: their budget-0 walks land there, so none of their
        # chunks is dropped
        tail = b"C" + b"A" * 12 + b"C" + b"AC" * 8 + b"G" + b"ACGGTCA" * 4 + _random_with_repeats(2_000, 13)[:40]
        self.seqs = [b"NNN" + _random_with_repeats(100_000, 11) + tail + b"nn", _random_with_repeats(9_000, 12), b"ACGTTACGTTACGTAACGTT" * 15]
        self.trimmed = [M.trim(s) for s in self.seqs]
        self.walks = {}

    def walk(self, i, k, m):
        if (i, k, m) not in self.walks:
            self.walks[(i, k, m)] = M.walk(self.trimmed[i][0], k, 3, 9, m, stride=8, slots=1 << 16)
        return self.walks[(i, k, m)]

    def rows(self, i, vec):
        s, head = self.trimmed[i]
        out = M.emit([(k, self.walk(i, k, vec[k]).cands) for k in sorted(vec)])
        return [(a + head, b + head, k, mask) for (a, b), (k, mask) in sorted(out.items())]

    def dropped(self, i, k, m, chunk):
        """The chunks behind the one that holds the walk's last landing."""
        if chunk == 0:
            return 0
        landings = self.walk(i, k, m).landings
        return C.n_chunks(len(self.trimmed[i][0]), chunk) - 1 - (landings[-1] // chunk if landings else 0)


@pytest.fixture(scope="module")
def model():
    return _Model()


@pytest.mark.parametrize("chunk", [0, 4096, 1 << 16])
def test_three_sequences_equal_the_model(ctx, model, chunk):
    want = [model.rows(i, STAIRS) for i in range(3)]
    assert len(want[0]) > 40 and {k for _a, _b, k, _m in want[0]} >= {1, 2, 3, 4, 5, 6}
    got, _stats, ctr = _gpu_rows(ctx, model.seqs, 1, 8, 3, 9, STAIRS, chunk=chunk)
    assert got == want
    assert all(mask == 0 for rows in got for _a, _b, k, mask in rows if STAIRS[k] == 0)
    assert ctr["lanes"] == C.lane_count(model.seqs, 1, 8, chunk)
    assert ctr["dropped_lanes"] == sum(model.dropped(i, k, STAIRS[k], chunk) for i in range(3) for k in STAIRS)
    # a motif size of budget 0 on the long sequence: no lane is dropped (its walk lands in the last chunk)
    assert all(model.dropped(0, k, 0, chunk) == 0 for k in (1, 2, 7))


@pytest.mark.parametrize("chunk", [4096, 1 << 16])
def test_absorbing_skip_fires_for_exactly_one_motif_size(ctx, model, chunk):
    want = [model.rows(i, ABSORB_2) for i in range(3)]
    got, _stats, ctr = _gpu_rows(ctx, model.seqs, 1, 8, 3, 9, ABSORB_2, chunk=chunk)
    assert got == want
    # k = 2 <= m_2: chunk 0 of every sequence ends the walk and all its other chunks are dropped; nothing else changed
    per_k = {k: sum(model.dropped(i, k, ABSORB_2[k], chunk) for i in range(3)) for k in ABSORB_2}
    assert per_k[2] == sum(C.n_chunks(len(t), chunk) - 1 for t, _head in model.trimmed) > 0
    assert ctr["dropped_lanes"] == sum(per_k.values())
    assert all(per_k[k] == sum(model.dropped(i, k, STAIRS[k], chunk) for i in range(3)) for k in STAIRS if k != 2)
    assert got != [model.rows(i, STAIRS) for i in range(3)]


# ---- the older entry points are this one ----

def test_uniform_vector_is_the_chunked_entry_point(ctx):
    import numpy as np
    whole = _random_with_repeats(200_000, 21)
    for chunk, m, seq in ((4096, 1, whole), (1 << 16, 2, whole[:50_000]), (0, 1, whole[:20_000])):     # (the whole input once)
        old_rows, old_stats, old_ctr = ctx.scan_interrupted([seq], 1, 6, 3, 9, m, chunk=chunk, counters=True)
        new_rows, new_stats, new_ctr = ctx.scan_interrupted([seq], 1, 6, 3, 9, 0, chunk=chunk, counters=True, max_interruptions_by_k=[m] * 6)
        assert len(old_rows) > len(seq) // 2000 and np.array_equal(old_rows, new_rows)
        assert new_ctr == old_ctr
        assert (new_stats.n_candidates, new_stats.n_hits, new_stats.n_launches, new_stats.path) == \
            (old_stats.n_candidates, old_stats.n_hits, old_stats.n_launches, old_stats.path)
    # a dict that the scalar fills, and a sequence that agrees with the scalar
    seq = whole[:20_000]
    a, _s = ctx.scan_interrupted([seq], 1, 6, 3, 9, 1, chunk=4096, max_interruptions_by_k={})
    b, _s = ctx.scan_interrupted([seq], 1, 6, 3, 9, 1, chunk=4096, max_interruptions_by_k=[1] * 6)
    c, _s = ctx.scan_interrupted([seq], 1, 6, 3, 9, 1, chunk=4096)
    assert np.array_equal(a, c) and np.array_equal(b, c)
    with pytest.raises(ValueError):
        ctx.scan_interrupted([seq], 1, 6, 3, 9, 1, chunk=4096, max_interruptions_by_k=[1, 1, 1, 2, 1, 1])


def test_all_zero_vector_is_the_model_with_no_interruptions(ctx):
    import prf_native
    seq = b"nN" + _random_with_repeats(50_000, 22) + b"N"
    want = [(a, b, k, mask) for a, b, k, mask, _motif in M.detect(seq, 1, 6, 3, 9, 0, stride=8, slots=1 << 16)]
    assert len(want) > 20 and all(mask == 0 for _a, _b, _k, mask in want)
    for chunk in (0, 1000, prf_native.INT_CHUNK):
        (got,), _stats, ctr = _gpu_rows(ctx, [seq], 1, 6, 3, 9, [0] * 6, chunk=chunk)
        assert got == want, chunk
        assert ctr["lanes"] == C.lane_count([seq], 1, 6, chunk)
    # the entry points with one budget keep their refusal of 0
    with pytest.raises(prf_native.PrfError) as exc:
        ctx.scan_interrupted([seq], 1, 6, 3, 9, 0, chunk=1000)
    assert exc.value.code == prf_native.PRF_EINVAL


def test_cli_writes_the_models_bed(ctx, tmp_path, monkeypatch):
    import perfect_repeat_finder as prf
    records = [("first", _random_with_repeats(4_000, 31)),
               ("second", b"nnnACGTACCTACGTACGTAcgtacgtacgtTTTTTTTTTTTTTGGGGGGGGGGGGAAAAAAAAAAAA" + _random_with_repeats(2_500, 32) + b"NN"),
               ("third", b"CAGCAGCATCAGCAGCTGCAGCAG" * 3 + _random_with_repeats(2_000, 33)[:1_500])]
    fa = tmp_path / "three.fa"
    with open(fa, "wb") as f:
        for name, seq in records:
            f.write(b">" + name.encode() + b" desc\n" + seq[:1_000] + b"\n" + seq[1_000:] + b"\n")
    monkeypatch.chdir(tmp_path)
    beds = {}
    for extra in ((), ("--interrupted-chunk", "777"), ("--max-interruptions", "1")):
        prf.main(["--max-interruptions-by-motif-size", "1-2:0,3-:1", "-min", "1", "-max", "6", *extra, str(fa)])
        beds[extra] = open(tmp_path / "three.bed").read()
    want = []
    for name, seq in records:
        want += [f"{name}\t{s}\t{e}\t{motif}\n" for s, e, _k, _mask, motif in
                 K.detect(seq, 1, 6, 3, 9, {1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 1}, stride=8, slots=1 << 16)]
    assert len(want) > 10 and any("N" in line.split("\t")[3] for line in want)
    assert all(bed == "".join(want) for bed in beds.values())
    # the scalar fills the motif sizes the SPEC leaves out
    prf.main(["--max-interruptions-by-motif-size", "1-2:0", "--max-interruptions", "1", "-min", "1", "-max", "6", str(fa)])
    assert open(tmp_path / "three.bed").read() == "".join(want)
    prf.main(["--max-interruptions", "1", "-min", "1", "-max", "6", str(fa)])
    assert open(tmp_path / "three.bed").read() != "".join(want)
