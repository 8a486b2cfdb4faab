"""GPU (-m gpu): interrupted repeats (prf_scan_interrupted, csrc/scan_interrupted.hip) against the reference's RepeatTracker
fixtures and against the CPU model (tests/interrupted_model.py)."""
import argparse
import os
import random
from collections import defaultdict

import numpy as np
import pytest

import interrupted_model as M
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu


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
    rows = out[0]
    per = [[] for _ in seqs]
    for row in rows:
        per[int(row["contig"])].append((int(row["start"]), int(row["end"]), int(row["k"]), int(row["nmask"])))
    return (per,) + tuple(out[1:])


def _model(seq, kmin, kmax, r, span, m):
    return [(a, b, k, mask) for a, b, k, mask, _motif in M.detect(seq, kmin, kmax, r, span, m, stride=8, slots=1 << 20)]


def test_every_fixture_batched(ctx):
    cases = load_jsonl_gz("interrupted.jsonl.gz")
    groups = defaultdict(list)
    for c in cases:
        st = c["settings"]
        groups[(st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], st["max_interruptions"])].append(c)
    assert len(groups) <= 24
    bad = []
    for settings, group in groups.items():
        per, stats = _gpu_rows(ctx, [c["seq"] for c in group], *settings)
        assert stats.path == 3 and stats.sorted_on_device == 1
        for c, rows in zip(group, per):
            got = [[a, b, M.motif_text(c["seq"].upper().encode(), a, k, mask)] for a, b, k, mask in rows]
            if got != c["rows"]:
                bad.append((c["tag"], settings))
    assert not bad, f"{len(bad)} of {len(cases)} fixture cases differ: {bad[:5]}"


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


@pytest.mark.parametrize("n,kmin,kmax,m,seed", [
    (100_000, 1, 6, 1, 1),
    (100_000, 1, 6, 2, 2),
    (300_000, 2, 6, 2, 3),
    (1_000_000, 1, 6, 1, 4),
])
def test_synthetic_equals_model(ctx, n, kmin, kmax, m, seed):
    seq = _random_with_repeats(n, seed)
    (got,), stats, ctr = _gpu_rows(ctx, [seq], kmin, kmax, 3, 9, m, counters=True)
    want = _model(seq, kmin, kmax, 3, 9, m)
    assert got == want
    assert len(got) > n // 5000
    assert ctr["hits"] > 0 and ctr["steps"] < 20 * n * (kmax - kmin + 1)


def test_absorbing_run_and_standin_with_n_blocks(ctx):
    import synth
    standin = synth.chr_standin(length=200_000, seed=5, n_head=20_000, n_tail=3_000).tobytes()
    standin = standin[:90_000] + b"N" * 5_000 + standin[95_000:]      # an N block inside: N == N is a match for this tracker
    absorbing = b"NNNN" + _random_with_repeats(100_000, 6) + b"nn"
    for seq, kmin, kmax, m in ((standin, 1, 6, 1), (standin, 2, 6, 2), (absorbing, 1, 2, 2)):
        (got,), _stats = _gpu_rows(ctx, [seq], kmin, kmax, 3, 9, m)
        assert got == _model(seq, kmin, kmax, 3, 9, m)
    # k <= m: the run starting at the first match never ends -- one row to the end of the trimmed sequence, motif all N
    (got,), _stats = _gpu_rows(ctx, [absorbing], 1, 1, 3, 9, 1)
    assert got[-1][1] == len(absorbing) - 2 and got[-1][3] == 1


def test_memo_does_not_change_rows(ctx):
    seq = _random_with_repeats(20_000, 7)
    seqs = [seq, seq[:7_000], b"", b"NNNN", seq[3_000:15_000].lower()]
    base, _s, c0 = _gpu_rows(ctx, seqs, 1, 6, 3, 9, 1, memo_stride=0, memo_slots=0, counters=True)
    for stride, slots in ((8, 1 << 20), (1, 7), (64, 1 << 10)):
        got, _s, c1 = _gpu_rows(ctx, seqs, 1, 6, 3, 9, 1, memo_stride=stride, memo_slots=slots, counters=True)
        assert got == base, (stride, slots)
    assert c0["hits"] == 0 and c1["hits"] > 0
    assert base[0] == _model(seq, 1, 6, 3, 9, 1)


def test_cli_writes_the_models_bed(ctx, tmp_path, monkeypatch):
    import perfect_repeat_finder as prf
    a = _random_with_repeats(30_000, 8)
    b = b"nnnACGTACCTACGTACGTAcgtacgtacgtTTTTTTTTTTTTTGGGGGGGGGGGG" + _random_with_repeats(5_000, 9) + b"NN"
    fa = tmp_path / "two.fa"
    with open(fa, "wb") as f:
        f.write(b">first desc\n" + a[:15_000] + b"\n" + a[15_000:] + b"\n>second\n" + b + b"\n")
    monkeypatch.chdir(tmp_path)
    prf.main(["--max-interruptions", "1", "-min", "1", "-max", "6", str(fa)])
    want = []
    for name, seq in (("first", a), ("second", b)):
        want += [f"{name}\t{s}\t{e}\t{motif}\n" for s, e, _k, _mask, motif in M.detect(seq, 1, 6, 3, 9, 1, stride=8, slots=1 << 20)]
    got = open(tmp_path / "two.bed").read()
    assert got == "".join(want) and len(want) > 5


def test_detect_repeats_takes_the_interrupted_lane(ctx):
    import perfect_repeat_finder as prf
    seq = "ttgcaCAGCAGCAGCATCAGCAGCAGCAGTTTACG" * 3
    fs = argparse.Namespace(min_motif_size=1, max_motif_size=6, min_repeats=3, min_span=9, max_interruptions=1)
    want = [(a, b, motif) for a, b, _k, _mask, motif in M.detect(seq, 1, 6, 3, 9, 1)]
    assert prf.detect_repeats(seq, fs, context=ctx) == want and any("N" in m for _a, _b, m in want)
    with pytest.raises(ValueError):
        prf.detect_repeats("ACGT-ACGT", fs, context=ctx)


def test_max_interruptions_zero_keeps_the_perfect_rows(ctx):
    import perfect_repeat_finder as prf
    import synth
    seq = synth.chr_standin(length=120_000, seed=11, n_head=5_000, n_tail=100).tobytes().decode()
    for st in (dict(min_motif_size=1, max_motif_size=50, min_repeats=3, min_span=9),
               dict(min_motif_size=1, max_motif_size=8, min_repeats=1, min_span=7)):
        plain = prf.detect_repeats(seq, argparse.Namespace(**st), context=ctx)
        zero = prf.detect_repeats(seq, argparse.Namespace(max_interruptions=0, **st), context=ctx)
        assert zero == plain and len(plain) > 50
