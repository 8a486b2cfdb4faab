"""CPU: the interrupted-repeat model (tests/interrupted_model.py) against the reference's RepeatTracker fixtures, the memo walk
against the plain walk, and the new entry point's ABI and refusals (no GPU needed)."""
import argparse
import ctypes
import random

import pytest

import interrupted_model as M
from conftest import load_jsonl_gz


@pytest.fixture(scope="module")
def golden_interrupted():
    return load_jsonl_gz("interrupted.jsonl.gz")


def _model_rows(case, stride=0, slots=0, episodes=None):
    st = case["settings"]
    rows = M.detect(case["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"],
                    st["max_interruptions"], stride, slots, episodes)
    return [[a, b, motif] for a, b, _k, _mask, motif in rows]


def test_fixture_covers_the_regimes(golden_interrupted):
    assert len(golden_interrupted) >= 3000
    tags = {c["tag"] for c in golden_interrupted}
    assert {"random", "planted", "homopolymer", "n_iupac", "lower", "large_k", "absorbing", "n_ends", "dense"} <= tags
    assert max(c["settings"]["max_motif_size"] for c in golden_interrupted) == 64
    assert {c["settings"]["max_interruptions"] for c in golden_interrupted} == {1, 2, 3}
    assert sum(len(c["rows"]) for c in golden_interrupted) > 3000
    # an absorbing run of k = 1 <= m: one row from the first match to the end, motif N
    assert any(c["tag"] == "absorbing" and any(m == "N" for _a, _b, m in c["rows"]) for c in golden_interrupted)


@pytest.mark.parametrize("mode", ["plain", "memo", "memo_tiny"])
def test_model_matches_every_fixture(golden_interrupted, mode):
    stride, slots, episodes = {"plain": (0, 0, None), "memo": (8, 1 << 12, None), "memo_tiny": (2, 3, 2)}[mode]
    bad = [c["tag"] for c in golden_interrupted if _model_rows(c, stride, slots, episodes) != c["rows"]]
    assert not bad, f"{len(bad)} of {len(golden_interrupted)} cases differ ({bad[:5]})"


@pytest.mark.parametrize("n,seed", [(2_000, 1), (10_000, 2), (100_000, 3)])
def test_memo_walk_equals_plain_walk(n, seed):
    rng = random.Random(seed)
    seq = bytes(rng.choice(b"ACGT") for _ in range(n))
    ks = range(2, 5) if n > 20_000 else range(1, 7)
    for k in ks:
        memo = M.walk(seq, k, 3, 9, 1, stride=8, slots=1 << 16)
        if n > 20_000:
            # the plain walk is quadratic on random sequence (tens of thousands of steps per position at 100 kb): compare
            # a memo walk with a very different table instead
            other = M.walk(seq, k, 3, 9, 1, stride=3, slots=1 << 10, episodes=n // 50)
        else:
            other = M.walk(seq, k, 3, 9, 1)
        assert memo.cands == other.cands, k
        for w in (memo, other):
            assert all(a < b for a, b in zip(w.landings, w.landings[1:])), "jump landings must increase strictly"


def test_memo_cuts_the_walk():
    rng = random.Random(4)
    seq = bytes(rng.choice(b"ACGT") for _ in range(10_000))
    plain = M.walk(seq, 3, 3, 9, 1)
    memo = M.walk(seq, 3, 3, 9, 1, stride=8, slots=1 << 14)
    assert memo.cands == plain.cands
    assert memo.hits > 0 and memo.steps * 5 < plain.steps


def test_absorbing_run_reports_one_row_to_the_end():
    rows = M.detect("ggACGTTGCA", 1, 1, 3, 3, 1)
    assert [(a, b, m) for a, b, _k, _mask, m in rows] == [(0, 10, "N")]


# ---- the C ABI of the new entry point (refusals are decided before the context is touched) ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _call(lib, pn, kmin, kmax, r, span, m, seqs=(b"ACGTACGT",), ctx=None):
    arr, _keep = pn._contig_array(list(seqs))
    hits, stats = pn._IHits(), pn.ScanStats()
    return lib.prf_scan_interrupted(ctx, arr, len(seqs), kmin, kmax, r, span, m, ctypes.byref(hits), ctypes.byref(stats))


def test_ihit_layout_matches_the_header():
    pn, _lib_ = _lib()
    assert ctypes.sizeof(pn._IHit) == 32
    assert pn._IHit.nmask.offset == 24


@pytest.mark.parametrize("args,code", [
    ((2, 6, 1, 9, 1), "PRF_EUNSUPPORTED"),   # min_repeats == 1
    ((2, 65, 3, 9, 1), "PRF_EUNSUPPORTED"),  # kmax > 64: the phase set is one 64-bit mask
    ((2, 6, 3, 9, 0), "PRF_EINVAL"),         # max_interruptions == 0 is the perfect path's
    ((0, 6, 3, 9, 1), "PRF_EINVAL"),
    ((4, 3, 3, 9, 1), "PRF_EINVAL"),
    ((2, 6, 3, 0, 1), "PRF_EINVAL"),
    ((2, 6, 3, 9, 1), "PRF_EINVAL"),         # valid parameters, NULL context
])
def test_refusals(args, code):
    pn, lib = _lib()
    assert _call(lib, pn, *args) == getattr(pn, code)
    assert lib.prf_last_error()


def test_detect_repeats_refuses_interval_mode_with_interruptions():
    import perfect_repeat_finder as prf
    fs = argparse.Namespace(min_motif_size=2, max_motif_size=6, min_repeats=3, min_span=9, max_interruptions=1,
                            interval_start_0based=0, interval_end=10)
    with pytest.raises(ValueError, match="interval"):
        prf.detect_repeats("ACGTACGTACGT", fs)


def test_cli_refuses_interval_and_multi_rank(tmp_path, monkeypatch, capsys):
    import perfect_repeat_finder as prf
    fa = tmp_path / "x.fa"
    fa.write_text(">a\nACGTACGTACGTACGT\n")
    with pytest.raises(SystemExit):
        prf.main(["--max-interruptions", "1", "-i", "a:0-10", str(fa)])
    assert "--interval" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        prf.main(["--max-interruptions", "1", str(fa)])
    assert "one process" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        prf.main(["--max-interruptions", "-1", str(fa)])
