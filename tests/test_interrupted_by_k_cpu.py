"""CPU: a budget of varying phases per motif size (prf_scan_interrupted_by_k, --max-interruptions-by-motif-size).  The
models with a budget per k equal the reference's RepeatTracker fixture (tests/golden/interrupted_by_k.jsonl.gz), the chunk argument
of DESIGN 9.1.5 holds for a budget of 0, the command line's SPEC parser, the all-zero dict that must stay on the perfect path, and
the new entry point's ABI and refusals (no GPU needed)."""
import argparse
import ctypes
import random

import pytest

import interrupted_by_k_model as K
import interrupted_chunks_model as C
import interrupted_model as M
from conftest import load_jsonl_gz

LONG = 5_000        # the fixture's cases are at most 600 positions, or 5-10 kb


@pytest.fixture(scope="module")
def golden_by_k():
    return load_jsonl_gz("interrupted_by_k.jsonl.gz")


def _settings(c):
    st = c["settings"]
    return st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], st["max_interruptions_by_k"]


def test_the_fixture_is_what_the_tool_promises(golden_by_k):
    short = [c for c in golden_by_k if len(c["seq"]) <= 600]
    long_ = [c for c in golden_by_k if len(c["seq"]) >= LONG]
    assert len(short) == 800 and len(long_) == 8 and all(len(c["seq"]) <= 10_400 for c in long_)
    assert len({repr(_settings(c)) for c in golden_by_k}) <= 40
    budgets = [(c["settings"]["min_motif_size"] + j, m) for c in golden_by_k for j, m in enumerate(_settings(c)[4])]
    assert all(len(_settings(c)[4]) == _settings(c)[1] - _settings(c)[0] + 1 for c in golden_by_k)
    assert {m for _k, m in budgets} == {0, 1, 2, 3}
    assert 3 * sum(m == 0 for _k, m in budgets) >= len(budgets)
    assert sum(k <= m for k, m in budgets) > 40
    assert any(v[4] == [0 if k % 2 == 0 else 2 for k in range(16, 65)] for v in map(_settings, long_))


@pytest.mark.parametrize("mode", ["memo", "chunks_7", "chunks_1000"])
def test_model_matches_every_fixture_case(golden_by_k, mode):
    bad, differ = [], 0
    for c in golden_by_k:
        kmin, kmax, r, span, vec = _settings(c)
        if mode == "memo":
            rows = K.detect(c["seq"], kmin, kmax, r, span, vec, stride=8, slots=1 << 16)
            if len(c["seq"]) <= 600:        # the budgets matter: the uniform budget max(m_k) gives other rows
                differ += M.detect(c["seq"], kmin, kmax, r, span, max(vec), stride=8, slots=1 << 16) != rows
        elif len(c["seq"]) >= LONG:
            continue                        # the 5-10 kb cases: the memo walk only
        else:
            rows = K.detect_chunked(c["seq"], kmin, kmax, r, span, vec, int(mode.split("_")[1]), stride=8, slots=1 << 10)
        if [[a, b, motif] for a, b, _k, _mask, motif in rows] != c["rows"]:
            bad.append((c["tag"], len(c["seq"]), vec))
    assert not bad, f"{len(bad)} cases differ ({bad[:5]})"
    if mode == "memo":
        assert differ >= 400


def test_budget_argument_forms_agree():
    rng = random.Random(3)
    seq = bytes(rng.choice(b"ACGT") for _ in range(400)) + b"CAGCAGCATCAGCAGCTGCAG" * 3
    as_list = K.detect(seq, 2, 5, 3, 9, [0, 1, 0, 2])
    assert as_list == K.detect(seq, 2, 5, 3, 9, {3: 1, 5: 2}) == K.detect(seq, 2, 5, 3, 9, {2: 0, 4: 0, 5: 2}, max_interruptions=1)
    assert as_list == K.detect_chunked(seq, 2, 5, 3, 9, {3: 1, 5: 2, 9: 3}, 64)
    assert M.detect(seq, 2, 5, 3, 9, 2) == K.detect(seq, 2, 5, 3, 9, [2] * 4) == K.detect(seq, 2, 5, 3, 9, {}, max_interruptions=2)
    assert M.detect(seq, 2, 5, 3, 9, 2) == K.detect(seq, 2, 5, 3, 9, None, max_interruptions=2) == K.detect_chunked(seq, 2, 5, 3, 9, [2] * 4, 0)
    assert as_list != M.detect(seq, 2, 5, 3, 9, 2)


def test_landings_are_the_boundaries_in_order_with_budget_zero():
    """DESIGN 9.1.5 for max_interruptions = 0: the walk still records its first interruption and every reset still lands on it + 1,
    so the chunks cut a budget-0 walk as they cut the others."""
    rng = random.Random(20261017)
    walked = landings = 0
    for _ in range(300):
        n = rng.choice([30, 100, 400, 1500])
        alpha = rng.choice([b"ACGT", b"AC", b"ACGTN", b"AAC"])
        s = bytes(rng.choice(alpha) for _ in range(n))
        if rng.random() < 0.3:
            unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 6)))
            at = rng.randrange(n)
            s = s[:at] + unit * rng.randint(3, 30) + s[at:]
        k, r, span = rng.randint(1, 8), rng.choice([2, 3, 5]), rng.choice([1, 9, 20])
        w = M.walk(s, k, r, span, 0)
        b = C.boundaries(s, k)
        assert w.landings == b[:len(w.landings)], (len(s), k, r, span)
        assert all(mask == 0 for _a, _b, mask, _h in w.cands)
        assert M.walk(s, k, r, span, 0, stride=4, slots=1 << 10).landings == w.landings
        for chunk in (7, 64):
            assert C.walk_chunked(s, k, r, span, 0, chunk) == w.cands
        walked += len(w.landings) > 3
        landings += len(w.landings)
    # (a jump back follows a check that passes both span tests: without varying phases that is rare on four random letters)
    assert walked > 60 and landings > 5_000


# ---- the command line's SPEC and how it composes with --max-interruptions ----

def test_spec_parser_good_forms():
    import perfect_repeat_finder as prf
    assert prf.parse_interruption_spec("1-2:0,3-6:1,7-:2", 1, 9) == {1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 1, 7: 2, 8: 2, 9: 2}
    assert prf.parse_interruption_spec("4:3", 1, 9) == {4: 3}
    assert prf.parse_interruption_spec("9-:1, 2-2:0", 2, 9) == {9: 1, 2: 0}
    assert prf.parse_interruption_spec("3-:0", 3, 3) == {3: 0}


@pytest.mark.parametrize("spec", ["1-3:0,3:1", "1-:0,5:1", "x", "3", "1-:", "3-2:1", "-3:1", "1:1:1", "", "1:0,,2:0", "1:-1", "2:1.5",
                                  "0:1", "5-12:1", "10-:1", "1:0", "1 -2:0"])
def test_spec_parser_bad_forms(spec):
    import perfect_repeat_finder as prf
    with pytest.raises(ValueError):
        prf.parse_interruption_spec(spec, 2, 9)


def test_bad_spec_is_a_parser_error(tmp_path, capsys):
    import perfect_repeat_finder as prf
    fa = tmp_path / "x.fa"
    fa.write_text(">a\nACGTACGTACGTACGT\n")
    for spec in ("1-3:0,2:1", "junk", "7-:1"):
        with pytest.raises(SystemExit):
            prf.main(["-min", "1", "-max", "6", "--max-interruptions-by-motif-size", spec, str(fa)])
        assert "--max-interruptions-by-motif-size" in capsys.readouterr().err
    with pytest.raises(SystemExit):     # interval mode stays refused
        prf.main(["-min", "1", "-max", "6", "--max-interruptions-by-motif-size", "3-:1", "-i", "a:0-10", str(fa)])
    assert "--interval" in capsys.readouterr().err


def test_budgets_compose_with_the_scalar():
    import perfect_repeat_finder as prf
    import prf_native
    ns = argparse.Namespace
    assert prf._interruption_budgets(ns(min_motif_size=1, max_motif_size=4)) == (0, None)
    assert prf._interruption_budgets(ns(min_motif_size=1, max_motif_size=4, max_interruptions=2)) == (2, None)
    assert prf._interruption_budgets(ns(min_motif_size=2, max_motif_size=5, max_interruptions=2,
                                        max_interruptions_by_motif_size={1: 3, 2: 0, 4: 1, 40: 1})) == (2, [0, 2, 1, 2])
    assert prf._interruption_budgets(ns(min_motif_size=2, max_motif_size=4, max_interruptions_by_motif_size={3: 1})) == (0, [0, 1, 0])
    for bad in ({3: -1}, {3: 1.5}, [0, 1, 0]):
        with pytest.raises(ValueError):
            prf._interruption_budgets(ns(min_motif_size=2, max_motif_size=4, max_interruptions_by_motif_size=bad))
    with pytest.raises(ValueError):
        prf._interruption_budgets(ns(min_motif_size=2, max_motif_size=4, max_interruptions=-1, max_interruptions_by_motif_size={}))
    # Context.scan_interrupted's argument: a dict is filled by the scalar, a sequence names every k
    f = prf_native.interruption_budgets
    assert f(1, 3, 2, {2: 0}) == [2, 0, 2] and f(1, 3, 0, [0, 1, 3]) == [0, 1, 3] and f(1, 3, 1, (1, 1, 1)) == [1, 1, 1]
    for args in ((1, 3, 2, [0, 1, 3]), (1, 3, 0, [0, 1]), (1, 3, 0, {4: 1}), (1, 3, 0, [0, -1, 0]), (1, 3, 0, {2: True}), (3, 1, 0, {})):
        with pytest.raises(ValueError):
            f(*args)
    assert f(1, 3, 0, {4: 1, 2: 1}, ignore_other_k=True) == [0, 1, 0]


class _FakeContext:
    """Stands in for prf_native.Context: records which native scan a call reaches."""

    def __init__(self):
        self.calls = []

    def scan(self, seqs, kmin, kmax, min_repeats, min_span, *a, **kw):
        self.calls.append(("perfect", kmin, kmax))
        return [{"start": 0, "end": 9, "k": 3}], None

    def scan_interrupted(self, seqs, kmin, kmax, min_repeats, min_span, max_interruptions, **kw):
        self.calls.append(("interrupted", max_interruptions, kw.get("max_interruptions_by_k")))
        return [], None


def test_all_zero_dict_takes_the_perfect_path():
    import perfect_repeat_finder as prf
    seq = "CAGCAGCAGTT"
    base = dict(min_motif_size=1, max_motif_size=6, min_repeats=3, min_span=9)
    for extra in ({"max_interruptions_by_motif_size": {i: 0 for i in range(1, 50)}},                        # the reference's own tests
                  {"max_interruptions_by_motif_size": {i: 0 for i in range(1, 50)}, "max_interruptions": 0},
                  {"max_interruptions_by_motif_size": {i: 0 for i in range(1, 7)}, "max_interruptions": 2},   # every k named: 0
                  {"max_interruptions_by_motif_size": {9: 3}},                                                # no k of the range
                  {"max_interruptions_by_motif_size": {}}):
        ctx = _FakeContext()
        assert prf.detect_repeats(seq, argparse.Namespace(**base, **extra), context=ctx) == [(0, 9, "CAG")]
        assert ctx.calls == [("perfect", 1, 6)]
    # and with an interval, which the interrupted lane would refuse
    ctx = _FakeContext()
    fs = argparse.Namespace(**base, max_interruptions_by_motif_size={i: 0 for i in range(1, 50)}, interval_start_0based=0, interval_end=11)
    prf.detect_repeats(seq, fs, context=ctx)
    assert [c[0] for c in ctx.calls] == ["perfect"]


def test_a_budget_above_zero_takes_the_interrupted_lane_with_the_vector():
    import perfect_repeat_finder as prf
    base = dict(min_motif_size=1, max_motif_size=6, min_repeats=3, min_span=9)
    ctx = _FakeContext()
    prf.detect_repeats("CAGCAGCAGTT", argparse.Namespace(**base, max_interruptions_by_motif_size={3: 1, 4: 0}, max_interruptions=2), context=ctx)
    assert ctx.calls == [("interrupted", 0, [2, 2, 1, 0, 2, 2])]
    ctx = _FakeContext()
    prf.detect_repeats("CAGCAGCAGTT", argparse.Namespace(**base, max_interruptions_by_motif_size={6: 1}), context=ctx)
    assert ctx.calls == [("interrupted", 0, [0, 0, 0, 0, 0, 1])]
    ctx = _FakeContext()        # without the dict: the call of before
    prf.detect_repeats("CAGCAGCAGTT", argparse.Namespace(**base, max_interruptions=1), context=ctx)
    assert ctx.calls == [("interrupted", 1, None)]
    with pytest.raises(ValueError, match="at least 0"):
        prf.detect_repeats("CAGCAGCAGTT", argparse.Namespace(**base, max_interruptions_by_motif_size={3: -1}), context=_FakeContext())
    with pytest.raises(ValueError, match="interval mode"):
        prf.detect_repeats("CAGCAGCAGTT", argparse.Namespace(**base, max_interruptions_by_motif_size={3: 1}, interval_end=5),
                           context=_FakeContext())


# ---- the C ABI of prf_scan_interrupted_by_k (refusals are decided before the context is touched) ----

def _lib():
    import prf_native
    return prf_native, prf_native.load_library()


def _call(lib, pn, kmin, kmax, r, span, vec, chunk, seqs=(b"ACGTACGT",), stride=8):
    arr, _keep = pn._contig_array(list(seqs))
    hits, stats = pn._IHits(), pn.ScanStats()
    ctr = (ctypes.c_uint64 * 6)()
    by_k = None if vec is None else (ctypes.c_uint32 * len(vec))(*vec)
    return lib.prf_scan_interrupted_by_k(None, arr, len(seqs), kmin, kmax, r, span, by_k, stride, 1 << 10, chunk, ctypes.byref(hits),
                                         ctypes.byref(stats), ctr)


def test_entry_point_is_exported_and_the_abi_version_stays():
    pn, lib = _lib()
    assert hasattr(lib, "prf_scan_interrupted_by_k")
    assert "prf_scan_interrupted_by_k" in pn.EXPORTS and len(set(pn.EXPORTS)) == 42
    assert all(hasattr(lib, name) for name in pn.EXPORTS)
    assert lib.prf_abi_version() == 4


@pytest.mark.parametrize("args,code,word", [
    ((2, 6, 3, 9, None, 4096), "PRF_EINVAL", b"max_interruptions_by_k"),      # NULL vector
    ((2, 6, 3, 9, [0, 1, 1, 0, 2], 1), "PRF_EINVAL", b"chunk"),               # a chunk below the minimum
    ((2, 6, 1, 9, [0, 1, 1, 0, 2], 4096), "PRF_EUNSUPPORTED", b"min_repeats"),
    ((2, 65, 3, 9, [1] * 64, 4096), "PRF_EUNSUPPORTED", b"64"),               # kmax > 64
    ((6, 2, 3, 9, [1] * 5, 4096), "PRF_EINVAL", b""),                         # an empty range of motif sizes
    ((2, 6, 3, 9, [0, 1, 1, 0, 2], 4096), "PRF_EINVAL", b"NULL context"),     # valid parameters: the context is looked at last
    ((2, 6, 3, 9, [0] * 5, 0), "PRF_EINVAL", b"NULL context"),                # all budgets 0 and chunk 0 are valid too
])
def test_refusals(args, code, word):
    pn, lib = _lib()
    assert _call(lib, pn, *args) == getattr(pn, code)
    assert word in lib.prf_last_error()


def test_memo_stride_refusal_and_the_old_entry_points_refusal_of_zero():
    pn, lib = _lib()
    assert _call(lib, pn, 2, 6, 3, 9, [1] * 5, 4096, stride=6) == pn.PRF_EINVAL
    assert b"power of two" in lib.prf_last_error()
    arr, _keep = pn._contig_array([b"ACGTACGT"])
    hits, stats = pn._IHits(), pn.ScanStats()
    ctr = (ctypes.c_uint64 * 6)()
    for call in (lambda: lib.prf_scan_interrupted(None, arr, 1, 2, 6, 3, 9, 0, ctypes.byref(hits), ctypes.byref(stats)),
                 lambda: lib.prf_scan_interrupted_ex(None, arr, 1, 2, 6, 3, 9, 0, 8, 1 << 10, ctypes.byref(hits), ctypes.byref(stats), ctr),
                 lambda: lib.prf_scan_interrupted_chunked(None, arr, 1, 2, 6, 3, 9, 0, 8, 1 << 10, 4096, ctypes.byref(hits),
                                                          ctypes.byref(stats), ctr)):
        assert call() == pn.PRF_EINVAL
        assert lib.prf_last_error().startswith(b"max_interruptions is 0: prf_scan_interrupted serves max_interruptions >= 1")
