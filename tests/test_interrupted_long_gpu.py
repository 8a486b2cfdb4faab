"""GPU (-m gpu): interrupted repeats (csrc/scan_interrupted.hip, csrc/interrupted.cpp) against the reference's RepeatTracker at
3-40 kb (tests/golden/interrupted_long.jsonl.gz) through every engine setting, the one-lane engine's overflow paths, and the CPU
model (tests/interrupted_model.py) over the scope of DESIGN 9.3 at 100-300 kb."""
import random
from collections import defaultdict

import pytest

import interrupted_chunks_model as C
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


@pytest.fixture(scope="module")
def golden_long():
    return load_jsonl_gz("interrupted_long.jsonl.gz")


def _gpu_rows(ctx, seqs, kmin, kmax, r, span, m, **kw):
    """[[ (start, end, k, nmask), ... ] per sequence]."""
    out = ctx.scan_interrupted([s if isinstance(s, bytes) else s.encode() for s in seqs], kmin, kmax, r, span, m, **kw)
    per = [[] for _ in seqs]
    for row in out[0]:
        per[int(row["contig"])].append((int(row["start"]), int(row["end"]), int(row["k"]), int(row["nmask"])))
    return (per,) + tuple(out[1:])


def _settings(case):
    st = case["settings"]
    return st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], st["max_interruptions"]


def _motif_rows(case, rows):
    return [[a, b, M.motif_text(case["seq"].upper().encode(), a, k, mask)] for a, b, k, mask in rows]


def _engines():
    import prf_native
    return {"one_lane": dict(chunk=0),
            "chunk_1000": dict(chunk=1000),
            "chunk_4096": dict(chunk=4096),
            "library_default": dict(chunk=prf_native.INT_CHUNK),
            "one_lane_no_memo": dict(chunk=0, memo_stride=0, memo_slots=0),
            "one_lane_memo_8_2^20": dict(chunk=0, memo_stride=8, memo_slots=1 << 20),
            "one_lane_memo_1_7": dict(chunk=0, memo_stride=1, memo_slots=7),
            "chunk_1000_no_memo": dict(chunk=1000, memo_stride=0, memo_slots=0),
            "chunk_1000_memo_8_2^20": dict(chunk=1000, memo_stride=8, memo_slots=1 << 20),
            "chunk_1000_memo_1_7": dict(chunk=1000, memo_stride=1, memo_slots=7)}


@pytest.mark.parametrize("engine", ["one_lane", "chunk_1000", "chunk_4096", "library_default", "one_lane_no_memo", "one_lane_memo_8_2^20",
                                    "one_lane_memo_1_7", "chunk_1000_no_memo", "chunk_1000_memo_8_2^20", "chunk_1000_memo_1_7"])
def test_every_long_case_batched(ctx, golden_long, engine):
    """One call per setting of the fixture's palette and engine: the one-lane engine, chunks of 1000 (not a power of two) and
    4096, the library's default, and the memo settings (0, 0), (8, 2^20) and (1, 7) on the one-lane engine and on chunks."""
    kw = _engines()[engine]
    groups = defaultdict(list)
    for c in golden_long:
        groups[_settings(c)].append(c)
    assert len(groups) <= 24
    bad = []
    for settings, group in groups.items():
        seqs = [c["seq"] for c in group]
        per, stats, ctr = _gpu_rows(ctx, seqs, *settings, counters=True, **kw)
        assert stats.path == 3 and stats.sorted_on_device == 1
        assert ctr["lanes"] == C.lane_count(seqs, settings[0], settings[1], kw["chunk"])
        if kw.get("memo_stride") == 0:
            assert ctr["hits"] == 0 and ctr["lookups"] == 0
        for c, rows in zip(group, per):
            if _motif_rows(c, rows) != c["rows"]:
                bad.append((c["tag"], len(c["seq"]), settings))
    assert not bad, f"{engine}: {len(bad)} of {len(golden_long)} cases differ: {bad[:5]}"


def test_overflowing_cases_alone_on_the_one_lane_engine(ctx, golden_long):
    """The low-complexity cases one by one with chunk 0.  The one-lane engine gives a lane len / 4 + 16 candidate slots and
    len / 4 + 64 episode outcomes (csrc/interrupted.cpp, size_walk_room).  A case with more candidates on some k takes the
    count-only path and walks a second time with the exact room; the statistics have no launch count of the walk alone, but
    `n_launches` is the sum over the stages and each walk is one launch, so an overflowing case shows exactly one launch more than
    a case that fits.  The `episodes` counter is the number of recorded episodes of the last walk: at most the episode room per
    lane."""
    seen_over = seen_fit = 0
    launches = {False: set(), True: set()}
    for c in golden_long:
        if c["tag"] != "low_complexity":
            continue
        kmin, kmax, r, span, m = _settings(c)
        s, _head = M.trim(c["seq"])
        n = len(c["seq"])
        walks = [M.walk(s, k, r, span, m, stride=8, slots=1 << 16) for k in range(kmin, kmax + 1)]
        over = any(len(w.cands) > n // 4 + 16 for w in walks)
        (rows,), stats, ctr = _gpu_rows(ctx, [c["seq"]], kmin, kmax, r, span, m, chunk=0, counters=True)
        assert _motif_rows(c, rows) == c["rows"], (n, _settings(c))
        assert stats.path == 3 and stats.n_hits == len(c["rows"]) > 0
        print(f"{n} positions, {_settings(c)}: most candidates {max(len(w.cands) for w in walks)}, most episodes "
              f"{max(len(w.landings) + 1 for w in walks)}, n_launches {stats.n_launches}, recorded episodes {ctr['episodes']}")
        launches[over].add(int(stats.n_launches))
        assert stats.n_candidates == sum(len(w.cands) for w in walks)
        assert ctr["episodes"] == sum(min(len(w.landings) + 1, n // 4 + 64) for w in walks)
        seen_over += over and any(len(w.landings) + 1 > n // 4 + 64 for w in walks)
        seen_fit += not over
    assert seen_over >= 1 and seen_fit >= 1
    assert len(launches[False]) == 1 and launches[True] == {n + 1 for n in launches[False]}, launches


def _sweep_seq(n, seed, alphabet, unit_lens, copies):
    rng = random.Random(seed)
    s = bytearray(rng.choice(alphabet) for _ in range(n))
    for _ in range(max(1, n // 2000)):             # planted interrupted repeats
        unit = bytes(rng.choice(alphabet) for _ in range(rng.randint(*unit_lens)))
        rep = bytearray(unit * rng.randint(*copies))
        for _ in range(rng.randint(0, 4)):
            rep[rng.randrange(len(rep))] = rng.choice(alphabet)
        if len(rep) < n:
            p = rng.randrange(n - len(rep))
            s[p:p + len(rep)] = rep
    return bytes(s)


# (lengths, alphabet, planted unit lengths, copies), (kmin, kmax, r, span, m), chunks: every setting the scope of DESIGN 9.3 names
# beyond the fixtures' corner appears at least once -- k 7-12, 16-64 and 60-64; m 4, 8 and 64; r 2 and 5; span 1 and 100; two letters
SWEEP = [
    pytest.param(((200_000, 3_000, 40), b"ACGT", (5, 12), (3, 20)), (7, 12, 2, 1, 4), (4096, 30_000), id="k7-12_m4_r2_span1"),
    pytest.param(((100_000, 5_000, 300), b"ACGT", (16, 64), (5, 12)), (16, 64, 5, 1, 2), (4096, 30_000), id="k16-64_m2_r5_span1"),
    pytest.param(((150_000, 2_000), b"ACGT", (60, 64), (2, 6)), (60, 64, 2, 100, 3), (1000, 1 << 16), id="k60-64_m3_r2_span100"),
    pytest.param(((100_000, 20_000, 1_000), b"AC", (2, 6), (3, 20)), (1, 6, 3, 9, 2), (4096, 30_000), id="two_letters_k1-6_m2"),
    pytest.param(((120_000, 7_000), b"ACGT", (2, 8), (5, 30)), (2, 8, 5, 100, 8), (1000, 50_000), id="k2-8_m8_r5_span100"),
    pytest.param(((100_000, 900), b"AT", (7, 12), (2, 10)), (7, 12, 2, 100, 64), (4096, 1 << 17), id="two_letters_k7-12_m64_r2_span100"),
]


@pytest.mark.parametrize("shape,settings,chunks", SWEEP)
def test_scope_sweep_equals_model(ctx, shape, settings, chunks):
    lengths, alphabet, unit_lens, copies = shape
    seqs = [_sweep_seq(n, 100 + i, alphabet, unit_lens, copies) for i, n in enumerate(lengths)] + [b"", b"NN"]
    seqs[1] = b"nn" + seqs[1].lower() + b"N"
    kmin, kmax, r, span, m = settings
    want = [[(a, b, k, mask) for a, b, k, mask, _motif in M.detect(s, kmin, kmax, r, span, m, stride=8, slots=1 << 20)] for s in seqs]
    assert want[0] and (len(want[0]) > 5 or m >= kmax)      # (k <= m: one row per k at most)
    for chunk in (0,) + chunks:
        got, stats, ctr = _gpu_rows(ctx, seqs, kmin, kmax, r, span, m, chunk=chunk, counters=True)
        assert stats.path == 3
        assert ctr["lanes"] == C.lane_count(seqs, kmin, kmax, chunk), chunk
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (chunk, i, len(g), len(w), [x for x in g if x not in w][:3], [x for x in w if x not in g][:3])
