#!/usr/bin/env python3
"""Write tests/golden/interrupted.jsonl.gz: interrupted-repeat cases run through the REFERENCE's RepeatTracker.

The reference has no driver for RepeatTracker (its perfect_repeat_finder.py drives PerfectRepeatTracker only), so this tool
runs the driver the project pins: upper-case, N-trimming of the whole sequence (reference perfect_repeat_finder.py
:35-46), one RepeatTracker(k, min_repeats, min_span, max_interruptions, seq, out) per k = kmin .. kmax in ascending order with
ONE shared dict, `while t.advance(): pass; t.done()`, rows = sorted(out.items()) shifted by the trimmed head.

    python3 tools/gen_interrupted_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--cases 3200] [--seed 9]
    python3 tools/gen_interrupted_golden.py --reference PATH_TO_REFERENCE_CHECKOUT --long [--seed 17] [--jobs 4]
    python3 tools/gen_interrupted_golden.py --reference PATH_TO_REFERENCE_CHECKOUT --by-k [--seed 31] [--jobs 4]

--long writes tests/golden/interrupted_long.jsonl.gz instead: a few dozen cases of 3-40 kb (the short fixture stops at 600
positions) in the same format and through the same driver, from one seed (long_cases() lists them): random ACGT of 5-40 kb with
and without planted interrupted repeats, 20 kb of two- and three-letter sequence, planted units of 16-64 under k 16-64 and 60-64
(one unit of exactly 64 with its interruption at phase 63), max_interruptions 4, 6, 8 and 64, min_repeats 2 and 5, min_span 1 and
100, and N blocks, N ends, lower case and IUPAC letters at 10 kb.  The reference rows take minutes (--jobs processes; the bytes do
not depend on it).  Before it writes, the tool checks with the project's model (tests/interrupted_model.py) that one (sequence, k)
of a low-complexity case lists more candidates than len / 4 + 16 and one has more episodes than len / 4 + 64 (the room the one-lane
engine gives a lane), and that the 64-long unit is reported with phase 63 varying.

--by-k writes tests/golden/interrupted_by_k.jsonl.gz: a budget per motif size, RepeatTracker(k, ..., m_k, ...) in the
same driver.  800 cases of at most 600 positions from make_case(), each with a vector of budgets 0-3 from a small palette per range
of motif sizes (at least a third of all budgets are 0, some motif sizes have k <= m_k), and 8 cases of 5-10 kb (by_k_long_cases()):
random ACGT with planted units, two letters, an N block with lower case, and units of 16-64 under k 16-64 with budgets 0 and 2
alternating.  At most 40 distinct (settings, vector), so that a test can hand all cases of one to one call.  Before it writes, the
tool checks with the project's model that at least half of the cases have rows that differ from those under the uniform budget
max(m_k): otherwise the fixture would show nothing.  The settings of these cases hold "max_interruptions_by_k", a list with one
entry per motif size, in place of "max_interruptions".

Each line: {"tag", "seq", "settings": {min_motif_size, max_motif_size, min_repeats, min_span, max_interruptions},
"rows": [[start, end, motif], ...]} -- the motif with N at the phases that were allowed to vary.
"""
import argparse
import gzip
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "interrupted.jsonl.gz")
LONG_OUT = os.path.join(ROOT, "tests", "golden", "interrupted_long.jsonl.gz")
BY_K_OUT = os.path.join(ROOT, "tests", "golden", "interrupted_by_k.jsonl.gz")


def reference_rows(RepeatTracker, seq, kmin, kmax, min_repeats, min_span, max_interruptions):
    """max_interruptions: one number, or a list with the budget of every motif size kmin .. kmax."""
    s = seq.upper()
    lo, hi = 0, len(s)
    while lo < hi and s[lo] == "N":
        lo += 1
    while hi > lo and s[hi - 1] == "N":
        hi -= 1
    s = s[lo:hi]
    out = {}
    for k in range(kmin, kmax + 1):
        m = max_interruptions[k - kmin] if isinstance(max_interruptions, list) else max_interruptions
        t = RepeatTracker(motif_size=k, min_repeats=min_repeats, min_span=min_span, max_interruptions=m,
                          input_sequence=s, output_intervals=out)
        while t.advance():
            pass
        t.done()
    return [[a + lo, b + lo, m] for (a, b), m in sorted(out.items())]


def planted(rng, unit_len, copies, n_changes, alphabet="ACGT"):
    unit = "".join(rng.choice(alphabet) for _ in range(unit_len))
    rep = list(unit * copies)
    for _ in range(n_changes):
        if rep:
            rep[rng.randrange(len(rep))] = rng.choice(alphabet)
    return "".join(rep)


def random_seq(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


# settings come from a small palette, so that a test can hand all cases of one setting to one call
SMALL_K = [(1, 6), (2, 8)]
LARGE_K = [(16, 64)]
THRESHOLDS = [(2, 5), (3, 9)]


def make_case(rng, i):
    kind = ["random", "planted", "homopolymer", "n_iupac", "lower", "large_k", "absorbing", "n_ends", "dense"][i % 9]
    m = rng.randint(1, 3)
    kmin, kmax = rng.choice(LARGE_K if kind == "large_k" else SMALL_K)
    r, span = rng.choice(THRESHOLDS)
    if kind == "random":                      # back-jumps and the stale phase set on plain random sequence
        seq = random_seq(rng, rng.choice([50, 200, 600]), "ACGT")
    elif kind == "planted":                   # interrupted repeats in random flanks: dict precedence, the previous-output rule
        parts = [random_seq(rng, rng.randint(0, 40), "ACGT")]
        for _ in range(rng.randint(1, 4)):
            parts.append(planted(rng, rng.randint(1, 8), rng.randint(2, 14), rng.randint(0, 4)))
            parts.append(random_seq(rng, rng.randint(0, 30), "ACGT"))
        seq = "".join(parts)
    elif kind == "homopolymer":               # AAAC-like units: motifs that are a homopolymer once the varying phases are N
        base = rng.choice("ACGT")
        unit = [base] * rng.randint(2, 7)
        unit[rng.randrange(len(unit))] = rng.choice("ACGT")
        seq = random_seq(rng, rng.randint(0, 20), "ACGT") + "".join(unit) * rng.randint(2, 10) + random_seq(rng, rng.randint(0, 20), "ACGT")
    elif kind == "n_iupac":                   # N inside runs (N == N is a match here) and other letters as ordinary symbols
        seq = random_seq(rng, rng.choice([40, 150, 400]), rng.choice(["ACGTN", "ACGTRY", "ACNNNGT", "ACGTWSKMN"]))
        if rng.random() < 0.5:
            p = rng.randrange(len(seq) + 1)
            seq = seq[:p] + planted(rng, rng.randint(1, 6), rng.randint(2, 8), rng.randint(0, 2), "ACGTN") + seq[p:]
    elif kind == "lower":                     # lower case (upper-cased by the driver)
        seq = random_seq(rng, rng.randint(0, 30), "ACGTacgtn") + planted(rng, rng.randint(1, 6), rng.randint(2, 10), rng.randint(0, 3), "acgtACGT") \
            + random_seq(rng, rng.randint(0, 30), "acgtACGT")
    elif kind == "large_k":                   # motif sizes up to 64, m = 1-3
        k = rng.randint(16, 64)
        seq = random_seq(rng, rng.randint(0, 30), "ACGT") + planted(rng, k, rng.randint(2, 4), rng.randint(0, 5)) + random_seq(rng, rng.randint(0, 30), "ACGT")
    elif kind == "absorbing":                 # k <= m: every phase may vary, a run never ends
        seq = random_seq(rng, rng.randint(0, 200), rng.choice(["ACGT", "AC", "ACGTN"]))
    elif kind == "n_ends":                    # N (either case) at both ends: the trimmed head shifts the rows
        seq = "N" * rng.randint(0, 12) + "n" * rng.randint(0, 3) + planted(rng, rng.randint(1, 5), rng.randint(2, 10), rng.randint(0, 3)) \
            + random_seq(rng, rng.randint(0, 40), "ACGTN") + "n" * rng.randint(0, 3) + "N" * rng.randint(0, 12)
        if rng.random() < 0.05:
            seq = "N" * rng.randint(0, 20)
    else:                                     # low-complexity sequence: many overlapping candidates per k
        seq = random_seq(rng, rng.choice([100, 300]), rng.choice(["AC", "AAC", "ACG", "AT"]))
    return {"tag": kind, "seq": seq,
            "settings": {"min_motif_size": kmin, "max_motif_size": kmax, "min_repeats": r, "min_span": span, "max_interruptions": m}}


# ---- the long fixture (--long) ----

def plant_into(rng, s, count, unit_lens, copies, changes, alphabet="ACGT"):
    """Overwrite `count` stretches of the list s with planted interrupted repeats."""
    for _ in range(count):
        rep = planted(rng, rng.randint(*unit_lens), rng.randint(*copies), rng.randint(*changes), alphabet)
        p = rng.randrange(len(s) - len(rep))
        s[p:p + len(rep)] = rep


def unit64_phase63(rng):
    """Four copies of a 64-long unit, the third with its last base changed, behind eight bases that match nothing 64 further on
    (no run of k = 64 starts early): the mismatch comes at run 127, phase 63."""
    unit = random_seq(rng, 64, "ACGT")

    def other(ch):
        return "ACGT"["ACGT".index(ch) ^ 1]
    return "".join(other(ch) for ch in unit[56:]) + unit * 2 + unit[:63] + other(unit[63]) + unit


def long_cases(seed):
    """[{"tag", "seq", "settings"}]: the settings come from a small palette (17 of them), so that a test can hand all cases of
    one setting to one call."""
    rng = random.Random(seed)
    cases = []

    def add(tag, seq, kmin, kmax, r, span, m):
        cases.append({"tag": tag, "seq": seq, "settings": {"min_motif_size": kmin, "max_motif_size": kmax, "min_repeats": r,
                                                          "min_span": span, "max_interruptions": m}})

    def acgt(n, plant, unit_lens=(1, 8), copies=(3, 20), changes=(0, 3)):
        s = list(random_seq(rng, n, "ACGT"))
        if plant:
            plant_into(rng, s, n // 1000, unit_lens, copies, changes)
        return "".join(s)

    a, b, c, d = (1, 6, 3, 9, 1), (2, 8, 2, 5, 2), (2, 8, 3, 9, 2), (1, 6, 2, 5, 3)
    for tag, n, plant, st in (("random", 5_000, False, a), ("random_planted", 5_000, True, b), ("random", 5_000, False, b),
                              ("random", 10_000, False, c), ("random_planted", 10_000, True, d), ("random", 20_000, False, a),
                              ("random_planted", 20_000, True, a), ("random_planted", 20_000, True, c), ("random", 20_000, False, d),
                              ("random_planted", 40_000, True, a)):
        add(tag, acgt(n, plant), *st)
    # two and three letters: nearly every position closes a candidate (the one-lane engine's candidate and episode room overflow)
    for alphabet, st in (("AC", (1, 6, 2, 5, 1)), ("AT", (1, 6, 2, 5, 1)), ("AAC", (1, 6, 2, 5, 1)), ("AC", (1, 6, 3, 9, 2))):
        add("low_complexity", random_seq(rng, 20_000, alphabet), *st)
    # On random two-letter sequence a quarter of the positions are boundaries of k = 2 (a mismatch right behind a match), and each
    # becomes an episode with a candidate: len / 4 on average, which is the room.  Take the first of the draws that lies far enough
    # above the average to overflow both (about one in forty does).
    for t in range(4000):
        seq = random_seq(random.Random(seed * 4000 + t), 20_000, "AC")
        if sum(seq[q - 1] == seq[q + 1] and seq[q] != seq[q + 2] for q in range(1, len(seq) - 2)) > len(seq) // 4 + 80:
            break
    else:
        raise RuntimeError("none of 4000 draws of 20 kb of AC has more than len / 4 + 80 boundaries of k = 2")
    add("low_complexity", seq, 1, 6, 2, 5, 1)
    # planted units of 16-64 under large k
    for n, st, with64 in ((3_000, (16, 64, 2, 5, 1), True), (5_000, (16, 64, 3, 9, 2), False), (10_000, (16, 64, 2, 5, 3), False),
                          (5_000, (60, 64, 2, 5, 1), True), (3_000, (60, 64, 3, 9, 3), True), (10_000, (60, 64, 2, 5, 2), True)):
        s = list(random_seq(rng, n, "ACGT"))
        plant_into(rng, s, n // 500, (max(16, st[0]), 64), (2, 5), (0, 4))
        if with64:
            rep = unit64_phase63(rng)
            p = rng.randrange(n - len(rep))
            s[p:p + len(rep)] = rep
        add("large_k_unit64" if with64 else "large_k", "".join(s), *st)
    # more interruptions than the short fixture has (m >= k for every k of the range in the last two)
    for n, m, r, span in ((5_000, 4, 3, 9), (5_000, 6, 3, 9), (10_000, 8, 2, 5), (5_000, 64, 3, 9)):
        add("many_interruptions", acgt(n, True, changes=(0, 8)), 1, 8, r, span, m)
    # thresholds: r 2 and 5, span 1, and a span that binds instead of r * k
    for n, st in ((10_000, (2, 8, 2, 1, 1)), (5_000, (2, 8, 5, 1, 2)), (10_000, (2, 8, 3, 100, 2)), (5_000, (1, 6, 5, 100, 1)),
                  (5_000, (1, 6, 2, 100, 2))):
        add("thresholds", acgt(n, True, copies=(3, 60)), *st)
    # N inside and at both ends, lower case, IUPAC letters (ordinary symbols for this tracker), at 10 kb
    body = acgt(10_000, True)
    add("n_block", "N" * 40 + body[:4_000] + "N" * 300 + body[4_300:9_900] + "N" * 25, *a)
    body = acgt(10_000, True).lower()
    add("lower_n_block", body[:7_000] + "n" * 500 + body[7_500:], *b)
    s = list(acgt(10_000, True))
    for _ in range(400):
        s[rng.randrange(len(s))] = rng.choice("RYKMSWBDHVN")
    plant_into(rng, s, 5, (1, 6), (3, 12), (0, 2), "ACGTRYN")
    add("iupac", "".join(s), *c)
    s = list(acgt(10_000, True))
    for _ in range(200):
        s[rng.randrange(len(s))] = rng.choice("RYKMSWNacgtn")
    s[2_000:2_150] = "N" * 150
    add("n_ends_lower_iupac", "nnNN" + "".join(s) + "Nn", *d)
    return cases


def check_long_cases(cases):
    """What the fixture is for, checked with the project's model before the reference runs."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import interrupted_model as M
    over_cands = over_eps = phase63 = False
    for c in cases:
        st = c["settings"]
        if c["tag"] == "low_complexity":
            s, _head = M.trim(c["seq"])
            for k in range(st["min_motif_size"], st["max_motif_size"] + 1):
                w = M.walk(s, k, st["min_repeats"], st["min_span"], st["max_interruptions"], stride=8, slots=1 << 16)
                over_cands |= len(w.cands) > len(c["seq"]) // 4 + 16
                over_eps |= len(w.landings) + 1 > len(c["seq"]) // 4 + 64
        if c["tag"] == "large_k_unit64":
            rows = M.detect(c["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], st["max_interruptions"],
                            stride=8, slots=1 << 16)
            phase63 |= any(k == 64 and (mask >> 63) & 1 for _a, _b, k, mask, _motif in rows)
    assert phase63, "no case reports a k = 64 row with phase 63 varying"
    assert over_cands, "no (sequence, k) of a low-complexity case has more than len / 4 + 16 candidates"
    assert over_eps, "no (sequence, k) of a low-complexity case has more than len / 4 + 64 episodes"


# ---- a budget per motif size (--by-k) ----

def by_k_palette(rng):
    """{(kmin, kmax): [vector, ...]}: four vectors per small range, two for 16-64, budgets 0-3 with 0 twice as likely as each
    other value; the first vector of every small range is the staircase (0 for k 1-2, 1 for 3-4, 2 above), and every range has a
    vector with some k <= m_k."""
    pal = {}
    for kmin, kmax in SMALL_K + LARGE_K:
        nk = kmax - kmin + 1
        want = 2 if (kmin, kmax) in LARGE_K else 4
        vs = [] if (kmin, kmax) in LARGE_K else [[0 if k <= 2 else 1 if k <= 4 else 2 for k in range(kmin, kmax + 1)]]
        while len(vs) < want:
            v = [rng.choice([0, 0, 1, 2, 3]) for _ in range(nk)]
            absorbing = any(kmin + j <= m for j, m in enumerate(v))
            if v in vs or 3 * v.count(0) < nk or not any(v) or (kmin <= 3 and len(vs) == 1 and not absorbing):
                continue
            vs.append(v)
        pal[(kmin, kmax)] = vs
    return pal


def by_k_long_cases(rng, pal):
    cases = []

    def add(tag, seq, kmin, kmax, r, span, vec):
        cases.append({"tag": tag, "seq": seq, "settings": {"min_motif_size": kmin, "max_motif_size": kmax, "min_repeats": r,
                                                          "min_span": span, "max_interruptions_by_k": list(vec)}})

    def acgt(n):
        s = list(random_seq(rng, n, "ACGT"))
        plant_into(rng, s, n // 500, (1, 8), (3, 20), (0, 3))
        return "".join(s)

    stairs = pal[(1, 6)][0]
    add("random_planted", acgt(8_000), 1, 6, 3, 9, stairs)
    add("random_planted", acgt(10_000), 2, 8, 2, 5, pal[(2, 8)][1])
    add("random_planted", acgt(5_000), 1, 6, 2, 5, pal[(1, 6)][1])
    add("random_planted", acgt(10_000), 1, 6, 3, 9, [1, 2, 0, 0, 3, 0])       # k 1 and 2 absorb (k <= m_k), 3, 4 and 6 may not vary
    add("two_letters", random_seq(rng, 5_000, "AC"), 1, 6, 2, 5, stairs)
    add("two_letters", random_seq(rng, 6_000, "AT"), 2, 8, 3, 9, pal[(2, 8)][0])
    body = acgt(10_000)
    add("n_block_lower", "NN" + body[:4_000] + "N" * 300 + body[4_300:7_000].lower() + "n" * 40 + body[7_040:] + "N" * 7, 1, 6, 3, 9, stairs)
    s = list(random_seq(rng, 5_000, "ACGT"))
    plant_into(rng, s, 12, (16, 64), (2, 5), (0, 4))
    add("large_k_alternating", "".join(s), 16, 64, 2, 5, [0 if k % 2 == 0 else 2 for k in range(16, 65)])
    return cases


def by_k_cases(seed, n_short):
    rng = random.Random(seed)
    pal = by_k_palette(rng)
    cases = []
    for i in range(n_short):
        case = make_case(rng, i)
        st = case["settings"]
        del st["max_interruptions"]
        st["max_interruptions_by_k"] = list(rng.choice(pal[(st["min_motif_size"], st["max_motif_size"])]))
        cases.append(case)
    return cases + by_k_long_cases(rng, pal)


def check_by_k_cases(cases):
    """What the fixture is for, checked with the project's model before the reference runs."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import interrupted_by_k_model as K
    import interrupted_model as M
    groups = {json.dumps(c["settings"], sort_keys=True) for c in cases}
    assert len(groups) <= 40, f"{len(groups)} distinct (settings, vector)"
    budgets = [(c["settings"]["min_motif_size"] + j, m) for c in cases for j, m in enumerate(c["settings"]["max_interruptions_by_k"])]
    assert all(0 <= m <= 3 for _k, m in budgets)
    assert 3 * sum(m == 0 for _k, m in budgets) >= len(budgets), "fewer than a third of the budgets are 0"
    assert sum(k <= m for k, m in budgets) > len(cases) // 20, "hardly any motif size with k <= m_k"
    assert sum(5_000 <= len(c["seq"]) <= 10_400 for c in cases) == 8 and all(len(c["seq"]) <= 600 or len(c["seq"]) >= 5_000 for c in cases)
    differ = 0
    for c in cases:
        st = c["settings"]
        p = (c["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"])
        vec = st["max_interruptions_by_k"]
        differ += K.detect(*p, vec, stride=8, slots=1 << 16) != M.detect(*p, max(vec), stride=8, slots=1 << 16)
    assert 2 * differ >= len(cases), f"only {differ} of {len(cases)} cases differ from the uniform budget max(m_k)"
    return differ, len(groups)


def _by_k_rows(case):
    st = case["settings"]
    return reference_rows(_TRACKER, case["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"],
                          st["max_interruptions_by_k"])


def write_by_k(RepeatTracker, seed, n_short, out, jobs):
    global _TRACKER
    import multiprocessing
    _TRACKER = RepeatTracker
    cases = by_k_cases(seed, n_short)
    differ, groups = check_by_k_cases(cases)
    order = sorted(range(len(cases)), key=lambda i: -len(cases[i]["seq"]))      # the long ones first
    if jobs > 1:
        with multiprocessing.get_context("fork").Pool(jobs) as pool:
            rows = pool.map(_by_k_rows, [cases[i] for i in order], chunksize=1)
    else:
        rows = [_by_k_rows(cases[i]) for i in order]
    for i, r in zip(order, rows):
        cases[i]["rows"] = r
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        for case in cases:
            f.write((json.dumps(case, separators=(",", ":")) + "\n").encode())
    size = os.path.getsize(out)
    assert size < os.path.getsize(LONG_OUT), f"{size} bytes: not below interrupted_long.jsonl.gz"
    print(f"wrote {len(cases)} cases ({groups} distinct settings, {differ} differ from the uniform budget max(m_k)) to {out} ({size} bytes)")


_TRACKER = None


def _long_rows(case):
    st = case["settings"]
    return reference_rows(_TRACKER, case["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"],
                          st["max_interruptions"])


def write_long(RepeatTracker, seed, out, jobs):
    global _TRACKER
    import multiprocessing
    _TRACKER = RepeatTracker
    cases = long_cases(seed)
    check_long_cases(cases)
    if jobs > 1:
        with multiprocessing.get_context("fork").Pool(jobs) as pool:
            rows = pool.map(_long_rows, cases, chunksize=1)
    else:
        rows = [_long_rows(c) for c in cases]
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        for case, r in zip(cases, rows):
            case["rows"] = r
            f.write((json.dumps(case, separators=(",", ":")) + "\n").encode())
    print(f"wrote {len(cases)} cases to {out} ({os.path.getsize(out)} bytes)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds utils/repeat_tracker.py)")
    ap.add_argument("--cases", type=int, default=None, help="default: 3200, with --by-k 800 (short cases)")
    ap.add_argument("--seed", type=int, default=None, help="default: 9, with --long 17, with --by-k 31")
    ap.add_argument("--out", default=None)
    ap.add_argument("--long", action="store_true", help="write the long fixture (interrupted_long.jsonl.gz) instead")
    ap.add_argument("--by-k", action="store_true", help="write the fixture with a budget per motif size (interrupted_by_k.jsonl.gz) instead")
    ap.add_argument("--jobs", type=int, default=4, help="--long, --by-k: processes that run the reference")
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils.repeat_tracker import RepeatTracker
    if args.long:
        write_long(RepeatTracker, 17 if args.seed is None else args.seed, args.out or LONG_OUT, args.jobs)
        return
    if args.by_k:
        write_by_k(RepeatTracker, 31 if args.seed is None else args.seed, 800 if args.cases is None else args.cases,
                   args.out or BY_K_OUT, args.jobs)
        return
    args.seed = 9 if args.seed is None else args.seed
    args.cases = 3200 if args.cases is None else args.cases
    args.out = args.out or OUT
    rng = random.Random(args.seed)
    with gzip.open(args.out, "wt") as f:
        for i in range(args.cases):
            case = make_case(rng, i)
            st = case["settings"]
            case["rows"] = reference_rows(RepeatTracker, case["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"],
                                          st["min_span"], st["max_interruptions"])
            f.write(json.dumps(case, separators=(",", ":")) + "\n")
    print(f"wrote {args.cases} cases to {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
