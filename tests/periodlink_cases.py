"""The planted junctions of tests/test_periodlink_cpu.py and tests/test_periodlink_gpu.py, built without a GPU: one short sequence
per case -- random flanks around a tandem repeat of a random unit of p letters, edited by a list of operations -- and the links the
case is there for.  What a case claims is asserted on the model's list of the whole band (check_claim), by the CPU test too, so a
chance match that spoils a case fails on the CPU.

Why an indel gives two links.  In a repeat of period p >= min_seed, d bases inserted at position `at` end the chain of line p at
cell at - p - 1; the cells t with t < at <= t + p form a DETOUR chain of p cells on line p + d; line p goes on at cell at + d.
So: X (line p) -> detour (shift +d, gap 0) -> Y (line p; shift -d, gap 0).  A deletion of d bases gives the detour on line p - d
(p - d cells, which must still make a seed) with the shifts -d and +d.  A chance match next to the breakpoint lengthens a run by a
cell or two: the gap stays 0 and the overlap grows, so the claims leave the overlap open unless the case plants it."""
import random


import periodlink_model as L

S, G, D = 10, 3, 4                                            # min_seed, max_gap, max_shift of the planted junctions, unless a case says otherwise
FLANK = 25
CHANGE = bytes.maketrans(b"ACGT", b"CGTA")


def _random(n, rng, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _unit(p, rng):
    """p random letters without a run of two equal ones (so that no homopolymer run lengthens a chain) whose last differs from the first."""
    out = bytearray()
    while len(out) < p:
        x = rng.choice(b"ACGT")
        if (out and x == out[-1]) or (len(out) == p - 1 and x == out[0]):
            continue
        out.append(x)
    return bytes(out)


def tandem(p, length, ops, seed, flank=FLANK):
    """flank + (a unit of p letters repeated to `length` letters, edited) + flank.  ops, applied from the last position to the
    first so that every `at` is a position of the unedited repeat:
      ("ins", at, d)        d letters in front of position at, none of which lengthens a run on the line in front or behind
      ("ins_same", at, r)   the r letters in front of `at` become one letter IN EVERY COPY of the unit, and one more of it is inserted
      ("del", at, d)        d letters from position at are left out
      ("sub", at, n)        n letters from position at are changed
      ("N", at, n)          the n letters from the phase of `at` are N in every copy of the unit"""
    rng = random.Random(seed)
    unit = bytearray(_unit(p, rng))
    for kind, at, n in ops:
        if kind == "ins_same":
            base = next(x for x in b"ACGT" if x not in (unit[(at - n - 1) % p], unit[at % p]))
            for q in range(at - n, at):
                unit[q % p] = base
        elif kind == "N":
            for q in range(at, at + n):
                unit[q % p] = ord("N")
    body = bytearray((bytes(unit) * (length // p + 1))[:length])
    for kind, at, n in sorted(ops, key=lambda op: -op[1]):
        if kind == "ins":
            junk = bytearray(_random(n, rng))
            # on line p the first inserted letter meets the unit's letter of phase `at` and ends the run in front; on the detour's
            # line the last one meets the letter of phase at - 1: both differ from the letters that would lengthen a run
            here, front = unit[at % p], unit[(at - 1) % p]
            junk[0] = next(x for x in b"ACGT" if x not in (here, front))
            junk[-1] = next(x for x in b"ACGT" if x not in (here, front, junk[0] if n > 1 else 0))
            body[at:at] = junk
        elif kind == "ins_same":
            body[at:at] = body[at - 1:at]
        elif kind == "del":
            del body[at:at + n]
        elif kind == "sub":
            body[at:at + n] = bytes(body[at:at + n]).translate(CHANGE)
    return _random(flank, rng) + bytes(body) + _random(flank, rng)


# name: (sequence, (min_seed, max_gap, max_shift), {n_matches: claim})
# claim: the links of the WHOLE band as [(k, shift, gap, overlap or None)], in the list's order (start, k)
def _both(claim):
    return {0: claim, 1: claim}


CASES = {
    "an insertion of 1": (tandem(20, 70, [("ins", 35, 1)], 1), (S, G, D), _both([(21, 1, 0, None), (20, -1, 0, None)])),
    "an insertion of max_shift": (tandem(20, 70, [("ins", 35, D)], 2), (S, G, D), _both([(20 + D, D, 0, None), (20, -D, 0, None)])),
    "an insertion of max_shift + 1": (tandem(20, 70, [("ins", 35, D + 1)], 3), (S, G, D), _both([])),
    "a deletion of 1": (tandem(20, 70, [("del", 35, 1)], 4), (S, G, D), _both([(19, -1, 0, None), (20, 1, 0, None)])),
    "a deletion of max_shift": (tandem(20, 70, [("del", 35, D)], 5), (S, G, D), _both([(20 - D, -D, 0, None), (20, D, 0, None)])),
    "a deletion of max_shift + 1": (tandem(20, 70, [("del", 35, D + 1)], 6), (S, G, D), _both([])),
    # the changed letters behind the insertion (changed first: equal positions keep the list's order) break the first cells of
    # the detour (t + p + 2 in them) and of the chain behind
    "a gap of exactly max_gap": (tandem(20, 70, [("sub", 35, G), ("ins", 35, 2)], 7), (S, G, D), _both([(22, 2, G, 0), (20, -2, G, 0)])),
    "a gap of max_gap + 1": (tandem(20, 70, [("sub", 35, G + 1), ("ins", 35, 2)], 8), (S, G, D), _both([])),
    "an overlap of ov = 15": (tandem(40, 140, [("ins_same", 70, 15)], 9), (16, G, D), _both([(41, 1, 0, 15), (40, -1, 0, 15)])),
    "an overlap of ov + 1 = 16": (tandem(40, 140, [("ins_same", 70, 16)], 10), (16, G, D), _both([])),
    "an overlap of ov = 16": (tandem(40, 140, [("ins_same", 70, 16)], 11), (20, G, D), _both([(41, 1, 0, 16), (40, -1, 0, 16)])),
    "an overlap of ov + 1 = 17": (tandem(40, 140, [("ins_same", 70, 17)], 12), (20, G, D), _both([])),
    "a shift of 32": (tandem(40, 140, [("ins", 70, 32)], 13), (S, G, 32), _both([(72, 32, 0, None), (40, -32, 0, None)])),
    "a shift of -32": (tandem(45, 180, [("del", 80, 32)], 14), (S, G, 32), _both([(13, -32, 0, None), (45, 32, 0, None)])),
    "a shift of 33": (tandem(40, 140, [("ins", 70, 33)], 15), (S, G, 32), _both([])),
    "max_gap = 0": (tandem(20, 70, [("ins", 35, 3)], 16), (S, 0, D), _both([(23, 3, 0, None), (20, -3, 0, None)])),
    # N N | N N around both breakpoints: letters like any other where N == N matches, four dead cells (> max_gap) where it does not
    "an N block next to the junction": (tandem(20, 70, [("N", 13, 4), ("ins", 35, 1)], 17), (S, G, D),
                                        {1: [(21, 1, 0, None), (20, -1, 0, None)], 0: []}),
    # p < min_seed: the insertion costs line p four cells (<= max_gap = 4 here), its chain runs over it, and so do those of lines 6 and 9
    # (their detours of 6 and 9 cells are no seeds); the heads on line 3 have no lines below 1 to look at (max_shift 8: the lanes
    # of s = 3 .. 8 idle).  The multiples 12, 15 and 18 are periods >= min_seed with a detour each; line 21 has 9 cells in front.
    "a period below min_seed": (tandem(3, 60, [("ins", 30, 1)], 18), (S, 4, 8),
                                _both([(19, 1, 0, None), (16, 1, 0, None), (13, 1, 0, None), (12, -1, 0, None), (15, -1, 0, None), (18, -1, 0, None)])),
    # from period 5 to period 3: X on line 5 ends 6 cells in front of the seam, Y on line 3 starts at it
    "a head on line 3": (tandem(5, 40, [], 19, flank=20)[:-20] + tandem(3, 45, [], 20, flank=20)[20:], (S, G, 8), _both([(3, -2, 3, None)])),
    # n = 16: Y is cells 1 .. 2 of line 13 = n - 3, X cells 0 .. 1 of line 11 (one cell of overlap).  Of Y's lanes s = -1 .. -4 the
    # lines 14 and 15 = n - 1 exist and hold no chain, the lines 16 and 17 do not exist; of X's, 12 .. 15 exist.  Line n - 1 has
    # one cell, cell 0, so it can hold neither side of a junction (t_s >= 1 + |s| or t_e <= -1 would be needed): what is pinned
    # is that a partner line at and beyond n - 1 changes nothing.  The two other chains (lines 3 and 6) have no candidate.
    "the partner line is n - 1 or does not exist": (b"CGCATCTACTTCGTGC", (2, 1, 4), _both([(13, 2, 0, 1)])),
}

# a dense band up to its last lines: two letters only, so that lines up to n - 2 hold seeds and the lanes of the lines n - 1
# (one cell) and beyond n - 1 (idle) are met.  No claim but the counts that tests/test_periodlink_cpu.py asserts.
DENSE = [(_random(48, random.Random(100 + k), b"AC"), (3, 2, 32)) for k in range(6)] + \
        [(_random(40, random.Random(200 + k), b"AC"), (2, 1, 8)) for k in range(6)]


def generated(count, seed=17):
    """Short sequences of two to four letters with planted repeats, to fill up a triple's links: (sequence, ...)."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        alphabet = (b"AC", b"ACG", b"ACGT")[k % 3]
        p = rng.randrange(8, 24)
        body = bytearray(_random(p, rng, alphabet) * rng.randrange(4, 7))
        for _ in range(rng.randrange(1, 4)):
            at = rng.randrange(p, len(body) - p)
            if rng.random() < 0.5:
                body[at:at] = _random(rng.randrange(1, 4), rng, alphabet)
            else:
                del body[at:at + rng.randrange(1, 4)]
        out.append(_random(rng.randrange(0, 9), rng, alphabet) + bytes(body) + _random(rng.randrange(0, 9), rng, alphabet))
    return out


def vntr(seed=5, p=24, copies=9, flank=60):
    """(sequence, start, end, indel): a repeat of period p with three indels far apart (+1, -2, +3), between random flanks."""
    length = p * copies
    ops = [("ins", 2 * p + 7, 1), ("del", 4 * p + 11, 2), ("ins", 7 * p - 5, 3)]
    seq = tandem(p, length, ops, seed, flank=flank)
    return seq, flank, flank + length + 1 - 2 + 3, 2 * (1 + 2 + 3)


def expected(name, n_matches):
    seq, params, _claims = CASES[name]
    return L.links(seq, 1, len(seq), *params, n_matches=n_matches)


def check_claim(name, links, n_matches):
    """What the case is there for, on the model's list of the whole band."""
    claim = CASES[name][2][n_matches]
    got = [(int(r["k"]), int(r["shift"]), int(r["gap"]), int(r["overlap"])) for r in links]
    assert len(got) == len(claim), (name, n_matches, got)
    for have, want in zip(got, claim):
        assert have[:3] == want[:3] and (want[3] is None or have[3] == want[3]), (name, n_matches, got)
