"""Planted gapped repeats for the tests of the consensus over phased segments, shared by the CPU and the GPU file: a
motif of period P x 30 copies with sparse substitutions between random flanks, with ONE insertion, ONE deletion, or one of each at
least 3 P apart; and a pair of indels closer than P.  Inserted bases are lower case, so a test can see where they went."""
import random

COPIES, FLANK, SUBSTITUTIONS = 30, 40, 4
MAX_GAP, MAX_SHIFT = 8, 4
MIN_SEED = {7: 5, 17: 12, 40: 12}              # a detour line holds about P cells: the seed must fit


def primitive(motif):
    return not any(len(motif) % d == 0 and motif[:d] * (len(motif) // d) == motif for d in range(1, len(motif)))


def plant(period, edits, seed):
    """(motif, sequence): edits are (copy, 'I' or 'D', d[, offset]), at `offset` (default: the middle) of that copy of the motif."""
    rng = random.Random(seed)
    motif = ""
    while not motif or not primitive(motif):
        motif = "".join(rng.choice("ACGT") for _ in range(period))
    body = list(motif * COPIES)
    for _ in range(SUBSTITUTIONS):
        at = rng.randrange(len(body))
        body[at] = rng.choice([c for c in "ACGT" if c != body[at]])
    for copy, kind, d, *where in sorted(edits, reverse=True):
        at = copy * period + (where[0] if where else period // 2)
        if kind == "I":
            body[at:at] = [rng.choice("acgt") for _ in range(d)]
        else:
            del body[at:at + d]
    left, right = ("".join(rng.choice("ACGT") for _ in range(FLANK)) for _ in range(2))
    return motif, left + "".join(body) + right


EDITS = {"ins": lambda d: [(12, "I", d)], "del": lambda d: [(12, "D", d)], "both": lambda d: [(8, "I", d), (20, "D", d)]}
# the seed of every (P, d, kind): the first for which the models of DESIGN 16 and 17 give ONE group of period P over the whole
# body whose detours are isolated (one chain Y with len <= k between two chains of line P); test_phased_cpu.py confirms that
# before it checks anything else.  A detour chain that chance matches extend beyond its line's k is NOT isolated by the rule, and
# an inserted base that happens to equal the base one period away is taken into the neighbouring chain: the seeds also avoid that
# (the chains decide what a segment is, and they cannot tell such a base from a copy's).
SEEDS = {(7, 1, "ins"): 11, (7, 1, "del"): 18, (7, 1, "both"): 19, (7, 2, "ins"): 1, (7, 2, "del"): 11, (7, 2, "both"): 113,
         (7, 3, "ins"): 1, (7, 3, "del"): 60, (7, 3, "both"): 2, (17, 1, "ins"): 1, (17, 1, "del"): 1, (17, 1, "both"): 1,
         (17, 2, "ins"): 1, (17, 2, "del"): 1, (17, 2, "both"): 1, (17, 3, "ins"): 3, (17, 3, "del"): 3, (17, 3, "both"): 8,
         (40, 1, "ins"): 1, (40, 1, "del"): 3, (40, 1, "both"): 12, (40, 2, "ins"): 3, (40, 2, "del"): 2, (40, 2, "both"): 4,
         (40, 3, "ins"): 3, (40, 3, "del"): 2, (40, 3, "both"): 4}
CLOSE_SEED = 1


def body_group(groups, period, n):
    """The index of the one group of `period` that covers the planted body of a sequence of n letters (to within a copy)."""
    found = [at for at, g in enumerate(groups) if g["period"] == period and g["start"] <= FLANK + period and g["end"] >= n - FLANK - period]
    assert len(found) == 1, found
    return found[0]


def planted(period, d, kind):
    return plant(period, EDITS[kind](d), SEEDS[(period, d, kind)])


def close_pair(period, seed=CLOSE_SEED):
    """Two insertions of one base closer than P: the phase between them is not decided locally."""
    return plant(period, [(12, "I", 1, 1), (12, "I", 1, period - 2)], seed)
