// dotlink_walk_check.cpp -- the two walks of csrc/dotlink_walk.h (the tail and the head in a stretch of a line, the join kernel's
// steps A and B), compiled for the host, against a brute force on random lines.  A stand-alone program:
// tests/test_dotlink_cpu.py builds it with the sanitizers and runs it.  Prints "ok <lines> <stretches> <tails> <heads>" and
// returns 0, or says what differs and returns 1.
//
// A line is a vector of cells (raw or not).  Brute force: the maximal runs, the seeds among them, the chains as (first cell, last
// cell); the tail (head) of a stretch is the chain whose last (first) cell lies in it, and the brute force checks that there is
// at most one.  The walks see the line as 64-cell words, cells behind its end not raw, as dr_step gives them.  Stretches have the
// kernel's length, max_gap + min(min_seed - 1, 16) + 1 cells, cut by the line's start and reaching behind its end.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/dotlink_walk.h"

namespace {

u64 rng_state = 0x2545F4914F6CDD1Dull;
u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

struct span {
    u64 first, last;
};

std::vector<span> brute(const std::vector<char> &cells, u64 min_seed, u32 max_gap) {
    std::vector<span> out;
    const u64 n = cells.size();
    for (u64 s = 0; s < n;) {
        if (!cells[s]) {
            ++s;
            continue;
        }
        u64 e = s;
        while (e + 1 < n && cells[e + 1]) ++e;
        if (e - s + 1 >= min_seed) {
            if (!out.empty() && s - out.back().last - 1 <= max_gap) out.back().last = e;
            else out.push_back(span{s, e});
        }
        s = e + 1;
    }
    return out;
}

}  // namespace

int main() {
    u64 lines = 0, stretches = 0, tails = 0, heads = 0;
    for (int round = 0; round < 4000; round++) {
        const u64 n = 1 + rnd() % (round % 7 == 0 ? 6000 : 500);
        const unsigned density = 40 + rnd() % 59;                 // per cent of raw cells
        std::vector<char> cells(n);
        for (u64 t = 0; t < n; t++) cells[t] = rnd() % 100 < density;
        if (round % 3 == 0)                                       // long exact stretches and long empty ones
            for (int k = 0; k < 6; k++) {
                const u64 at = rnd() % n, len = rnd() % 300;
                const char v = rnd() & 1;
                for (u64 t = at; t < n && t < at + len; t++) cells[t] = v;
            }
        std::vector<u64> words((n + 63) / 64 + 1, 0);
        for (u64 t = 0; t < n; t++)
            if (cells[t]) words[t >> 6] |= 1ull << (t & 63);
        u64 have = ~0ull, kept = 0;                               // the word looked at last, as the kernel keeps it
        const auto word = [&](u64 k) {
            if (k != have) kept = k < words.size() ? words[k] : 0ull, have = k;
            return kept;
        };
        const u32 gaps_at[] = {0, 1, 2, 5, 8, 16, 47, 63, 64, 65, 300, 4096};
        const u64 min_seed = round % 4 == 0 ? 1 + (u64)(round / 4) % 70 : 1 + rnd() % 70;       // 1 .. 70, every value
        const u32 max_gap = gaps_at[rnd() % 12];
        const u64 ov = min_seed - 1 < 16 ? min_seed - 1 : 16;
        const std::vector<span> chains = brute(cells, min_seed, max_gap);
        for (int probe = 0; probe < 40; probe++) {
            // hi anywhere from cell 0 to behind the line's end; lo cut by the line's start
            u64 hi = rnd() % (n + max_gap + 40);
            if (probe < 8 && !chains.empty()) {                   // around the ends and the starts of the chains
                const span &c = chains[rnd() % chains.size()];
                const u64 at = probe & 1 ? c.last : c.first;
                hi = at + rnd() % (max_gap + ov + 1);
                if (probe & 2) hi = at + (probe & 4 ? max_gap + ov : 0);
            }
            const u64 lo = hi > max_gap + ov ? hi - max_gap - ov : 0;
            u64 want_tail = ~0ull, want_head = ~0ull;
            int n_tail = 0, n_head = 0;
            for (const span &c : chains) {
                if (c.last >= lo && c.last <= hi) want_tail = c.last, ++n_tail;
                if (c.first >= lo && c.first <= hi) want_head = c.first, ++n_head;
            }
            if (n_tail > 1 || n_head > 1) return printf("round %d: %d tails, %d heads in one stretch\n", round, n_tail, n_head), 1;
            const u64 got_tail = dl_tail_in_stretch(lo, hi, min_seed, max_gap, word);
            const u64 got_head = dl_head_in_stretch(lo, hi, min_seed, max_gap, word);
            if (got_tail != want_tail)
                return printf("round %d: tail in %llu .. %llu is %llu, the brute force has %llu (n %llu, min_seed %llu, max_gap %u)\n", round, lo, hi,
                              got_tail, want_tail, n, min_seed, max_gap), 1;
            if (got_head != want_head)
                return printf("round %d: head in %llu .. %llu is %llu, the brute force has %llu (n %llu, min_seed %llu, max_gap %u)\n", round, lo, hi,
                              got_head, want_head, n, min_seed, max_gap), 1;
            ++stretches;
            tails += want_tail != ~0ull;
            heads += want_head != ~0ull;
        }
        ++lines;
    }
    printf("ok %llu %llu %llu %llu\n", lines, stretches, tails, heads);
    return 0;
}
