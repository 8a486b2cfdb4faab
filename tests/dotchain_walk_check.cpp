// dotchain_walk_check.cpp -- the two walks of csrc/dotchain_walk.h (the head test and the follow of the chain kernels),
// compiled for the host, against a brute force on random lines.  A stand-alone program: tests/test_dotchain_cpu.py builds it
// with the sanitizers and runs it.  Prints "ok <lines> <chains> <handed over>" and returns 0, or says what differs and returns 1.
//
// A line is a vector of cells (raw or not).  Brute force: the maximal runs, the seeds among them, the links, the chains with their
// matches counted cell by cell.  The walks see the line as 64-cell words, cells behind its end not raw, as dr_step gives them.
// Every head's follow runs three ways: in one go; stopped after every `stride` cells and resumed from the state alone, as the
// long kernel resumes what the link kernel hands over; and over words fetched 64 at a time, as the long kernel's wave loads them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/dotchain_walk.h"

namespace {

struct chain {
    u64 t0, len, matches;
    u32 seeds;
    bool operator==(const chain &o) const { return t0 == o.t0 && len == o.len && matches == o.matches && seeds == o.seeds; }
};

u64 rng_state = 0x9E3779B97F4A7C15ull;
u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

std::vector<chain> brute(const std::vector<char> &cells, u64 min_seed, u32 max_gap) {
    std::vector<chain> out;
    const u64 n = cells.size();
    bool open = false;
    u64 end = 0;
    for (u64 s = 0; s < n;) {
        if (!cells[s]) {
            ++s;
            continue;
        }
        u64 e = s;
        while (e + 1 < n && cells[e + 1]) ++e;
        if (e - s + 1 >= min_seed) {
            if (open && s - end - 1 <= max_gap) {
                chain &c = out.back();
                for (u64 t = end + 1; t <= e; t++) c.matches += cells[t] ? 1 : 0;
                c.len = e - c.t0 + 1;
                c.seeds++;
            } else {
                out.push_back(chain{s, e - s + 1, e - s + 1, 1u});
            }
            open = true;
            end = e;
        }
        s = e + 1;
    }
    return out;
}

}  // namespace

int main() {
    u64 lines = 0, chains = 0, handed = 0;
    for (int round = 0; round < 6000; round++) {
        const u64 n = 1 + rnd() % (round % 7 == 0 ? 9000 : 700);
        const unsigned density = 40 + rnd() % 59;                 // per cent of raw cells
        std::vector<char> cells(n);
        for (u64 t = 0; t < n; t++) cells[t] = rnd() % 100 < density;
        if (round % 5 == 0)                                       // long exact stretches and long empty ones
            for (int k = 0; k < 6; k++) {
                const u64 at = rnd() % n, len = rnd() % 300;
                const char v = rnd() & 1;
                for (u64 t = at; t < n && t < at + len; t++) cells[t] = v;
            }
        std::vector<u64> words((n + 63) / 64 + 1, 0);
        for (u64 t = 0; t < n; t++)
            if (cells[t]) words[t >> 6] |= 1ull << (t & 63);
        const auto word = [&](u64 k) { return k < words.size() ? words[k] : 0ull; };
        const u64 seeds_at[] = {1, 2, 3, 4, 8, 11, 16, 17, 64, 65, 200};
        const u32 gaps_at[] = {0, 1, 2, 5, 8, 16, 63, 64, 65, 300, 4096};
        const u64 min_seed = seeds_at[rnd() % 11];
        const u32 max_gap = gaps_at[rnd() % 11];
        const std::vector<chain> want = brute(cells, min_seed, max_gap);
        std::vector<chain> got;
        for (u64 s = 0; s < n;) {                                 // every seed of the line, as the link kernel gets them
            if (!cells[s]) {
                ++s;
                continue;
            }
            u64 e = s;
            while (e + 1 < n && cells[e + 1]) ++e;
            const u64 len = e - s + 1;
            if (len >= min_seed && dc_is_head(s, min_seed, max_gap, word)) {
                dc_state one = dc_first_seed(s, len);
                if (!dc_follow(one, min_seed, max_gap, ~0ull, word)) return printf("round %d: the follow stopped without a stop\n", round), 1;
                got.push_back(chain{s, one.end - s + 1, one.matches, one.seeds});
                // stopped and resumed
                const u64 stride = 1 + rnd() % 130;
                dc_state cut = dc_first_seed(s, len);
                u64 stop = s + len + stride;
                while (!dc_follow(cut, min_seed, max_gap, stop, word)) {
                    const dc_state saved = cut;                   // what prf_dotchain_long carries
                    cut = dc_state{saved.end, saved.matches, saved.pending, saved.p, saved.run_start, saved.seeds, saved.in_run};
                    stop = cut.p + stride;
                    ++handed;
                }
                // words fetched 64 at a time, from the first one asked for
                dc_state wave = dc_first_seed(s, len);
                u64 base = 0, block[64];
                bool loaded = false;
                dc_follow(wave, min_seed, max_gap, ~0ull, [&](u64 k) {
                    if (!loaded || k - base >= 64) {
                        base = k;
                        for (u64 lane = 0; lane < 64; lane++) block[lane] = word(base + lane);
                        loaded = true;
                    }
                    return block[k - base];
                });
                for (const dc_state *other : {&cut, &wave})
                    if (other->end != one.end || other->matches != one.matches || other->seeds != one.seeds)
                        return printf("round %d: seed at %llu: a resumed or block-fed follow differs\n", round, s), 1;
            }
            s = e + 1;
        }
        if (got.size() != want.size()) return printf("round %d: %zu chains, the brute force has %zu (n %llu, min_seed %llu, max_gap %u)\n", round, got.size(), want.size(), n, min_seed, max_gap), 1;
        for (size_t k = 0; k < want.size(); k++)
            if (!(got[k] == want[k]))
                return printf("round %d: chain %zu is (%llu, %llu, %llu, %u), the brute force has (%llu, %llu, %llu, %u)\n", round, k, got[k].t0, got[k].len,
                              got[k].matches, got[k].seeds, want[k].t0, want[k].len, want[k].matches, want[k].seeds), 1;
        ++lines;
        chains += want.size();
    }
    printf("ok %llu %llu %llu\n", lines, chains, handed);
    return 0;
}
