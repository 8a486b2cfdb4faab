// periodchain_word_check.cpp -- the word source of the period lines (csrc/periodchain_word.h: pc_word, pc_run_end) and the walks
// of csrc/dotchain_walk.h over it, compiled for the host, against a brute force that walks each line symbol by
// symbol.  A stand-alone program: tests/test_periodchain_cpu.py builds it with the sanitizers and runs it.  Prints
// "ok <lines> <chains> <words> <handed over>" and returns 0, or says what differs and returns 1.
//
// The planes are vectors of exactly the words that exist; the accessor refuses (and the sanitizer would catch) a word outside
// first .. last of the range, so "forms no address outside the words that hold [begin, end)" is checked, not assumed.  Ranges
// begin and end inside a word, at word 0 of the planes and in their last word; the positions around a range hold letters too.
// Every start of every line goes the way of the find kernel: the first run by pc_run_end (in one go, and stopped every few cells
// and resumed, as the long list hands it over), then dc_is_head, then dc_follow; words come from a one-word cache, as in the find
// kernel, or 64 at a time in the direction of the walk, as in the long kernel.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/periodchain_word.h"

namespace {

struct chain {
    u64 t0, len, matches;
    u32 seeds;
    bool operator==(const chain &o) const { return t0 == o.t0 && len == o.len && matches == o.matches && seeds == o.seeds; }
};

u64 rng_state = 0x2545F4914F6CDD1Dull;
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

// the planes of a text, as the packer writes them: H, L the two code bits ((ascii >> 1) & 3), X not ACGT, E the low five bits of
// a letter other than A, C, G, T, N
struct planes {
    std::vector<u64> H, L, X, E[5];
    bool five;
    u64 first, last;       // what the range may ask for
    mutable bool refused = false;
    u64 get(const std::vector<u64> &p, u64 w) const {
        if (w < first || w > last || w >= p.size()) {
            refused = true;
            return 0;
        }
        return p[w];
    }
    u64 h(u64 w) const { return get(H, w); }
    u64 l(u64 w) const { return get(L, w); }
    u64 x(u64 w) const { return get(X, w); }
    u64 e(int i, u64 w) const { return get(E[i], w); }
    bool exotic() const { return five; }
};

planes pack(const std::string &text, bool five) {
    planes p;
    const u64 words = (text.size() + 63) / 64;
    p.H.assign(words, 0), p.L.assign(words, 0), p.X.assign(words, 0);
    for (auto &e : p.E) e.assign(five ? words : 0, 0);
    p.five = five;
    for (u64 i = 0; i < text.size(); i++) {
        const char c = text[i];
        const u64 bit = 1ull << (i & 63);
        const bool acgt = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        if (acgt) {
            if ((c >> 1) & 2) p.H[i >> 6] |= bit;
            if ((c >> 1) & 1) p.L[i >> 6] |= bit;
        } else {
            p.X[i >> 6] |= bit;
            if (c != 'N')
                for (int k = 0; k < 5; k++)
                    if ((c >> k) & 1) p.E[k][i >> 6] |= bit;
        }
    }
    return p;
}

bool raw(char a, char b, u32 n_matches) { return a == b && (n_matches || a != 'N'); }

}  // namespace

int main() {
    u64 lines = 0, chains = 0, words_checked = 0, handed = 0;
    for (int round = 0; round < 1500; round++) {
        const bool five = round % 3 == 0;
        const char *letters = five ? "ACGTNRY" : "ACGTN";
        const u64 n_letters = five ? 7 : 5;
        const bool hand_made = round % 8 == 1;
        // the planes: `total` positions; the range [begin, begin + n)
        const u64 total = 1 + rnd() % (round % 10 == 0 ? 2600 : 700);
        u64 begin = rnd() % total, n = 1 + rnd() % (total - begin);
        switch (round % 6) {
            case 0: begin = 0; n = 1 + rnd() % total; break;                       // from word 0 of the planes
            case 1: n = total - begin; break;                                      // ends in the last word of the planes
            case 2: begin = 0; n = total; break;                                   // both
            case 3: begin = (begin / 64) * 64; n = 1 + rnd() % (total - begin); break;
            default: break;                                                        // begins and ends inside a word
        }
        std::string text(total, 'A');
        const unsigned n_share = rnd() % 4 == 0 ? 30 : 4;                          // per cent of N
        for (u64 i = 0; i < total; i++) text[i] = rnd() % 100 < n_share ? 'N' : letters[rnd() % n_letters];
        if (hand_made) {                                                           // a repeat of period 1 .. 70 with substitutions and an N block
            const u64 period = 1 + rnd() % 70;
            for (u64 i = begin + period; i < begin + n; i++) text[i] = text[i - period];
            for (int k = 0; k < 8; k++) text[begin + rnd() % n] = letters[rnd() % n_letters];
            const u64 at = begin + rnd() % n;
            for (u64 i = at; i < begin + n && i < at + 90; i++) text[i] = 'N';
        }
        const planes pl = [&] {
            planes p = pack(text, five);
            p.first = begin >> 6, p.last = (begin + n - 1) >> 6;
            return p;
        }();
        const u64 seeds_at[] = {1, 2, 3, 4, 8, 11, 16, 17, 64, 65};
        const u32 gaps_at[] = {0, 1, 2, 5, 8, 16, 63, 64, 65, 300, 4096};
        for (u32 n_matches = 0; n_matches < 2; n_matches++) {
            const pc_range r = pc_range_of(begin, n, n_matches);
            const u64 ks[] = {1, 2, 3, 1 + rnd() % 9, 63, 64, 65, 127, 128, 1 + rnd() % (n + 3), n > 1 ? n - 1 : 1, n, n + 5};
            for (const u64 k : ks) {
                std::vector<char> cells(k < n ? n - k : 0);
                for (u64 t = 0; t < cells.size(); t++) cells[t] = raw(text[begin + t], text[begin + t + k], n_matches);
                // ---- the words
                for (u64 wk = 0; wk < cells.size() / 64 + 3; wk++) {
                    u64 want = 0;
                    for (u64 b = 0; b < 64; b++)
                        if (64 * wk + b < cells.size() && cells[64 * wk + b]) want |= 1ull << b;
                    const u64 got = pc_word(pl, r, k, wk);
                    if (got != want)
                        return printf("round %d: word %llu of line %llu is %016llx, the brute force has %016llx (begin %llu, n %llu, n_matches %u)\n", round, wk, k, got,
                                      want, begin, n, n_matches), 1;
                    ++words_checked;
                }
                // ---- the walks, as the find kernel runs them
                const u64 min_seed = seeds_at[rnd() % 10];
                const u32 max_gap = gaps_at[rnd() % 11];
                const std::vector<chain> want = brute(cells, min_seed, max_gap);
                std::vector<chain> got;
                for (u64 s = 0; s < cells.size(); s++) {
                    if (!cells[s] || (s && cells[s - 1])) continue;                // a run starts at s
                    u64 have = ~0ull, held = 0;
                    const auto cached = [&](u64 wk) {
                        if (wk != have) held = pc_word(pl, r, k, wk), have = wk;
                        return held;
                    };
                    u64 p = s + 1;
                    if (!pc_run_end(p, ~0ull, cached)) return printf("round %d: a run without an end\n", round), 1;
                    u64 e = s;
                    while (e + 1 < cells.size() && cells[e + 1]) ++e;
                    if (p != e + 1) return printf("round %d: line %llu: the run at %llu ends at %llu, the brute force has %llu\n", round, k, s, p, e + 1), 1;
                    // stopped and resumed from p alone
                    const u64 stride = 1 + rnd() % 100;
                    u64 q = s + 1;
                    while (!pc_run_end(q, q + stride, cached)) ++handed;
                    if (q != p) return printf("round %d: a resumed run differs\n", round), 1;
                    const u64 len = p - s;
                    if (len < min_seed) continue;
                    // the head test over words fetched 64 at a time, backwards, as the long kernel's wave loads them
                    u64 base = 0, block[64];
                    bool loaded = false, back = true;
                    const auto wave = [&](u64 wk) {
                        if (!loaded || wk < base || wk - base >= 64) {
                            base = back ? (wk >= 63 ? wk - 63 : 0) : wk;
                            for (u64 lane = 0; lane < 64; lane++) block[lane] = pc_word(pl, r, k, base + lane);
                            loaded = true;
                        }
                        return block[wk - base];
                    };
                    const bool head = dc_is_head(s, min_seed, max_gap, cached);
                    if (head != dc_is_head(s, min_seed, max_gap, wave)) return printf("round %d: the block-fed head test differs\n", round), 1;
                    if (!head) continue;
                    dc_state one = dc_first_seed(s, len);
                    if (!dc_follow(one, min_seed, max_gap, ~0ull, cached)) return printf("round %d: the follow stopped without a stop\n", round), 1;
                    got.push_back(chain{s, one.end - s + 1, one.matches, one.seeds});
                    dc_state cut = dc_first_seed(s, len);
                    u64 stop = s + len + stride;
                    while (!dc_follow(cut, min_seed, max_gap, stop, cached)) stop = cut.p + stride, ++handed;
                    back = false;
                    dc_state fed = dc_first_seed(s, len);
                    dc_follow(fed, min_seed, max_gap, ~0ull, wave);
                    for (const dc_state *other : {&cut, &fed})
                        if (other->end != one.end || other->matches != one.matches || other->seeds != one.seeds)
                            return printf("round %d: seed at %llu: a resumed or block-fed follow differs\n", round, s), 1;
                }
                if (got.size() != want.size())
                    return printf("round %d: line %llu: %zu chains, the brute force has %zu (n %llu, min_seed %llu, max_gap %u, n_matches %u)\n", round, k, got.size(),
                                  want.size(), n, min_seed, max_gap, n_matches), 1;
                for (size_t i = 0; i < want.size(); i++)
                    if (!(got[i] == want[i]))
                        return printf("round %d: line %llu: chain %zu is (%llu, %llu, %llu, %u), the brute force has (%llu, %llu, %llu, %u)\n", round, k, i, got[i].t0,
                                      got[i].len, got[i].matches, got[i].seeds, want[i].t0, want[i].len, want[i].matches, want[i].seeds), 1;
                ++lines;
                chains += want.size();
            }
        }
        if (pl.refused) return printf("round %d: a word outside the range's words was asked for (begin %llu, n %llu)\n", round, begin, n), 1;
    }
    printf("ok %llu %llu %llu %llu\n", lines, chains, words_checked, handed);
    return 0;
}
