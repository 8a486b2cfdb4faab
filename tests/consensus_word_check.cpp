// consensus_word_check.cpp -- the per-lane text of the consensus kernels (csrc/consensus_word.h: cs_count_item, cs_window,
// cs_base, cs_consensus) and the item cutting (cs_n_items, cs_item_span, cs_regime), compiled for the host, against a brute force
// that counts each column letter by letter.  A stand-alone program: tests/test_consensus_cpu.py builds it with the
// sanitizers and runs it.  Prints "ok <rows> <items> <words> <positions>" and returns 0, or says what differs and returns 1.
//
// The planes are vectors of exactly the words that exist.  The source refuses (and the sanitizer would catch) a word outside the
// words of the range, a word outside the words that hold the item, a word asked for twice and a word asked for out of order, so
// "every word once, as a whole word, and no word outside the range's" is checked, not assumed.  Ranges begin and end inside a
// word, at word 0 of the planes and in their last word; the positions around a range hold letters too.  The 64 lanes of a wave
// are run one after the other, each over a source of its own, as the kernel's lanes each see the same words.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/consensus_word.h"

namespace {

u64 rng_state = 0x9E3779B97F4A7C15ull;
u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// the planes of a text, as the packer writes them: H, L the two code bits ((ascii >> 1) & 3), X not ACGT
struct planes {
    std::vector<u64> H, L, X;
};

planes pack(const std::string &text) {
    planes p;
    const u64 words = (text.size() + 63) / 64;
    p.H.assign(words, 0), p.L.assign(words, 0), p.X.assign(words, 0);
    for (u64 i = 0; i < text.size(); i++) {
        const char c = (char)(text[i] & ~0x20);
        const u64 bit = 1ull << (i & 63);
        if (c == 'A' || c == 'C' || c == 'G' || c == 'T') {
            if ((c >> 1) & 2) p.H[i >> 6] |= bit;
            if ((c >> 1) & 1) p.L[i >> 6] |= bit;
        } else {
            p.X[i >> 6] |= bit;
        }
    }
    return p;
}

struct source {
    const planes &pl;
    u64 range_first, range_last;   // the words of the range
    u64 item_first, item_last;     // the words that hold the item
    u64 next;                      // the word that may be asked for next
    u64 taken = 0;
    const char *refused = nullptr;
    void take(u64 w, u64 *out) {
        out[0] = out[1] = out[2] = 0;
        if (w < range_first || w > range_last || w >= pl.H.size()) refused = "a word outside the range's words";
        else if (w < item_first || w > item_last) refused = "a word that holds no position of the item";
        else if (w != next) refused = "a word twice or out of order";
        if (refused) return;
        next = w + 1;
        ++taken;
        out[0] = pl.H[w], out[1] = pl.L[w], out[2] = pl.X[w];
    }
};

int base_of(char c) {
    switch (c & ~0x20) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}

}  // namespace

int main() {
    u64 rows_checked = 0, items_checked = 0, words_taken = 0, positions = 0;
    const u32 ks[] = {1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 500, 1023, 1024, 1025, 1500, 3000};
    for (int round = 0; round < 600; round++) {
        const char *letters = round % 3 == 0 ? "ACGTNRYacgtn" : "ACGT";
        const u64 n_letters = round % 3 == 0 ? 12 : 4;
        const u64 total = 1 + rnd() % (round % 10 == 0 ? 9000 : 1200);
        u64 begin = rnd() % total, n = 1 + rnd() % (total - begin);
        switch (round % 6) {
            case 0: begin = 0; n = 1 + rnd() % total; break;                       // from word 0 of the planes
            case 1: n = total - begin; break;                                      // ends in the last word of the planes
            case 2: begin = 0; n = total; break;                                   // both
            case 3: begin = (begin / 64) * 64; n = 1 + rnd() % (total - begin); break;
            default: break;                                                        // begins and ends inside a word
        }
        std::string text(total, 'A');
        for (u64 i = 0; i < total; i++) text[i] = letters[rnd() % n_letters];
        if (round % 4 == 1) {                                                      // a repeat with substitutions and an N block
            const u64 period = 1 + rnd() % 200;
            for (u64 i = begin + period; i < begin + n; i++) text[i] = text[i - period];
            for (int j = 0; j < 10; j++) text[begin + rnd() % n] = letters[rnd() % n_letters];
            const u64 at = begin + rnd() % n;
            for (u64 i = at; i < begin + n && i < at + 90; i++) text[i] = 'N';
        }
        const planes pl = pack(text);
        for (int trial = 0; trial < 12; trial++) {
            cs_row r{};
            r.k = trial < 2 ? (u32)(1 + rnd() % (n + 3)) : ks[rnd() % (sizeof ks / sizeof *ks)];
            r.start = rnd() % n;
            r.end = r.start + 1 + rnd() % (n - r.start);
            if (trial == 0) r.start = 0, r.end = n;                                // the whole range
            if (trial == 1) r.end = n;                                             // to the range's last position
            r.offset = rnd() % 1000;
            const u64 len = r.end - r.start;
            const u64 slices[] = {64, 100, r.k > 1 ? r.k - 1 : 1, 1 + rnd() % 300, 4096, len, 1};
            const u64 slice = slices[rnd() % (len > 400 ? 6 : 7)];
            // ---- the brute force
            std::vector<u32> want(4 * (size_t)r.k, 0), got(4 * (size_t)r.k, 0);
            for (u64 q = r.start; q < r.end; q++) {
                const int b = base_of(text[begin + q]);
                if (b < 4) want[4 * ((q - r.start) % r.k) + b]++;
            }
            // ---- the items, lane by lane
            const u64 n_items = cs_n_items(len, slice);
            u64 covered = 0;
            for (u64 j = 0; j < n_items; j++) {
                u64 first, end;
                cs_item_span(len, slice, j, &first, &end);
                if (first != covered || end <= first || end - first > slice || end > len)
                    return printf("round %d: item %llu of %llu positions at slice %llu is [%llu, %llu)\n", round, j, len, slice, first, end), 1;
                covered = end;
                const cs_item it{r.start + first, r.start + end, 0u, 0u};
                const u32 regime = cs_regime(r.k), step = cs_step(r.k);
                if ((regime == PRF_CS_REG) != (r.k <= 64) || (regime == PRF_CS_GLOBAL) != (r.k > PRF_CS_LDS_K) || step > 64 || step < 33 ||
                    (regime == PRF_CS_REG && step % r.k) || (regime != PRF_CS_REG && step != 64))
                    return printf("round %d: k %u: regime %u, step %u\n", round, r.k, regime, step), 1;
                u64 words = 0;
                for (u32 lane = 0; lane < 64; lane++) {
                    source src{pl, begin >> 6, (begin + n - 1) >> 6, (begin + it.first) >> 6, (begin + it.end - 1) >> 6, (begin + it.first) >> 6};
                    u32 lane_col = ~0u;
                    cs_count_item(src, begin, r, it, lane, [&](u32 col, u32 b) {
                        if (col >= r.k || b >= 4) {
                            src.refused = "a column or a base out of range";
                            return;
                        }
                        if (regime == PRF_CS_REG) {                                // the lane's column never changes
                            if (lane_col == ~0u) lane_col = col;
                            if (col != lane_col || col != cs_lane_column(r, it, lane) || lane >= step) src.refused = "a lane of k <= 64 left its column";
                        }
                        got[4 * (size_t)col + b]++;
                    });
                    if (src.refused)
                        return printf("round %d: %s (begin %llu, n %llu, row [%llu, %llu) k %u, item [%llu, %llu), lane %u)\n", round, src.refused, begin, n, r.start,
                                      r.end, r.k, it.first, it.end, lane), 1;
                    if (src.taken != src.item_last - src.item_first + 1)
                        return printf("round %d: lane %u took %llu words of the item's %llu\n", round, lane, src.taken, src.item_last - src.item_first + 1), 1;
                    words = src.taken;
                }
                words_taken += words;
                ++items_checked;
            }
            if (covered != len) return printf("round %d: the items cover %llu of %llu positions\n", round, covered, len), 1;
            if (got != want) {
                for (size_t i = 0; i < want.size(); i++)
                    if (got[i] != want[i])
                        return printf("round %d: row [%llu, %llu) k %u slice %llu: count[%zu][%zu] is %u, the brute force has %u (begin %llu, n %llu)\n", round,
                                      r.start, r.end, r.k, slice, i / 4, i % 4, got[i], want[i], begin, n), 1;
            }
            // ---- the letters
            for (u32 p = 0; p < r.k; p++) {
                u32 best;
                const char c = cs_consensus(&got[4 * (size_t)p], &best);
                u32 at = 0;
                for (u32 b = 1; b < 4; b++)
                    if (want[4 * (size_t)p + b] > want[4 * (size_t)p + at]) at = b;
                const u32 most = want[4 * (size_t)p + at];
                if (best != most || c != (most ? "ACGT"[at] : 'N')) return printf("round %d: column %u: letter %c, count %u\n", round, p, c, best), 1;
            }
            ++rows_checked;
            positions += len;
        }
    }
    // the lanes of a step of k > 64 hit 64 different columns: the LDS and the global regime rest on it
    for (u32 k = 65; k <= 2100; k += (k < 140 ? 1 : 97)) {
        const cs_row r{3, 3 + 5 * (u64)k + 17, 0, k, 0u};
        const cs_item it{r.start + 70, r.end, 0u, 0u};
        const std::string text(r.end + 64, 'C');
        const planes pl = pack(text);
        std::vector<std::vector<u32>> cols(64);
        for (u32 lane = 0; lane < 64; lane++) {
            source src{pl, 0, (r.end - 1) >> 6, it.first >> 6, (it.end - 1) >> 6, it.first >> 6};
            cs_count_item(src, 0, r, it, lane, [&](u32 col, u32) { cols[lane].push_back(col); });
        }
        for (size_t s = 0; s < cols[0].size(); s++)
            for (u32 x = 0; x < 64; x++)
                for (u32 y = x + 1; y < 64; y++)
                    if (s < cols[x].size() && s < cols[y].size() && cols[x][s] == cols[y][s])
                        return printf("k %u: lanes %u and %u share column %u in step %zu\n", k, x, y, cols[x][s], s), 1;
    }
    printf("ok %llu %llu %llu %llu\n", rows_checked, items_checked, words_taken, positions);
    return 0;
}
