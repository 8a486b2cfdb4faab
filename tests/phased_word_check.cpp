// phased_word_check.cpp -- the per-lane text of the phased-consensus kernels (csrc/phased_word.h: ph_count_item, ph_first_column,
// ph_lane_column, on cs_window, cs_base, cs_step of csrc/consensus_word.h) and the item cutting of a segment, compiled for the
// host, against a brute force that puts every position of every segment into its column letter by letter.  A
// stand-alone program: tests/test_phased_cpu.py builds it with the sanitizers and runs it.  Prints
// "ok <rows> <segments> <items> <words> <positions>" and returns 0, or says what differs and returns 1.
//
// The planes are vectors of exactly the words that exist.  The source refuses (and the sanitizer would catch) a word outside the
// words of the range, a word outside the words that hold the item, a word asked for twice and a word asked for out of order.
// Segments begin and end inside a word, at word 0 of the planes and in their last word.  A row has 1 .. 5 segments in any order,
// which may overlap; their counts meet in one table, as the kernels' adds meet in the global counts.  The 64 lanes of a wave are
// run one after the other, each over a source of its own.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/phased_word.h"

namespace {

u64 rng_state = 0xD1B54A32D192ED03ull;
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

u32 phase_of(u32 k, u64 pick) {
    switch (pick % 4) {
        case 0: return 0;
        case 1: return k > 1 ? 1u : 0u;
        case 2: return k - 1;
        default: return (u32)(rnd() % k);
    }
}

}  // namespace

int main() {
    u64 rows_checked = 0, segments_checked = 0, items_checked = 0, words_taken = 0, positions = 0;
    const u32 ks[] = {1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 500, 1023, 1024, 1025, 1500, 3000};
    for (int round = 0; round < 500; round++) {
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
        const planes pl = pack(text);
        for (int trial = 0; trial < 10; trial++) {
            const u32 k = trial < 2 ? (u32)(1 + rnd() % (n + 3)) : ks[rnd() % (sizeof ks / sizeof *ks)];
            const u32 regime = cs_regime(k), step = cs_step(k);
            const u32 n_segments = 1 + (u32)(rnd() % 5);
            std::vector<u32> want(4 * (size_t)k, 0), got(4 * (size_t)k, 0);
            for (u32 at = 0; at < n_segments; at++) {
                ph_segment s{};
                s.start = rnd() % n;
                s.end = s.start + 1 + rnd() % (n - s.start);
                if (trial == 0 && at == 0) s.start = 0, s.end = n;                 // the whole range
                if (trial == 1 && at == 0) s.end = n;                              // to the range's last position
                if (trial == 2 && at == 0) s.start = 0;                            // from the range's first position
                s.row = 0;
                s.phase = phase_of(k, trial + at);
                const u64 len = s.end - s.start;
                const u64 slices[] = {64, 100, k > 1 ? k - 1 : 1, 1 + rnd() % 300, 4096, len, 1};
                const u64 slice = slices[rnd() % (len > 400 ? 6 : 7)];
                // ---- the brute force
                for (u64 q = s.start; q < s.end; q++) {
                    const int b = base_of(text[begin + q]);
                    if (b < 4) want[4 * (size_t)((s.phase + (q - s.start)) % k) + b]++;
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
                    const ph_item it{s.start + first, s.start + end, at, 0u};
                    const u32 col0 = ph_first_column(s, k, it);
                    if (col0 != (s.phase + first) % k) return printf("round %d: the first column of an item is %u\n", round, col0), 1;
                    u64 words = 0;
                    for (u32 lane = 0; lane < 64; lane++) {
                        source src{pl, begin >> 6, (begin + n - 1) >> 6, (begin + it.first) >> 6, (begin + it.end - 1) >> 6, (begin + it.first) >> 6};
                        u32 lane_col = ~0u;
                        ph_count_item(src, begin, k, s, it, lane, [&](u32 col, u32 b) {
                            if (col >= k || b >= 4) {
                                src.refused = "a column or a base out of range";
                                return;
                            }
                            if (regime == PRF_CS_REG) {                            // the lane's column never changes
                                if (lane_col == ~0u) lane_col = col;
                                if (col != lane_col || col != ph_lane_column(s, k, it, lane) || lane >= step) src.refused = "a lane of k <= 64 left its column";
                            }
                            got[4 * (size_t)col + b]++;
                        });
                        if (src.refused)
                            return printf("round %d: %s (begin %llu, n %llu, segment [%llu, %llu) k %u phase %u, item [%llu, %llu), lane %u)\n", round, src.refused,
                                          begin, n, s.start, s.end, k, s.phase, it.first, it.end, lane), 1;
                        if (src.taken != src.item_last - src.item_first + 1)
                            return printf("round %d: lane %u took %llu words of the item's %llu\n", round, lane, src.taken, src.item_last - src.item_first + 1), 1;
                        words = src.taken;
                    }
                    words_taken += words;
                    ++items_checked;
                }
                if (covered != len) return printf("round %d: the items cover %llu of %llu positions\n", round, covered, len), 1;
                ++segments_checked;
                positions += len;
            }
            for (size_t i = 0; i < want.size(); i++)
                if (got[i] != want[i])
                    return printf("round %d trial %d: k %u: count[%zu][%zu] is %u, the brute force has %u (begin %llu, n %llu)\n", round, trial, k, i / 4, i % 4,
                                  got[i], want[i], begin, n), 1;
            ++rows_checked;
        }
    }
    // the lanes of a step of k > 64 hit 64 different columns at every phase: the LDS and the global regime rest on it.  Every
    // k = 65 .. 2 100 at six phases; the columns of a step are marked in a table of k entries
    for (u32 k = 65; k <= 2100; k++) {
        const u32 phases[] = {0, 1, k - 1, k / 2, 64, k - 64};
        const ph_segment whole{3, 3 + 5 * (u64)k + 17, 0u, 0u};
        const std::string text(whole.end + 64, 'C');
        const planes pl = pack(text);
        for (u32 phase : phases) {
            const ph_segment s{whole.start, whole.end, 0u, phase};
            const ph_item it{s.start + 70, s.end, 0u, 0u};
            std::vector<std::vector<u32>> cols(64);
            for (u32 lane = 0; lane < 64; lane++) {
                source src{pl, 0, (s.end - 1) >> 6, it.first >> 6, (it.end - 1) >> 6, it.first >> 6};
                ph_count_item(src, 0, k, s, it, lane, [&](u32 col, u32) { cols[lane].push_back(col); });
            }
            std::vector<size_t> seen(k, ~(size_t)0);               // the step that marked a column last
            for (size_t st = 0; st < cols[0].size(); st++)
                for (u32 x = 0; x < 64; x++) {
                    if (st >= cols[x].size()) continue;
                    const u32 col = cols[x][st];
                    if (col >= k || seen[col] == st) return printf("k %u phase %u: lane %u shares column %u with another lane in step %zu\n", k, phase, x, col, st), 1;
                    seen[col] = st;
                }
            if (cols[0].empty() || cols[0][0] != (phase + 70) % k) return printf("k %u phase %u: the first column is not %u\n", k, phase, (phase + 70) % k), 1;
        }
    }
    printf("ok %llu %llu %llu %llu %llu\n", rows_checked, segments_checked, items_checked, words_taken, positions);
    return 0;
}
