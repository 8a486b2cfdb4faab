// alignpath_word_check.cpp -- the per-lane text of the alignment-path kernels (csrc/alignpath_word.h: the two bits of a cell, the
// packing of the trace words, the trace-word address, the step of the walk, the batch dealer), compiled for the host.
// A stand-alone program: tests/test_alignpath_cpu.py builds it with the sanitizers and runs it.  Prints "ok <rows> <cells>
// <batches>" and returns 0, or says what differs and returns 1.
//
// The 64 lanes of a wave are run one after the other; what the kernels do across lanes is done here on arrays, in the same
// order.  The reference keeps the full matrix of explicit triples and of the two bits by their definition (from_del compares D'
// with T, both kept), then walks it.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/alignpath_word.h"

namespace {

u64 rng_state = 0x9E3779B97F4A7C15ull;
u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            printf("FAILED %s: ", #cond);    \
            printf(__VA_ARGS__);             \
            printf("\n");                    \
            if (++failures > 20) exit(1);    \
        }                                    \
    } while (0)

using triple = std::tuple<u32, u32, u32>;
triple add(const triple &a, u32 e, u32 i, u32 c) { return triple{std::get<0>(a) + e, std::get<1>(a) + i, std::get<2>(a) + c}; }

struct answer {
    al_result al;
    std::vector<u32> path;         // without the SUB bit
    u64 deletions = 0;
};

// bases 0 .. 3, 4 for none; motif codes 0 .. 3, 5 for N
answer reference(const std::vector<u32> &seq, const std::vector<u32> &motif) {
    const u32 k = (u32)motif.size(), n = (u32)seq.size();
    std::vector<triple> D(k, triple{0, 0, 0}), T(k), P(k);
    std::vector<std::vector<unsigned char>> ins(n, std::vector<unsigned char>(k)), del(n, std::vector<unsigned char>(k));
    for (u32 i = 0; i < n; i++) {
        for (u32 j = 0; j < k; j++) {
            const triple across = add(D[(j + k - 1) % k], motif[j] == seq[i] ? 0u : 1u, 0, 1), down = add(D[j], 1, 1, 0);
            ins[i][j] = down < across;
            P[j] = T[j] = std::min(across, down);
        }
        for (u32 j = 1; j < k; j++) P[j] = std::min(P[j], add(P[j - 1], 1, 1, 1));
        const triple last = P[k - 1];
        for (u32 j = 0; j < k; j++) {
            D[j] = std::min(P[j], add(last, j + 1, j + 1, j + 1));
            del[i][j] = D[j] < T[j];
        }
        for (u32 j = 0; j < k; j++)                                           // the identity the walk rests on
            CHECK(D[j] == std::min(T[j], add(D[(j + k - 1) % k], 1, 1, 1)), "k %u position %u column %u: D' is not min(T, left + del)", k, i, j);
    }
    u32 col = 0;
    for (u32 j = 1; j < k; j++)
        if (D[j] < D[col]) col = j;
    const u32 consumed = std::get<2>(D[col]);
    answer out;
    out.al = al_result{std::get<0>(D[col]), std::get<1>(D[col]), consumed, (u32)(((long long)col + 1 - consumed) % k + k) % k, col, 0};
    out.path.assign(n, 0);
    u32 j = col;
    for (u32 i = n; i-- > 0;) {
        u32 run = 0;
        while (del[i][j]) {
            j = (j + k - 1) % k;
            ++out.deletions;
            CHECK(++run < k, "k %u position %u: a run of k deletions", k, i);
        }
        if (ins[i][j]) out.path[i] = j | PRF_AP_INS;
        else out.path[i] = j, j = (j + k - 1) % k;
    }
    return out;
}

template <int C>
answer wave(const std::vector<u32> &seq, const std::string &letters, u64 slack) {
    const u32 k = (u32)letters.size(), n = (u32)seq.size(), R = al_regime(k);
    CHECK((1u << R) == (u32)C, "k %u in regime %u", k, R);
    std::array<std::array<u64, C>, 64> D, U;
    u32 real[64], bits[64], own[64], word[64] = {};
    u64 bias0[64], codes[64], inc[64];
    const u32 lanes = al_real_lanes(k, C);
    // the row's trace between two guards, every word written exactly once
    const u64 words = ap_trace_words(n, R);
    std::vector<u32> trace(slack + words + slack, 0xDEADBEEFu);
    std::vector<unsigned char> written(words, 0);
    for (u32 lane = 0; lane < 64; lane++) {
        real[lane] = al_real_slots(k, C, lane);
        bias0[lane] = real[lane] ? al_bias(k, lane * C) : 0;
        codes[lane] = al_lane_codes<C>(letters.data(), k, lane);
        al_lane_open<C>(D[lane].data(), real[lane]);
    }
    u64 last = 0;
    for (u32 i = 0; i < n; i++) {
        const u32 b = seq[i];
        u64 up[64];
        for (u32 lane = 0; lane < 64; lane++) up[lane] = lane ? D[lane - 1][C - 1] : last;
        for (u32 lane = 0; lane < 64; lane++)
            inc[lane] = ap_lane_scan<C>(D[lane].data(), up[lane], b, codes[lane], real[lane], bias0[lane], U[lane].data(), &bits[lane], &own[lane]);
        for (u32 d = 1; d < lanes; d <<= 1)                                   // the steps of the kernel's scan, all lanes at once
            for (u32 lane = 63; lane >= d; lane--) inc[lane] = al_min(inc[lane], inc[lane - d]);
        last = inc[lanes - 1];
        for (u32 lane = 0; lane < 64; lane++)
            ap_lane_wrap<C>(U[lane].data(), lane ? inc[lane - 1] : AL_SENTINEL, last, real[lane], bias0[lane], lane * C, own[lane], D[lane].data(), &bits[lane]);
        for (u32 lane = 0; lane < 64; lane++) {
            CHECK((u64)bits[lane] < (1ull << (2 * C)),"k %u lane %u: bits %x", k, lane, bits[lane]);
            if (ap_pack(&word[lane], bits[lane], i, n, R)) {
                const u64 at = ap_word_index(i, lane, R);
                CHECK(at < words && !written[at], "k %u n %u position %u lane %u: word %llu", k, n, i, lane, (unsigned long long)at);
                if (at < words) trace[slack + at] = word[lane], written[at] = 1;
                word[lane] = 0;
            }
        }
    }
    for (u64 at = 0; at < words; at++) CHECK(written[at], "k %u n %u: word %llu is not written", k, n, (unsigned long long)at);
    u64 best = AL_SENTINEL;
    u32 best_col = 0xFFFFFFFFu;
    for (u32 lane = 64; lane-- > 0;) {
        u64 v;
        u32 col;
        al_lane_pick<C>(D[lane].data(), real[lane], lane * C, &v, &col);
        al_pick(&best, &best_col, v, col);
    }
    answer out;
    out.al = al_finish(best, best_col, k);
    out.path.assign(n, 0);
    // the walk
    u32 j = out.al.end_column;
    for (u32 i = n; i-- > 0;) {
        u32 entry = 0, run = 0;
        for (;;) {
            const u32 code = ap_code(trace[slack + ap_word_index(i, j >> R, R)], i, j, R);
            if (ap_walk_step(code, k, &j, &entry)) break;
            ++out.deletions;
            if (++run >= k) {
                CHECK(false, "k %u position %u: a run of k deletions", k, i);
                break;
            }
        }
        out.path[i] = entry;
    }
    return out;
}

answer run(const std::vector<u32> &seq, const std::string &letters) {
    const u64 slack = rnd() % 3;
    switch (al_regime((u32)letters.size())) {
    case 0: return wave<1>(seq, letters, slack);
    case 1: return wave<2>(seq, letters, slack);
    case 2: return wave<4>(seq, letters, slack);
    case 3: return wave<8>(seq, letters, slack);
    default: return wave<16>(seq, letters, slack);
    }
}

bool same(const al_result &a, const al_result &b) {
    return a.edits == b.edits && a.indels == b.indels && a.consumed == b.consumed && a.start_column == b.start_column &&
           a.end_column == b.end_column && !a.reserved && !b.reserved;
}

u64 check_deal(const std::vector<ap_row> &in, u64 budget, u64 want_batches) {
    std::vector<ap_row> rows = in;
    std::vector<ap_batch> batches;
    ap_deal(rows, budget, batches);
    u64 at = 0;
    for (const ap_batch &b : batches) {
        CHECK(b.row0 == at && b.n_rows >= 1, "batch at %llu", (unsigned long long)at);
        u64 words = 0;
        for (u64 i = 0; i < b.n_rows; i++) {
            const ap_row &r = rows[b.row0 + i];
            CHECK(r.trace == words, "row %llu begins at %llu, not %llu", (unsigned long long)(b.row0 + i), (unsigned long long)r.trace, (unsigned long long)words);
            words += ap_trace_words((u32)(r.end - r.start), al_regime(r.k));
        }
        CHECK(words == b.words && (words <= budget || b.n_rows == 1), "batch of %llu rows holds %llu words, budget %llu", (unsigned long long)b.n_rows,
              (unsigned long long)words, (unsigned long long)budget);
        at += b.n_rows;
        // greedy: the next row would not have fitted
        if (at < rows.size())
            CHECK(words + ap_trace_words((u32)(rows[at].end - rows[at].start), al_regime(rows[at].k)) > budget, "batch closed early at %llu", (unsigned long long)at);
    }
    CHECK(at == rows.size(), "the batches hold %llu of %llu rows", (unsigned long long)at, (unsigned long long)rows.size());
    if (want_batches) CHECK(batches.size() == want_batches, "%llu batches, not %llu", (unsigned long long)batches.size(), (unsigned long long)want_batches);
    return batches.size();
}

}  // namespace

int main() {
    // ---- the layout: every (position, column) has its own two bits of its own word
    for (u32 R = 0; R < PRF_AL_REGIMES; R++) {
        const u32 C = 1u << R, per = ap_group_positions(R);
        CHECK(per * 2 * C == 32 && (1u << ap_group_shift(R)) == per, "regime %u", R);
        for (u32 n : {1u, per - 1 ? per - 1 : 1u, per, per + 1, 64u, 65u, 300u}) {
            CHECK(ap_n_groups(n, R) == (n + per - 1) / per && ap_trace_words(n, R) == 64ull * ((n + per - 1) / per), "regime %u n %u", R, n);
            std::vector<u32> seen(ap_trace_words(n, R), 0);
            for (u32 i = 0; i < n; i++)
                for (u32 j = 0; j < 64 * C; j += (j % 7 == 0 ? 1 : 5)) {
                    const u64 at = ap_word_index(i, j >> R, R);
                    const u32 shift = ap_field_shift(i, R) + 2 * (j & (C - 1));
                    CHECK(at < seen.size() && shift <= 30 && !(seen[at] & (3u << shift)), "regime %u position %u column %u", R, i, j);
                    if (at < seen.size()) seen[at] |= 3u << shift;
                    CHECK(ap_code(2u << shift, i, j, R) == 2u && ap_code(1u << shift, i, j, R) == 1u && ap_code(~(3u << shift), i, j, R) == 0u, "code");
                }
        }
    }
    CHECK(ap_trace_words((u32)PRF_AL_MAX_LEN, 4) * sizeof(u32) == 128ull << 20, "a row at the limits holds 128 MiB");
    // ---- the step of the walk
    {
        u32 j = 0, entry = 99;
        CHECK(!ap_walk_step(2, 5, &j, &entry) && j == 4 && entry == 99, "a deletion at column 0 wraps");
        CHECK(!ap_walk_step(3, 5, &j, &entry) && j == 3, "a deletion wins over an insertion");
        CHECK(ap_walk_step(1, 5, &j, &entry) && j == 3 && entry == (3u | PRF_AP_INS), "an insertion keeps the column");
        CHECK(ap_walk_step(0, 5, &j, &entry) && j == 2 && entry == 3u, "the diagonal");
        j = 0;
        CHECK(ap_walk_step(0, 1, &j, &entry) && j == 0 && entry == 0u, "k = 1");
    }
    // ---- the dealer: one row per batch, several rows, an oversized row
    u64 n_batches = 0;
    {
        std::vector<ap_row> rows;
        for (u32 i = 0; i < 40; i++) rows.push_back(ap_row{0, 16, 0, 3, i, ~0ull, 0});          // regime 0: 64 words each
        n_batches += check_deal(rows, 64, 40);
        n_batches += check_deal(rows, 65, 40);
        n_batches += check_deal(rows, 64 * 7, 6);
        n_batches += check_deal(rows, 1ull << 40, 1);
        n_batches += check_deal(rows, 1, 40);                                                  // every row is oversized
        rows[17] = ap_row{0, 300, 0, 1000, 17, ~0ull, 0};                                       // 300 groups of regime 4
        n_batches += check_deal(rows, 64 * 8, 3 + 1 + 3);
        rows.clear();
        n_batches += check_deal(rows, 64, 0) + 0;
        std::vector<ap_batch> none;
        ap_deal(rows, 64, none);
        CHECK(none.empty(), "no rows, no batches");
        for (u32 i = 0; i < 500; i++) {
            const u32 len = 1 + (u32)(rnd() % 400);
            rows.push_back(ap_row{5, 5ull + len, 0, 1 + (u32)(rnd() % 1024), i, ~0ull, 0});
        }
        for (u64 budget : {1ull, 64ull, 1000ull, 6400ull, 100000ull}) n_batches += check_deal(rows, budget, 0);
    }
    // ---- the wave against the reference
    u64 n_rows = 0, cells = 0;
    const u32 ks[] = {1, 2, 3, 5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024};
    const u32 ns[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65};
    for (u32 round = 0; round < 300; round++) {
        const u32 k = round < 20 ? ks[round] : round < 40 ? ks[round - 20] : round < 220 ? 1 + (u32)(rnd() % 80) : 1 + (u32)(rnd() % 1024);
        const u32 n = round < 20 ? ns[round % 11] : round < 40 ? k + 1 + round % 3 : k > 300 ? 1 + (u32)(rnd() % 40) : 1 + (u32)(rnd() % (2 * k + 70));
        std::string letters(k, 'A');
        std::vector<u32> motif(k);
        const u32 alphabet = round % 5 == 0 ? 2 : 4;                           // few letters: many ties
        for (u32 j = 0; j < k; j++) {
            const bool none = round % 4 == 1 && rnd() % 9 == 0;
            const u32 code = (u32)(rnd() % alphabet);
            letters[j] = none ? "Nn"[rnd() & 1] : (rnd() & 1 ? "ACGT" : "acgt")[code];
            motif[j] = none ? 5u : code;
        }
        // copies of the motif from a random phase, with substitutions, insertions, deletions and N; or random bases
        std::vector<u32> seq;
        u32 col = (u32)(rnd() % k);
        const u32 noise = round % 3 == 2 ? 2 : 1 + (u32)(rnd() % 12);
        while (seq.size() < n) {
            const u32 what = (u32)(rnd() % (8 * noise));
            if (round % 7 == 6) seq.push_back((u32)(rnd() % 5));
            else if (what == 0) seq.push_back((u32)(rnd() % alphabet)), col = (col + 1) % k;
            else if (what == 1) seq.push_back((u32)(rnd() % alphabet));
            else if (what == 2) col = (col + 1 + (u32)(rnd() % 3)) % k;
            else if (what == 3) seq.push_back(4u), col = (col + 1) % k;
            else seq.push_back(motif[col] == 5u ? 4u : motif[col]), col = (col + 1) % k;
        }
        const answer got = run(seq, letters), want = reference(seq, motif);
        CHECK(same(got.al, want.al), "k %u n %u: (%u %u %u %u %u), the reference has (%u %u %u %u %u)", k, n, got.al.edits, got.al.indels, got.al.consumed,
              got.al.start_column, got.al.end_column, want.al.edits, want.al.indels, want.al.consumed, want.al.start_column, want.al.end_column);
        CHECK(got.deletions == want.deletions, "k %u n %u: %llu deletions, the reference has %llu", k, n, (unsigned long long)got.deletions,
              (unsigned long long)want.deletions);
        for (u32 i = 0; i < n; i++)
            if (got.path[i] != want.path[i]) {
                CHECK(false, "k %u n %u position %u: entry %x, the reference has %x", k, n, i, got.path[i], want.path[i]);
                break;
            }
        // what the path must add up to
        u64 n_ins = 0;
        for (u32 e : want.path) n_ins += (e & PRF_AP_INS) ? 1 : 0;
        CHECK(n_ins + want.deletions == want.al.indels && n - n_ins + want.deletions == want.al.consumed, "k %u n %u: the path's sums", k, n);
        CHECK(!(want.path[0] & PRF_AP_INS) && (want.path[0] & PRF_AP_COLUMN) == want.al.start_column, "k %u n %u: the first entry", k, n);
        ++n_rows;
        cells += (u64)k * n;
    }
    if (failures) return 1;
    printf("ok %llu %llu %llu\n", (unsigned long long)n_rows, (unsigned long long)cells, (unsigned long long)n_batches);
    return 0;
}
