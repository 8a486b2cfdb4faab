// alignlocal_word_check.cpp -- the per-lane text of the local alignment kernel (csrc/alignlocal_word.h: the packing of a cell, the
// saturating subtraction, the fresh-start label, all_lane_scan, all_lane_wrap, the running best and the final pick), compiled for
// the host.  A stand-alone program: tests/test_alignlocal_cpu.py builds it with the sanitizers and runs it.  Prints
// "ok <packs> <rows> <cells>" and returns 0, or says what differs and returns 1.
//
// The 64 lanes of a wave are run one after the other; what the kernel does across lanes (the diagonal term of a lane's first
// column, the prefix maximum over the lanes' totals, the broadcast of the last column's cell, the butterfly of the best) is done
// here on arrays, in the same order.  The reference is the recurrence on explicit triples on a full matrix, column by column.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/alignlocal_word.h"

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

using triple = std::tuple<u32, u32, u32>;    // (score, p, a)
const triple ZERO{0, 0, 0};
triple sub(const triple &v, u32 w) { return std::get<0>(v) > w ? triple{std::get<0>(v) - w, std::get<1>(v), std::get<2>(v)} : ZERO; }

struct weights3 {
    u32 match, mismatch, indel;
};

// bases 0 .. 3, 4 for none; motif codes 0 .. 3, 5 for N.  Every cell of the matrix is kept.
all_result reference(const std::vector<u32> &seq, const std::vector<u32> &motif, const weights3 &w) {
    const u32 k = (u32)motif.size(), n = (u32)seq.size();
    std::vector<std::vector<triple>> cells(n + 1, std::vector<triple>(k, ZERO));
    std::vector<triple> T(k), P(k);
    triple best = ZERO;
    u32 best_end = 0, best_col = 0;
    for (u32 i = 0; i < n; i++) {
        const std::vector<triple> &D = cells[i];
        for (u32 j = 0; j < k; j++) {
            triple din = D[(j + k - 1) % k];
            if (!std::get<0>(din)) din = triple{0, i, j};
            const triple step = motif[j] == seq[i] ? triple{std::get<0>(din) + w.match, std::get<1>(din), std::get<2>(din)} : sub(din, w.mismatch);
            T[j] = std::max(step, sub(D[j], w.indel));
        }
        P[0] = T[0];
        for (u32 j = 1; j < k; j++) P[j] = std::max(T[j], sub(P[j - 1], w.indel));
        for (u32 j = 0; j < k; j++) {
            cells[i + 1][j] = std::max(P[j], sub(P[k - 1], (j + 1) * w.indel));
            if (std::get<0>(cells[i + 1][j]) > std::get<0>(best)) best = cells[i + 1][j], best_end = i + 1, best_col = j;
        }
    }
    if (!std::get<0>(best)) return all_result{0, 0, 0, 0, 0, 0};
    return all_result{std::get<0>(best), std::get<1>(best), best_end, std::get<2>(best), best_col, 0};
}

template <int C>
all_result wave(const std::vector<u32> &seq, const std::string &letters, const weights3 &w3) {
    const u32 k = (u32)letters.size();
    const all_weights w = all_weights_of(w3.match, w3.mismatch, w3.indel);
    std::array<std::array<u64, C>, 64> D, U;
    u32 real[64];
    u64 bias0[64], codes[64], inc[64];
    all_best best[64];
    const u32 lanes = al_real_lanes(k, C);
    for (u32 lane = 0; lane < 64; lane++) {
        real[lane] = al_real_slots(k, C, lane);
        bias0[lane] = (u64)(lane * C) * w.indel;
        codes[lane] = al_lane_codes<C>(letters.data(), k, lane);
        D[lane].fill(0);
        best[lane] = all_best{0, 0};
    }
    u64 last = 0;
    for (u32 i = 0; i < seq.size(); i++) {
        const u32 b = seq[i];
        u64 up[64];
        for (u32 lane = 0; lane < 64; lane++) up[lane] = lane ? D[lane - 1][C - 1] : last;
        for (u32 lane = 0; lane < 64; lane++)
            inc[lane] = all_lane_scan<C>(D[lane].data(), up[lane], b, codes[lane], real[lane], bias0[lane], all_fresh(i, lane * C), w, U[lane].data());
        for (u32 d = 1; d < lanes; d <<= 1)                                   // the steps of the kernel's scan, all lanes at once
            for (u32 lane = 63; lane >= d; lane--) inc[lane] = all_max(inc[lane], inc[lane - d]);
        CHECK(inc[lanes - 1] >= (u64)(k - 1) * w.indel, "k %u: the total is below the bias of column k - 1", k);
        last = all_last(inc[lanes - 1], k, w);
        for (u32 lane = 0; lane < 64; lane++)
            all_lane_wrap<C>(U[lane].data(), lane ? inc[lane - 1] : 0ull, last, real[lane], bias0[lane], w, D[lane].data());
        for (u32 lane = 0; lane < 64; lane++) {
            for (u32 c = 0; c < (u32)C; c++) {
                const bool is_real = lane * C + c < k;
                CHECK(is_real ? D[lane][c] < (1ull << 54) && all_score(D[lane][c]) <= (i + 1) * w3.match : D[lane][c] == 0,
                      "k %u lane %u slot %u holds %llx", k, lane, c, (unsigned long long)D[lane][c]);
            }
            all_lane_best<C>(D[lane].data(), all_where(i, lane * C), &best[lane]);
        }
        CHECK(last == D[al_lane_of(k - 1, C)][al_slot_of(k - 1, C)], "k %u: the broadcast value is not the cell of column k - 1", k);
    }
    for (u32 d = 32; d; d >>= 1) {                                            // the butterfly
        all_best other[64];
        for (u32 lane = 0; lane < 64; lane++) other[lane] = best[lane ^ d];
        for (u32 lane = 0; lane < 64; lane++) all_pick(&best[lane], other[lane].key, other[lane].cell);
    }
    for (u32 lane = 1; lane < 64; lane++) CHECK(best[lane].key == best[0].key && best[lane].cell == best[0].cell, "the butterfly leaves lane %u apart", lane);
    return all_finish(best[0]);
}

all_result run(const std::vector<u32> &seq, const std::string &letters, const weights3 &w) {
    switch (al_regime((u32)letters.size())) {
    case 0: return wave<1>(seq, letters, w);
    case 1: return wave<2>(seq, letters, w);
    case 2: return wave<4>(seq, letters, w);
    case 3: return wave<8>(seq, letters, w);
    default: return wave<16>(seq, letters, w);
    }
}

bool same(const all_result &a, const all_result &b) {
    return a.score == b.score && a.first == b.first && a.end == b.end && a.start_column == b.start_column && a.end_column == b.end_column &&
           !a.reserved && !b.reserved;
}

}  // namespace

int main() {
    // ---- the cells at the field maxima: score 2^23 plus the largest bias, p = 2^19 - 1, a = 1023
    u64 packs = 0;
    const u32 max_score = PRF_ALL_MAX_WEIGHT * (u32)PRF_AL_MAX_LEN, max_bias = (PRF_AL_MAX_K - 1u) * PRF_ALL_MAX_WEIGHT;
    CHECK(max_score == 1u << 23 && max_bias < 1u << 14, "the maxima");
    for (u32 s : {0u, 1u, 16u, 17u, max_score - 1, max_score})
        for (u32 p : {0u, 1u, (u32)PRF_AL_MAX_LEN - 1})
            for (u32 a : {0u, 1u, PRF_AL_MAX_K - 1}) {
                const u64 v = all_pack(s, p, a);
                CHECK(all_score(v) == s && all_p(v) == p && all_a(v) == a, "pack %u %u %u", s, p, a);
                const u64 biased = v + all_weight(max_bias) + all_weight(PRF_ALL_MAX_WEIGHT);    // a step and the largest bias on top
                CHECK(all_score(biased) == s + max_bias + PRF_ALL_MAX_WEIGHT && all_p(biased) == p && all_a(biased) == a && biased < (1ull << 54),
                      "carry at %u %u %u", s, p, a);
                CHECK(biased - all_weight(max_bias) == v + all_weight(PRF_ALL_MAX_WEIGHT), "bias off again");
                // sub at score == w and at score == w + 1, with the labels at their maxima
                for (u32 w = 1; w <= PRF_ALL_MAX_WEIGHT; w++) {
                    CHECK(all_sub(all_pack(w, p, a), all_weight(w)) == 0, "sub at score == w = %u", w);
                    CHECK(all_sub(all_pack(w + 1, p, a), all_weight(w)) == all_pack(1, p, a), "sub at score == w + 1 = %u", w + 1);
                    CHECK(all_sub(all_pack(0, p, a), all_weight(w)) == 0 && all_sub(all_pack(w - 1, p, a), all_weight(w)) == 0, "sub below w = %u", w);
                }
                if (s > PRF_ALL_MAX_WEIGHT) CHECK(all_sub(v, all_weight(PRF_ALL_MAX_WEIGHT)) == all_pack(s - PRF_ALL_MAX_WEIGHT, p, a), "sub keeps the labels");
                // the wrap's largest subtrahend: 1024 x 16
                const u64 wrap = all_weight(PRF_AL_MAX_K * PRF_ALL_MAX_WEIGHT);
                CHECK(all_sub(v, wrap) == (s > PRF_AL_MAX_K * PRF_ALL_MAX_WEIGHT ? all_pack(s - PRF_AL_MAX_K * PRF_ALL_MAX_WEIGHT, p, a) : 0ull), "the wrap at %u", s);
                ++packs;
            }
    CHECK(all_pack(1, 0, 0) > all_pack(0, (u32)PRF_AL_MAX_LEN - 1, 1023) && all_pack(0, 1, 0) > all_pack(0, 0, 1023), "the order of the fields");
    CHECK(all_max(all_pack(5, 3, 9), all_pack(5, 4, 0)) == all_pack(5, 4, 0) && all_max(all_pack(5, 4, 7), all_pack(5, 4, 8)) == all_pack(5, 4, 8),
          "of equal scores the greatest p, then the greatest a");
    CHECK(all_fresh((u32)PRF_AL_MAX_LEN - 1, 1023) == all_pack(0, (u32)PRF_AL_MAX_LEN - 1, 1023) && all_fresh(7, 1008) + 15 == all_fresh(7, 1023), "the fresh label");
    // ---- the stale label of the prefix pass: a cell of score 0 with another column's label behaves as 0
    {
        const all_weights w = all_weights_of(2, 7, 7);
        const u64 stale = all_pack(0, 77, 5);
        CHECK(all_sub(stale, w.indel) == 0 && all_sub(stale, w.mismatch) == 0, "sub drops a stale label");
        // one lane, C = 4, k = 4, motif ACGT, base A: column 0 matches with score 7 from a diagonal of 5; one deletion behind it costs
        // all of it, so P[1] has score 0 and keeps the label (3, 2) of column 0: stale
        u64 D[4] = {0, 0, 0, 0}, U[4];
        const u64 codes = al_lane_codes<4>("ACGT", 4, 0);
        const u64 total = all_lane_scan<4>(D, all_pack(5, 3, 2), 0u, codes, 4, 0, all_fresh(9, 0), w, U);
        const u64 last = all_last(total, 4, w);
        all_lane_wrap<4>(U, 0, last, 4, 0, w, D);
        CHECK(D[0] == all_pack(7, 3, 2) && D[1] == all_pack(0, 3, 2), "the match, and a stale label behind it: %llx %llx", (unsigned long long)D[0], (unsigned long long)D[1]);
        CHECK(all_score(D[2]) == 0 && all_score(D[3]) == 0 && all_score(last) == 0, "more deletions cost more than the score");
        all_best best{0, 0};
        all_lane_best<4>(D, all_where(9, 0), &best);
        CHECK(all_score(best.key) == 7 && best.cell == all_pack(7, 3, 2) && best.key == all_key(best.cell, all_where(9, 0)), "the best never takes a score of 0");
        // the next position, base G: the diagonal step into column 2 comes from the stale cell and is a fresh start with its own label
        const u64 total2 = all_lane_scan<4>(D, last, 2u, codes, 4, 0, all_fresh(10, 0), w, U);
        all_lane_wrap<4>(U, 0, all_last(total2, 4, w), 4, 0, w, D);
        CHECK(D[2] == all_pack(2, 10, 2), "a fresh start takes its own label: %llx", (unsigned long long)D[2]);
        CHECK(all_score(D[0]) == 0 && all_score(D[1]) == 0 && all_score(D[3]) == 0, "the rest is 0");
    }
    // ---- the order of the best key: the score, then the earliest end, then the least column
    {
        const u64 cell = all_pack(40, 11, 2);
        CHECK(all_key(cell, all_where(5, 9)) > all_key(all_pack(39, 500, 1000), all_where(0, 0)), "the score first");
        CHECK(all_key(cell, all_where(5, 9)) > all_key(cell, all_where(6, 0)), "then the earliest end");
        CHECK(all_key(cell, all_where(5, 9)) > all_key(cell, all_where(5, 10)), "then the least column");
        CHECK(all_where(5, 1008) - 15 == all_where(5, 1023) && all_where((u32)PRF_AL_MAX_LEN - 1, 1023) == 0, "the inverted column of a slot");
        all_best best{0, 0};
        all_pick(&best, all_key(cell, all_where(5, 9)), cell);
        all_pick(&best, all_key(all_pack(40, 300, 7), all_where(5, 10)), all_pack(40, 300, 7));
        all_pick(&best, 0, 0);
        const all_result r = all_finish(best);
        CHECK(r.score == 40 && r.first == 11 && r.end == 6 && r.start_column == 2 && r.end_column == 9 && !r.reserved, "finish");
        const all_result none = all_finish(all_best{0, 0});
        CHECK(!none.score && !none.first && !none.end && !none.start_column && !none.end_column && !none.reserved, "the zero row");
        const all_result top = all_finish(all_best{all_key(all_pack(max_score, 0, 1023), all_where((u32)PRF_AL_MAX_LEN - 1, 1023)), all_pack(max_score, 0, 1023)});
        CHECK(top.score == max_score && top.first == 0 && top.end == PRF_AL_MAX_LEN && top.start_column == 1023 && top.end_column == 1023, "finish at the maxima");
    }
    // ---- the wave against the reference
    u64 n_rows = 0, cells = 0;
    const u32 ks[] = {1, 2, 3, 5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024};
    const weights3 triples[] = {{2, 7, 7}, {1, 1, 1}, {2, 3, 5}, {16, 16, 16}, {16, 1, 1}, {1, 16, 16}, {3, 1, 2}, {2, 5, 1}};
    for (u32 round = 0; round < 300; round++) {
        const u32 k = round < 40 ? ks[round % 20] : round < 220 ? 1 + (u32)(rnd() % 80) : 1 + (u32)(rnd() % 1024);
        const u32 n = k > 300 ? 1 + (u32)(rnd() % 40) : 1 + (u32)(rnd() % (2 * k + 70));
        const weights3 w = round < 20 ? weights3{1, 16, 16} : round < 40 ? weights3{16, 1, 1} : triples[round % 8];
        std::string letters(k, 'A');
        std::vector<u32> motif(k);
        const u32 alphabet = round % 5 == 0 ? 2 : 4;                           // few letters: many ties
        for (u32 j = 0; j < k; j++) {
            const bool none = round % 4 == 1 && rnd() % 9 == 0;
            const u32 code = (u32)(rnd() % alphabet);
            letters[j] = none ? "Nn"[rnd() & 1] : (rnd() & 1 ? "ACGT" : "acgt")[code];
            motif[j] = none ? 5u : code;
        }
        // a random flank, copies of the motif from a random phase with substitutions, insertions, deletions and N, a flank; or random
        std::vector<u32> seq;
        u32 col = (u32)(rnd() % k);
        const u32 noise = round % 3 == 2 ? 2 : 1 + (u32)(rnd() % 12);
        const u32 flank = n / 5;
        while (seq.size() < n) {
            const u32 what = (u32)(rnd() % (8 * noise));
            if (round % 7 == 6 || seq.size() < flank || seq.size() + flank >= n) seq.push_back((u32)(rnd() % 5));
            else if (what == 0) seq.push_back((u32)(rnd() % alphabet)), col = (col + 1) % k;
            else if (what == 1) seq.push_back((u32)(rnd() % alphabet));
            else if (what == 2) col = (col + 1 + (u32)(rnd() % 3)) % k;
            else if (what == 3) seq.push_back(4u), col = (col + 1) % k;
            else seq.push_back(motif[col] == 5u ? 4u : motif[col]), col = (col + 1) % k;
        }
        const all_result got = run(seq, letters, w), want = reference(seq, motif, w);
        CHECK(same(got, want), "k %u n %u weights %u %u %u: (%u %u %u %u %u), the reference has (%u %u %u %u %u)", k, n, w.match, w.mismatch, w.indel, got.score,
              got.first, got.end, got.start_column, got.end_column, want.score, want.first, want.end, want.start_column, want.end_column);
        ++n_rows;
        cells += (u64)k * n;
    }
    if (failures) return 1;
    printf("ok %llu %llu %llu\n", (unsigned long long)packs, (unsigned long long)n_rows, (unsigned long long)cells);
    return 0;
}
