// align_word_check.cpp -- the per-lane text of the alignment kernel (csrc/align_word.h: the packing of a cell, the deal of the
// columns, al_lane_scan, al_lane_wrap, the final pick, the host's sort), compiled for the host.  A stand-alone
// program: tests/test_align_cpu.py builds it with the sanitizers and runs it.  Prints "ok <deals> <rows> <cells>" and returns 0, or
// says what differs and returns 1.
//
// The 64 lanes of a wave are run one after the other; what the kernel does across lanes (the diagonal term of a lane's first
// column, the prefix minimum over the lanes' totals, the broadcast of the last column's cell) is done here on arrays, in the same
// order.  The reference is the recurrence on explicit triples, column by column, with two plain passes over the columns.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/align_word.h"

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

// bases 0 .. 3, 4 for none; motif codes 0 .. 3, 5 for N
al_result reference(const std::vector<u32> &seq, const std::vector<u32> &motif) {
    const u32 k = (u32)motif.size();
    std::vector<triple> D(k, triple{0, 0, 0}), P(k);
    for (u32 b : seq) {
        for (u32 j = 0; j < k; j++)
            P[j] = std::min(add(D[(j + k - 1) % k], motif[j] == b ? 0u : 1u, 0, 1), add(D[j], 1, 1, 0));
        for (u32 j = 1; j < k; j++) P[j] = std::min(P[j], add(P[j - 1], 1, 1, 1));
        const triple last = P[k - 1];
        for (u32 j = 0; j < k; j++) D[j] = std::min(P[j], add(last, j + 1, j + 1, j + 1));
    }
    u32 col = 0;
    for (u32 j = 1; j < k; j++)
        if (D[j] < D[col]) col = j;
    const u32 consumed = std::get<2>(D[col]);
    return al_result{std::get<0>(D[col]), std::get<1>(D[col]), consumed, (u32)(((long long)col + 1 - consumed) % k + k) % k, col, 0};
}

template <int C>
al_result wave(const std::vector<u32> &seq, const std::string &letters) {
    const u32 k = (u32)letters.size();
    std::array<std::array<u64, C>, 64> D, U;
    u32 real[64];
    u64 bias0[64], codes[64], inc[64];
    const u32 lanes = al_real_lanes(k, C);
    for (u32 lane = 0; lane < 64; lane++) {
        real[lane] = al_real_slots(k, C, lane);
        bias0[lane] = real[lane] ? al_bias(k, lane * C) : 0;
        codes[lane] = al_lane_codes<C>(letters.data(), k, lane);
        al_lane_open<C>(D[lane].data(), real[lane]);
    }
    u64 last = 0;
    for (u32 b : seq) {
        u64 up[64];
        for (u32 lane = 0; lane < 64; lane++) up[lane] = lane ? D[lane - 1][C - 1] : last;
        for (u32 lane = 0; lane < 64; lane++) inc[lane] = al_lane_scan<C>(D[lane].data(), up[lane], b, codes[lane], real[lane], bias0[lane], U[lane].data());
        for (u32 d = 1; d < lanes; d <<= 1)                                   // the steps of the kernel's scan, all lanes at once
            for (u32 lane = 63; lane >= d; lane--) inc[lane] = al_min(inc[lane], inc[lane - d]);
        last = inc[lanes - 1];
        for (u32 lane = 0; lane < 64; lane++)
            al_lane_wrap<C>(U[lane].data(), lane ? inc[lane - 1] : AL_SENTINEL, last, real[lane], bias0[lane], lane * C, D[lane].data());
        for (u32 lane = 0; lane < 64; lane++)
            for (u32 c = 0; c < (u32)C; c++) {
                const bool is_real = lane * C + c < k;
                CHECK(is_real ? D[lane][c] < (1ull << 61) : D[lane][c] == AL_SENTINEL, "k %u lane %u slot %u holds %llx", k, lane, c, (unsigned long long)D[lane][c]);
            }
        CHECK(last == D[al_lane_of(k - 1, C)][al_slot_of(k - 1, C)], "k %u: the broadcast value is not the cell of column k - 1", k);
    }
    u64 best = AL_SENTINEL;
    u32 best_col = 0xFFFFFFFFu;
    for (u32 lane = 64; lane-- > 0;) {                                        // any order: the tie rule decides
        u64 v;
        u32 col;
        al_lane_pick<C>(D[lane].data(), real[lane], lane * C, &v, &col);
        al_pick(&best, &best_col, v, col);
    }
    return al_finish(best, best_col, k);
}

al_result run(const std::vector<u32> &seq, const std::string &letters) {
    switch (al_regime((u32)letters.size())) {
    case 0: return wave<1>(seq, letters);
    case 1: return wave<2>(seq, letters);
    case 2: return wave<4>(seq, letters);
    case 3: return wave<8>(seq, letters);
    default: return wave<16>(seq, letters);
    }
}

bool same(const al_result &a, const al_result &b) {
    return a.edits == b.edits && a.indels == b.indels && a.consumed == b.consumed && a.start_column == b.start_column &&
           a.end_column == b.end_column && !a.reserved && !b.reserved;
}

}  // namespace

int main() {
    // ---- the deal: every column in exactly one (lane, slot), the rest padded
    u64 deals = 0;
    for (u32 k = 1; k <= PRF_AL_MAX_K; k++) {
        const u32 C = 1u << al_regime(k);
        CHECK(k <= 64 * C && (C == 1 || k > 32 * C), "k %u has C %u", k, C);
        std::vector<u32> seen(64 * C, 0);
        for (u32 j = 0; j < k; j++) {
            const u32 lane = al_lane_of(j, C), slot = al_slot_of(j, C);
            CHECK(lane < 64 && slot < C && lane * C + slot == j, "k %u column %u", k, j);
            ++seen[lane * C + slot];
        }
        u32 total = 0;
        for (u32 lane = 0; lane < 64; lane++) {
            const u32 real = al_real_slots(k, C, lane);
            total += real;
            for (u32 c = 0; c < C; c++) CHECK(seen[lane * C + c] == (c < real ? 1u : 0u), "k %u lane %u slot %u", k, lane, c);
            CHECK((real > 0) == (lane < al_real_lanes(k, C)), "k %u lane %u", k, lane);
            if (real) CHECK(al_bias(k, lane * C) == (u64)(k - 1 - lane * C) * AL_DEL, "bias");
        }
        CHECK(total == k, "k %u deals %u columns", k, total);
        ++deals;
    }
    CHECK(al_bias(1024, 1023) == 0 && al_wrap(1023) == 1024 * AL_DEL, "the last column");
    // ---- the cells at the limits
    const u32 max_e = (u32)PRF_AL_MAX_LEN, max_c = 2 * (u32)PRF_AL_MAX_LEN;
    for (u32 e : {0u, 1u, max_e - 1, max_e})
        for (u32 i : {0u, 1u, max_e})
            for (u32 c : {0u, 1u, max_c}) {
                const u64 v = al_pack(e, i, c);
                CHECK(al_edits(v) == e && al_indels(v) == i && al_consumed(v) == c, "pack %u %u %u", e, i, c);
                // one step and a bias or a wrap of k (1, 1, 1) on top: no field carries, the sentinel stays above
                const u64 w = v + AL_DEL + PRF_AL_MAX_K * AL_DEL;
                CHECK(al_edits(w) == e + 1025 && al_indels(w) == i + 1025 && al_consumed(w) == c + 1025 && w < (1ull << 61), "carry at %u %u %u", e, i, c);
                CHECK(w < AL_SENTINEL && w - PRF_AL_MAX_K * AL_DEL == v + AL_DEL, "bias off again");
            }
    CHECK(al_pack(1, 0, 0) > al_pack(0, max_e, max_c) && al_pack(0, 1, 0) > al_pack(0, 0, max_c), "the order of the fields");
    u64 s = AL_SENTINEL;
    for (u64 i = 0; i < PRF_AL_MAX_LEN + 2 * PRF_AL_MAX_K; i++) s += AL_DEL;
    CHECK(s >= AL_SENTINEL && s < (1ull << 63), "the sentinel after 2^19 + 2048 steps");
    // ---- the tie rule
    {
        u64 best = AL_SENTINEL;
        u32 col = 0xFFFFFFFFu;
        al_pick(&best, &col, 7, 9);
        al_pick(&best, &col, 7, 3);
        al_pick(&best, &col, 7, 5);
        al_pick(&best, &col, 8, 0);
        CHECK(best == 7 && col == 3, "ties go to the first column");
        al_pick(&best, &col, 6, 11);
        CHECK(best == 6 && col == 11, "a smaller cell wins");
        const al_result r = al_finish(al_pack(2, 1, 10), 1, 4);
        CHECK(r.edits == 2 && r.indels == 1 && r.consumed == 10 && r.end_column == 1 && r.start_column == 0, "finish");
    }
    // ---- the host's sort: by regime, the longest first, stable; the indices follow
    {
        std::vector<al_row> rows;
        for (u32 i = 0; i < 3000; i++) {
            const u32 k = 1 + (u32)(rnd() % 1024), len = 1 + (u32)(rnd() % 500);
            const u64 start = rnd() % 100000;
            rows.push_back(al_row{start, start + len, 0, k, i});
        }
        const std::vector<al_row> before = rows;
        u64 per[PRF_AL_REGIMES];
        al_sort_rows(rows, per);
        u64 sum = 0;
        for (u32 r = 0; r < PRF_AL_REGIMES; r++) sum += per[r];
        CHECK(sum == rows.size(), "the regimes' counts");
        std::vector<u32> seen(rows.size(), 0);
        u64 at = 0;
        for (u32 r = 0; r < PRF_AL_REGIMES; r++)
            for (u64 i = 0; i < per[r]; i++, at++) {
                const al_row &x = rows[at];
                CHECK(al_regime(x.k) == r, "row %llu in regime %u", (unsigned long long)at, r);
                if (i) {
                    const al_row &p = rows[at - 1];
                    CHECK(p.end - p.start > x.end - x.start || (p.end - p.start == x.end - x.start && p.index < x.index), "order at %llu", (unsigned long long)at);
                }
                ++seen[x.index];
                CHECK(before[x.index].start == x.start && before[x.index].end == x.end && before[x.index].k == x.k, "row %u changed", x.index);
            }
        for (u32 v : seen) CHECK(v == 1, "every row once");
    }
    // ---- the wave against the reference
    u64 n_rows = 0, cells = 0;
    const u32 ks[] = {1, 2, 3, 5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024};
    for (u32 round = 0; round < 260; round++) {
        const u32 k = round < 20 ? ks[round] : round < 200 ? 1 + (u32)(rnd() % 80) : 1 + (u32)(rnd() % 1024);
        const u32 n = k > 300 ? 1 + (u32)(rnd() % 40) : 1 + (u32)(rnd() % (2 * k + 70));
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
        const al_result got = run(seq, letters), want = reference(seq, motif);
        CHECK(same(got, want), "k %u n %u: (%u %u %u %u %u), the reference has (%u %u %u %u %u)", k, n, got.edits, got.indels, got.consumed,
              got.start_column, got.end_column, want.edits, want.indels, want.consumed, want.start_column, want.end_column);
        ++n_rows;
        cells += (u64)k * n;
    }
    if (failures) return 1;
    printf("ok %llu %llu %llu\n", (unsigned long long)deals, (unsigned long long)n_rows, (unsigned long long)cells);
    return 0;
}
