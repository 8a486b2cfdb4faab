// periodlink_step_check.cpp -- the junction arithmetic of csrc/periodlink_step.h (the lanes' shifts, the stretches of steps A and
// B, the packed key, Y's lane) with the walks of csrc/dotlink_walk.h, compiled for the host, against a brute force on
// random bands with planted junctions.  A stand-alone program: tests/test_periodlink_cpu.py builds it with the sanitizers and runs
// it.  Prints "ok <bands> <heads> <links> <shifts seen> <links with an overlap> <heads at a line's start or end>" and returns 0,
// or says what differs and returns 1.
//
// A band is the lines k = 1 .. n - 1 of a range of n positions, line k a vector of n - k cells (raw or not): lines of different
// lengths, independent of each other (more than a sequence can give).  Brute force: per line the maximal runs, the seeds, the
// chains as (first cell, last cell); for a head Y every chain of the 2 max_shift neighbouring lines is tried as X by the
// definition's words (include/prf_periodlink.h), the smallest key must be unique; the same for succ(X); a link iff mutual.
// The steps see a line as 64-cell words through line(k, wk), 0 behind the line's end; a wave is 64 calls and a minimum.
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "../colab-repeat-finder_amd/csrc/periodlink_step.h"

namespace {

u64 rng_state = 0x9E3779B97F4A7C15ull;
u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

struct span {
    long long first, last;
};
typedef std::tuple<long long, long long, long long, int> jkey;   // (m + |s|, |s|, o, s < 0)

std::vector<span> chains_of(const std::vector<char> &cells, u64 min_seed, u32 max_gap) {
    std::vector<span> out;
    const long long n = (long long)cells.size();
    for (long long s = 0; s < n;) {
        if (!cells[s]) {
            ++s;
            continue;
        }
        long long e = s;
        while (e + 1 < n && cells[e + 1]) ++e;
        if ((u64)(e - s + 1) >= min_seed) {
            if (!out.empty() && s - out.back().last - 1 <= (long long)max_gap) out.back().last = e;
            else out.push_back(span{s, e});
        }
        s = e + 1;
    }
    return out;
}

struct band {
    long long n;
    std::vector<std::vector<char>> cells;        // [k], k = 1 .. n - 1; [0] unused
    std::vector<std::vector<u64>> words;
    std::vector<std::vector<span>> chains;
};

bool key_of(const pl_params &p, long long k_x, long long t_e, long long k_y, long long t_s, jkey *key) {
    const long long s = k_y - k_x, a = s < 0 ? -s : s;
    if (a < 1 || a > (long long)p.max_shift) return false;
    const long long gi = t_s - t_e - 1, gc = gi + s, g = gi < gc ? gi : gc;
    const long long ov = (long long)(p.min_seed - 1 < 16 ? p.min_seed - 1 : 16);
    if (g < -ov || g > (long long)p.max_gap) return false;
    *key = jkey(( g > 0 ? g : 0) + a, a, g < 0 ? -g : 0, s < 0);
    return true;
}

// the best partner of the chain `me` of line k: forward: succ (me is X), otherwise pred (me is Y); false: none.  *bad: a tie
bool best(const band &b, const pl_params &p, long long k, const span &me, bool forward, jkey *key, long long *line, span *who, bool *bad) {
    bool any = false;
    for (long long other = k - (long long)p.max_shift; other <= k + (long long)p.max_shift; other++) {
        if (other == k || other < 1 || other > b.n - 1) continue;
        for (const span &c : b.chains[other]) {
            jkey got;
            if (!(forward ? key_of(p, k, me.last, other, c.first, &got) : key_of(p, other, c.last, k, me.first, &got))) continue;
            if (any && got == *key) *bad = true;
            if (!any || got < *key) *key = got, *line = other, *who = c, *bad = false;
            any = true;
        }
    }
    return any;
}

}  // namespace

int main() {
    u64 bands = 0, heads = 0, links = 0, with_overlap = 0, at_edges = 0;
    u64 seen[65] = {0};                                           // links per shift -32 .. 32
    for (int round = 0; round < 140; round++) {
        band b;
        b.n = round % 4 == 1 ? 900 + (long long)(rnd() % 300) : 40 + (long long)(rnd() % (round % 5 == 0 ? 700 : 200));
        const u64 min_seed = round < 70 ? 1 + (u64)round : 1 + rnd() % 12;     // 1 .. 70, every value; then short seeds: dense bands
        const u32 gaps_at[] = {0, 1, 2, 5, 8, 16, 47, 63, 64, 65, 300};
        const u32 max_gap = gaps_at[rnd() % 11];
        const u32 max_shift = round % 2 == 0 || round % 4 == 1 ? 32u : 1u + (u32)(rnd() % 32);
        const pl_params p{(u64)b.n, min_seed, max_gap, max_shift};
        const long long ov = (long long)(min_seed - 1 < 16 ? min_seed - 1 : 16);
        b.cells.resize(b.n);
        // per cent of raw cells; in a dense band a near line always offers a smaller key than a far one: every fourth band is
        // empty but for its planted junctions, so that those of 20 and more lines' shift are links
        const unsigned density = round % 4 == 1 ? 0 : 55 + rnd() % 44;
        for (long long k = 1; k < b.n; k++) {
            b.cells[k].resize(b.n - k);
            for (char &c : b.cells[k]) c = rnd() % 100 < density;
        }
        // planted junctions: X ends on line k - s, Y starts on line k, clean cells around.  A dense band gets 64 of them, g anywhere
        // in [-ov - 1, max_gap + 1]; an empty one gets 8 candidates 100 lines apart with room for both chains, so that over the
        // empty bands every shift -32 .. -1, 1 .. 32 is a link several times
        const bool sparse = round % 4 == 1;
        for (int plant = 0; plant < (sparse ? 8 : 64); plant++) {
            const int nth = sparse ? (round / 4 * 8 + plant) % 64 : (int)(rnd() % 64);
            const long long s = nth < 32 ? nth - 32 : nth - 31;
            const long long k_y = sparse ? 40 + 100ll * plant : 1 + (long long)(rnd() % (b.n - 1)), k_x = k_y - s;
            if (k_x < 1 || k_x > b.n - 1) continue;
            const long long len = (long long)min_seed + (long long)(rnd() % 20);
            const long long g = sparse ? (long long)(rnd() % (max_gap + ov + 1)) - ov : (long long)(rnd() % (max_gap + ov + 3)) - ov - 1;
            const long long t_e = len + (long long)(rnd() % (b.n / (sparse ? 8 : 2)));   // X = t_e - len + 1 .. t_e
            const long long t_s = g + t_e + 1 - (s < 0 ? s : 0);                   // g = min(gi, gi + s)
            std::vector<char> &lx = b.cells[k_x], &ly = b.cells[k_y];
            for (long long t = t_e - len - (long long)max_gap - 2; t <= t_e + (long long)max_gap + 2; t++)
                if (t >= 0 && t < (long long)lx.size()) lx[t] = t > t_e - len && t <= t_e;
            for (long long t = t_s - (long long)max_gap - 2; t <= t_s + len + (long long)max_gap + 1; t++)
                if (t >= 0 && t < (long long)ly.size()) ly[t] = t >= t_s && t < t_s + len;
        }
        b.words.resize(b.n);
        b.chains.resize(b.n);
        for (long long k = 1; k < b.n; k++) {
            b.words[k].assign((b.cells[k].size() + 63) / 64, 0);
            for (size_t t = 0; t < b.cells[k].size(); t++)
                if (b.cells[k][t]) b.words[k][t >> 6] |= 1ull << (t & 63);
            b.chains[k] = chains_of(b.cells[k], min_seed, max_gap);
        }
        u64 asked_outside = 0;
        const auto line = [&](u64 k, u64 wk) {
            if (k < 1 || k > (u64)b.n - 1) return ++asked_outside, 0ull;       // a lane on a line that takes no part
            return wk < b.words[k].size() ? b.words[k][wk] : 0ull;
        };
        for (long long k = 1; k < b.n; k++) {
            for (const span &y : b.chains[k]) {
                // ---- the brute force
                jkey key{}, back{};
                long long k_x = 0, k_back = 0;
                span x{}, y_back{};
                bool bad = false, linked = false;
                if (best(b, p, k, y, false, &key, &k_x, &x, &bad)) {
                    if (bad) return printf("round %d: two candidates of one key into (%lld, %lld)\n", round, k, y.first), 1;
                    if (!best(b, p, k_x, x, true, &back, &k_back, &y_back, &bad)) return printf("round %d: X without a candidate\n", round), 1;
                    if (bad) return printf("round %d: two candidates of one key out of (%lld, %lld)\n", round, k_x, x.last), 1;
                    linked = k_back == k && y_back.first == y.first;
                }
                // ---- the wave: 64 lanes, a minimum, 64 lanes, a minimum
                u32 keys[64], best_key = PL_NO_KEY;
                u64 x_end[64] = {0};
                for (u32 lane = 0; lane < 64; lane++) {
                    keys[lane] = pl_step_a(p, (u64)y.first, (u64)k, lane, line, &x_end[lane]);
                    if (keys[lane] < best_key) best_key = keys[lane];
                }
                bool got = false;
                u64 t_e = 0;
                long long got_k_x = 0;
                if (best_key != PL_NO_KEY) {
                    const u32 y_lane = pl_key_lane(best_key);
                    if (y_lane >= 64 || keys[y_lane] != best_key) return printf("round %d: the key %x does not name its lane\n", round, best_key), 1;
                    t_e = x_end[y_lane];
                    got_k_x = k - pl_key_shift(best_key);
                    u32 next = PL_NO_KEY;
                    bool is_y[64] = {false};
                    for (u32 lane = 0; lane < 64; lane++) {
                        const u32 kb = pl_step_b(p, t_e, (u64)got_k_x, lane, best_key, (u64)y.first, line, &is_y[lane]);
                        if (kb < next) next = kb;
                    }
                    got = next == best_key && is_y[y_lane];
                }
                // ---- compare
                const bool has_pred = k_x != 0;
                if (has_pred != (best_key != PL_NO_KEY))
                    return printf("round %d: head (%lld, %lld): pred %s, the brute force %s (n %lld, min_seed %llu, max_gap %u, max_shift %u)\n", round, k,
                                  y.first, best_key != PL_NO_KEY ? "found" : "none", has_pred ? "has one" : "has none", b.n, min_seed, max_gap, max_shift), 1;
                if (has_pred) {
                    const u32 want = pl_key((long long)std::get<2>(key) ? -std::get<2>(key) : std::get<0>(key) - std::get<1>(key), (u32)std::get<1>(key),
                                            std::get<3>(key) != 0);
                    if (want != best_key || got_k_x != k_x || (long long)t_e != x.last)
                        return printf("round %d: head (%lld, %lld): pred (%lld, %llu) key %x, the brute force (%lld, %lld) key %x\n", round, k, y.first,
                                      got_k_x, t_e, best_key, k_x, x.last, want), 1;
                    if (pl_key_most(best_key) - pl_key_abs_shift(best_key) != (u32)(std::get<0>(key) - std::get<1>(key)) ||
                        pl_key_overlap(best_key) != (u32)std::get<2>(key) || pl_key_shift(best_key) != (int)(k - k_x))
                        return printf("round %d: the key %x unpacks wrongly\n", round, best_key), 1;
                }
                if (got != linked)
                    return printf("round %d: head (%lld, %lld): link %d, the brute force %d (n %lld, min_seed %llu, max_gap %u, max_shift %u)\n", round, k,
                                  y.first, (int)got, (int)linked, b.n, min_seed, max_gap, max_shift), 1;
                ++heads;
                if (linked) {
                    ++links;
                    ++seen[k - k_x + 32];
                    with_overlap += std::get<2>(key) != 0;
                }
                at_edges += y.first == 0 || y.last == (long long)b.cells[k].size() - 1;
            }
        }
        if (asked_outside) return printf("round %d: %llu words asked of lines below 1 or above n - 1\n", round, asked_outside), 1;
        ++bands;
    }
    u64 shifts = 0;
    for (int s = 0; s < 65; s++) shifts += s != 32 && seen[s] > 0;
    printf("ok %llu %llu %llu %llu %llu %llu\n", bands, heads, links, shifts, with_overlap, at_edges);
    return 0;
}
