// plan.cpp -- the work planner of the fused kernel: which wave runs which motif sizes, and how much LDS a workgroup takes.
// Pure host code without HIP headers: part of libprf.so, and built a second time with g++ -fsanitize=address,undefined
// (make asan -> libprf_host_asan.so) for the CPU suite (tests/test_asan_host.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "prf_plan.h"

using namespace prf_layout;
static constexpr int MAX_WAVES = PRF_VMAX_WAVES;

// ---------------------------------------------------------------------------------------------------
// What a task costs the wave that runs it, in cycles per tile: the median from a task's stamp to the next one's, the push of its
// answers included, on the default workload's stand-in at six workgroups per CU (make STAMPS=1, tools/stamps.py 400000000
// standin2; profiles/scan_handover/stamps_parent_*.txt: seven runs that agree within 60 cycles per task).  Measured are the
// thirteen tasks of the default plan; the rest of the table is carried over from them and says so.  A wave's first task costs
// about 300 cycles more than the same task later (k = 3: 4 340 first, 4 032 second): every wave has one first task, so that is
// a constant of the wave (FIRST_TASK), taken off the figures of the four tasks that were measured as first ones.
namespace {
constexpr u32 FIRST_TASK = 300;
constexpr u32 K1_HANDOVER = 1660;  // the derived k = 1 task on a clean tile: a word read back from LDS and pushed (1 656 - 1 664)

u32 task_price(const prf_vtask &t) {
    if (t.kind != 0) {
        if (t.pad & PRF_TASK_DERIVED) return K1_HANDOVER;
        const u32 k = t.k0, M = t.kind;
        if (M <= 8) {
            // the exact form, per (k, M): (2, 7) 3 988 - 4 016, (3, 6) 4 340 - 4 348 as a first task, (4, 8) 4 256 - 4 268 as a first
            // task; the classes that were not measured read as many slots of rows as these (10 or 11) and are priced alike
            if (k == 2 && M == 7) return 4000;
            if (k == 3 && M == 6) return 4040;
            if (k == 4 && M == 8) return 3960;
            return 4000;
        }
        // the coarse form: groups of 2 rows for M = 9, 10 ((5, 10): 3 632 - 3 636), of 4 from M = 11 on ((6, 12): 3 740 - 3 756 in the
        // middle of its wave, (7, 14): 3 436 - 3 448 as its wave's last task)
        return M <= 10 ? 3630 : 3600;
    }
    // group tasks, by stride and number of sizes.  Measured: stride 1 with 4 sizes 4 940 - 4 956 as a first task, stride 2 with 8
    // sizes 5 448 - 5 456 as a first task, stride 4 with 8 sizes 3 636 - 3 708 (three tasks), with 7 sizes 3 576 - 3 624.  A size more
    // or less is worth 100 cycles at stride 4, where one block of rows is examined; the slopes of the strides 2 and 1 (two and
    // four blocks) are that times the blocks and are NOT measured: the default plan has one task of each.
    const u32 n = (u32)__builtin_popcount((unsigned)t.valid);
    if (t.stride == 1) return 3050 + 400 * n;
    if (t.stride == 2) return 3550 + 200 * n;
    return 2900 + 100 * n;
}

// What the deal minimises.  The first two waves to leave the scan load the verify window, and their wait for the slowest wave
// hides that load: with the waves' loads sorted a1 <= a2 <= a3 <= a4 the verify phase can begin at max(a4, a2 + W'), W' being the
// time from the second wave's arrival to its window data being in registers less the code that follows the last arrival anyway
// (its arrival atomic and the barrier).  Measured (profiles/scan_handover_notes.md): W' = 1.35 k cycles -- and a deal that
// respects it buys nothing on any workload (the wait of one workgroup is issue time for the five others), while the one it
// picks for the default parameters costs chr22-real, whose kernel time is its densest tile, 9 % by the order in which the
// group tasks reach the record list.  So W' is 0 in the product: plain levelling.  A wave without tasks has load 0.
#ifdef PRF_DIAG
const u32 WINDOW_W = getenv("PRF_PLAN_W") ? (u32)strtoul(getenv("PRF_PLAN_W"), nullptr, 0) : 0u;  // (diagnostic: sweep)
#else
constexpr u32 WINDOW_W = 0;
#endif

constexpr u32 PRIO_HANDOVER = 3, PRIO_FLAGS = 2;  // (prf_vplan::prio, the fields << 12 and << 6: the best of the sweep, see prio_cfg below)

struct DealKey {  // smaller is better: the objective, then the busiest wave, then the sum of the two busiest
    u32 obj, a4, a34;
    bool operator<(const DealKey &o) const { return obj != o.obj ? obj < o.obj : (a4 != o.a4 ? a4 < o.a4 : a34 < o.a34); }
};
DealKey deal_key(const u32 (&load)[PRF_VMAX_WAVES]) {
    u32 a[PRF_VMAX_WAVES];
    std::copy(load, load + PRF_VMAX_WAVES, a);
    std::sort(a, a + PRF_VMAX_WAVES);
    return DealKey{std::max(a[PRF_VMAX_WAVES - 1], a[1] + WINDOW_W), a[PRF_VMAX_WAVES - 1], a[PRF_VMAX_WAVES - 1] + a[PRF_VMAX_WAVES - 2]};
}

// Every deal of a dozen tasks can be looked at: depth first over the tasks in order of falling cost, a task into each wave whose
// load differs from that of the waves tried before it (equal loads give the same deals), a branch given up when what is dealt
// already does no better than the best complete deal -- the loads only grow, and with them a4 and a2.  `best` comes in as the
// local search's deal, so the bound bites from the start.  The count of nodes is capped: a plan with more tasks than that
// allows keeps the best deal seen.
struct DealSearch {
    const std::vector<u32> &cost;
    std::vector<u32> where, best_where;
    u32 load[PRF_VMAX_WAVES] = {};
    DealKey best;
    long nodes = 0;
    static constexpr long MAX_NODES = 400000;
    void go(size_t i) {
        if (++nodes > MAX_NODES) return;
        const DealKey here = deal_key(load);
        if (!(here < best)) return;
        if (i == cost.size()) {
            best = here;
            best_where = where;
            return;
        }
        for (u32 w = 0; w < (u32)PRF_VMAX_WAVES; w++) {
            bool seen = false;
            for (u32 v = 0; v < w; v++) seen = seen || load[v] == load[w];
            if (seen) continue;
            load[w] += cost[i];
            where[i] = w;
            go(i + 1);
            load[w] -= cost[i];
        }
    }
};
}  // namespace

// ---------------------------------------------------------------------------------------------------
// Work plan: which wave runs which motif sizes.  Pure host code.
static bool build_plan(u32 kmin, u32 kmax, u32 min_repeats, u32 min_span, prf_vplan *plan) {
    if (kmin < 1 || kmax < kmin || kmax > PRF_VMAX_K || min_repeats < 2) return false;
    struct Item {
        prf_vtask t;
        u32 cost;
    };
    std::vector<Item> items;
    u32 reach = 0;       // furthest row of a lane's extended stream any task reads
    u32 covered_to = 0;  // group chunks cover motif sizes below this
    // the k = 1 flags of a clean tile come out of the k = 2 task (prf_plan.h); the k = 1 task stays for the mixed tiles
    const bool derive_k1 = prf_plan_derives_k1(kmin, kmax, min_repeats, min_span);
    for (u32 k = kmin; k <= kmax; k++) {
        const long long M = prf_plan_min_matches(k, min_repeats, min_span);
        if (M < SMALL_M) {
            Item it;
            it.t.k0 = (unsigned short)k;   // <= 14: M >= (min_repeats - 1) * k >= k
            it.t.kind = (unsigned char)M;  // M >= 1 because min_repeats >= 2
            it.t.valid = 1;
            it.t.stride = 1;
            it.t.pad = 0;
            if (derive_k1 && k == 1) it.t.pad = PRF_TASK_DERIVED;
            if (derive_k1 && k == 2) it.t.pad = PRF_TASK_RAISES_K1;
            it.cost = task_price(it.t);
            items.push_back(it);
            reach = std::max<u32>(reach, 4 * (((u32)T + (u32)M - 1 + k + 3) / 4) - 1);
        } else if (k >= covered_to) {
            // A group task takes the motif sizes k0 .. k0+7 (k0 a multiple of 4: whole 16-byte slots), or only the first four of
            // them where the two halves want different strides (default thresholds: 8-11 every group, 12-19 every 2nd, 20..
            // every 4th).  Examine every group, every 2nd or every 4th: a run of >= 8*S + 7 positions contains an aligned group
            // of 8 whose index is a multiple of S.
            const u32 k0 = k & ~3u;
            u32 valid = 0;
            long long mmin[2] = {1ll << 40, 1ll << 40};
            for (u32 kk = 0; kk < 8; kk++) {
                const u32 kx = k0 + kk;
                const long long Mx = prf_plan_min_matches(kx, min_repeats, min_span);
                if (kx >= kmin && kx <= kmax && Mx >= SMALL_M) {
                    valid |= 1u << kk;
                    mmin[kk >> 2] = std::min(mmin[kk >> 2], Mx);
                }
            }
            auto stride_of = [](long long m) { return m >= 39 ? 4u : (m >= 23 ? 2u : 1u); };
            const bool both = (valid & 0x0Fu) && (valid & 0xF0u);
            if (both && stride_of(mmin[0]) != stride_of(mmin[1])) valid &= 0x0Fu;  // the second half starts a task of its own
            const bool half = (valid & 0xF0u) == 0;
            const u32 stride = stride_of(half ? mmin[0] : std::min(mmin[0], mmin[1]));
            Item it;
            it.t.k0 = (unsigned short)k0;
            it.t.kind = 0;
            it.t.valid = (unsigned char)valid;
            it.t.stride = (unsigned char)stride;
            it.t.pad = 0;
            it.cost = task_price(it.t);
            items.push_back(it);
            reach = std::max<u32>(reach, 24 + k0 + (half ? 11 : 15));
            covered_to = k0 + (half ? 4 : 8);
        }
    }
    if (items.size() > PRF_VMAX_TASKS) return false;
    // The deal.  The derived k = 1 task is not dealt: it goes behind the k = 2 task, whose wave hands it the word (below), and is
    // priced with it.  Longest first onto the least loaded wave, then a local search over moves and swaps between any two waves
    // (which is all a large plan gets), then -- up to EXHAUSTIVE_TASKS tasks -- every deal.
    std::vector<Item> sorted;
    u32 handover = 0;
    for (const Item &it : items)
        if (it.t.pad & PRF_TASK_DERIVED) handover = it.cost;
        else sorted.push_back(it);
    for (Item &it : sorted)
        if (it.t.pad & PRF_TASK_RAISES_K1) it.cost += handover;
    std::stable_sort(sorted.begin(), sorted.end(), [](const Item &a, const Item &b) { return a.cost > b.cost; });
    const size_t n_dealt = sorted.size();
    std::vector<u32> cost(n_dealt), where(n_dealt, 0);
    u32 load[PRF_VMAX_WAVES] = {};
    for (size_t i = 0; i < n_dealt; i++) {
        cost[i] = sorted[i].cost;
        where[i] = (u32)(std::min_element(load, load + PRF_VMAX_WAVES) - load);
        load[where[i]] += cost[i];
    }
    for (bool better = true; better;) {
        better = false;
        DealKey cur = deal_key(load);
        for (size_t i = 0; i < n_dealt && !better; i++) {
            for (u32 w = 0; w < (u32)PRF_VMAX_WAVES && !better; w++) {  // move task i to wave w
                if (w == where[i]) continue;
                u32 l2[PRF_VMAX_WAVES];
                std::copy(load, load + PRF_VMAX_WAVES, l2);
                l2[where[i]] -= cost[i];
                l2[w] += cost[i];
                if (deal_key(l2) < cur) {
                    std::copy(l2, l2 + PRF_VMAX_WAVES, load);
                    where[i] = w;
                    better = true;
                }
            }
            for (size_t j = i + 1; j < n_dealt && !better; j++) {  // swap the tasks i and j
                if (where[i] == where[j] || cost[i] == cost[j]) continue;
                u32 l2[PRF_VMAX_WAVES];
                std::copy(load, load + PRF_VMAX_WAVES, l2);
                l2[where[i]] = l2[where[i]] - cost[i] + cost[j];
                l2[where[j]] = l2[where[j]] - cost[j] + cost[i];
                if (deal_key(l2) < cur) {
                    std::copy(l2, l2 + PRF_VMAX_WAVES, load);
                    std::swap(where[i], where[j]);
                    better = true;
                }
            }
        }
    }
    constexpr size_t EXHAUSTIVE_TASKS = 16;
    if (n_dealt <= EXHAUSTIVE_TASKS) {
        DealSearch ds{cost, std::vector<u32>(n_dealt, 0), where};
        ds.best = deal_key(load);
        ds.go(0);
        where = ds.best_where;
    }
    // waves in the order of their first (most expensive) task; the waves that got no task are the last ones
    u32 n_used = 0;
    {
        u32 name[PRF_VMAX_WAVES];
        std::fill(name, name + PRF_VMAX_WAVES, ~0u);
        for (size_t i = 0; i < n_dealt; i++)
            if (name[where[i]] == ~0u) name[where[i]] = n_used++;
        for (size_t i = 0; i < n_dealt; i++) where[i] = name[where[i]];
    }
    const u32 nw = std::max<u32>(1, n_used);
    std::vector<std::vector<Item>> bins(nw);
    std::fill(load, load + PRF_VMAX_WAVES, 0u);
    for (size_t i = 0; i < n_dealt; i++) {
        Item it = sorted[i];
        load[where[i]] += it.cost;
        if (it.t.pad & PRF_TASK_RAISES_K1) it.cost -= handover;
        bins[where[i]].push_back(it);
    }
    for (u32 w = 0; w < nw; w++) load[w] += FIRST_TASK;
    // (the ticket for the workgroup's next launch slot is drawn by the wave that leaves the scan first, whichever that is; the plan
    // names the wave it expects there.  Tried and dropped: the waves of a workgroup pulling tasks from one list through an LDS
    // counter at run time -- every wave's scan got 2-3 k cycles longer; the stride-1 group task cut in two halves of four sizes -- a
    // half costs three quarters of the whole, its four blocks are LDS latency, not arithmetic.)
    plan->ticket_wave = (u32)(std::min_element(load, load + PRF_VMAX_WAVES) - load);
    // The order inside a wave: group tasks that examine every or every 2nd group first, exact tasks next, stride-4 group tasks
    // last.  The tile's record list takes 192 records, first come first served, and a record that finds no slot is verified on
    // the spot by the general routine with one look per examined group of its stream: four looks at stride 1, one at stride 4.
    // In a tile of clusters (chr22-real's densest tile sets that workload's kernel time; its group tasks have several times 192
    // records) the slots should therefore go to the small strides.  With the tasks in the order of the deal, the stride-1 task
    // of k = 8 .. 11 came behind two exact tasks, found the list full and verified alone for 103 k cycles, where the parent's
    // three waves with stride-4 tasks took 22 - 33 k each; first in its wave but behind two stride-4 tasks of other waves it
    // still took 75 k (profiles/derived_k1_notes.md).  Only a plan that derives the k = 1 flags is ordered so; the others keep the
    // order of falling cost.
    auto rank_of = [](const Item &it) { return it.t.kind != 0 ? 1 : (it.t.stride < 4 ? 0 : 2); };
    for (auto &bin : bins)
        if (derive_k1) std::stable_sort(bin.begin(), bin.end(), [&](const Item &a, const Item &b) {
            if (rank_of(a) != rank_of(b)) return rank_of(a) < rank_of(b);
            return a.t.kind == 0 && a.t.k0 < b.t.k0;
        });
    // the derived k = 1 task directly behind the k = 2 task, in the same wave: on a clean tile it pushes the word that task left
    // for it in LDS (a wave's LDS operations are carried out in order: no barrier in between)
    for (const Item &it : items)
        if (it.t.pad & PRF_TASK_DERIVED)
            for (auto &bin : bins)
                for (size_t i = 0; i < bin.size(); i++)
                    if (bin[i].t.pad & PRF_TASK_RAISES_K1) {
                        bin.insert(bin.begin() + (long)i + 1, it);
                        break;
                    }
    {
        // The fields: prf_plan.h.  The short, latency-bound phases (stage, the record waves of the verify phase, rows) at
        // priority 2, the scan (long, plenty of independent arithmetic) at 0; the hand-over between scan and verify, for which
        // every wave of the workgroup waits, and the flag waves of the verify phase, whose flags are that phase's longest leg,
        // have fields of their own.  The sweep: tools/prio_sweep.sh, profiles/scan_handover_notes.md section 4.
        // PRF_PRIO overrides in a diagnostic build (PRF_DIAG).
        constexpr u32 PRIO_DEFAULT = 0x0A02u | (PRIO_HANDOVER << 12) | (PRIO_FLAGS << 6);
#ifdef PRF_DIAG
        static const u32 prio_cfg = getenv("PRF_PRIO") ? (u32)strtoul(getenv("PRF_PRIO"), nullptr, 0) : PRIO_DEFAULT;
#else
        const u32 prio_cfg = PRIO_DEFAULT;
#endif
        plan->prio = prio_cfg;
        const u32 busiest = *std::max_element(load, load + PRF_VMAX_WAVES);
        plan->slack_waves = 0;
        for (u32 w = 0; w < (u32)PRF_VMAX_WAVES; w++)
            if (w >= nw || 10u * load[w] < 9u * busiest) plan->slack_waves |= 1u << w;
    }
    plan->n_waves = nw;
    plan->n_tasks = 0;
    plan->n_group_k = 0;
    plan->n_exact = 0;
    // the motif sizes of the exact tasks are consecutive: M(k) = max((r-1) k, span - k) is V-shaped, so {k : M(k) < 15} is an interval
    u32 k_exact0 = ~0u, k_exact1 = 0, n_exact_items = 0;
    for (const Item &it : items)
        if (it.t.kind) {
            k_exact0 = std::min<u32>(k_exact0, it.t.k0);
            k_exact1 = std::max<u32>(k_exact1, it.t.k0);
            n_exact_items++;
        }
    if (n_exact_items && k_exact1 - k_exact0 + 1 != n_exact_items) return false;
    plan->k_exact0 = n_exact_items ? k_exact0 : 0;
    for (u32 w = 0; w < nw; w++) {
        plan->wave_begin[w] = plan->n_tasks;
        for (const Item &it : bins[w]) {
            prf_vtask t = it.t;
            t.item0 = 0;
            if (t.kind == 0) {
                t.item0 = (unsigned short)plan->n_group_k;
                plan->n_group_k += (u32)__builtin_popcount((unsigned)t.valid);
            } else {
                plan->n_exact++;
                t.item0 = (unsigned short)(t.k0 - k_exact0);
            }
            plan->tasks[plan->n_tasks++] = t;
        }
    }
    for (u32 w = nw; w <= PRF_VMAX_WAVES; w++) plan->wave_begin[w] = plan->n_tasks;
    const u32 need_nc = 64 + reach / T;  // row r of a lane's extended stream lies in virtual lane + r / 32
    plan->nc = need_nc <= 72 ? 72 : 80;  // the widths the kernel is instantiated for
    plan->cof_words = (kmax + 1 + 3) & ~3u;  // <= PRF_VMAX_K + 4: the table is declared with that many entries
    // header, R1 (image / window), records, row list, all-N masks, flag lists + counts, boundary items, cofactor table
    plan->lds_bytes = (u32)(SMEM_HDR + (size_t)2 * RG * plan->nc * 16 + (size_t)REC_CAP * sizeof(u64) +
                            (size_t)2 * ROW_CAP_LDS * sizeof(u32) + (size_t)SLOW_CAP * 16 + (size_t)FLAG_CAP * 2 +
                            (size_t)plan->n_group_k * sizeof(u32) + (size_t)plan->cof_words * sizeof(u32));
    plan->per_cu = 0;  // (set at the first launch: the occupancy the runtime reports for this much LDS)
    return need_nc <= 80;
}

// A scan asks for its plan every time, and the deal looks at every deal of a small plan: the thread's last plan is kept.
bool prf_vertical_plan(u32 kmin, u32 kmax, u32 min_repeats, u32 min_span, prf_vplan *plan) {
    struct Last {
        u32 key[4];
        bool have, ok;
        prf_vplan plan;
    };
    thread_local Last last = {};
    if (!(last.have && last.key[0] == kmin && last.key[1] == kmax && last.key[2] == min_repeats && last.key[3] == min_span)) {
        last.have = false;
        last.plan = prf_vplan{};
        last.ok = build_plan(kmin, kmax, min_repeats, min_span, &last.plan);
        last.key[0] = kmin; last.key[1] = kmax; last.key[2] = min_repeats; last.key[3] = min_span;
        last.have = true;
    }
    *plan = last.plan;
    return last.ok;
}

int prf_plan_json(u32 kmin, u32 kmax, u32 min_repeats, u32 min_span, char *buf, u64 buf_len) {
    std::string out;
    prf_vplan plan;
    if (!prf_vertical_plan(kmin, kmax, min_repeats, min_span, &plan)) {
        out = "{\"path\": \"generic\"}";
    } else {
        char tmp[240];
        // (price: what the deal charges for the task, cycles per tile; window: the W' of its objective; first_task: what a wave with
        // tasks is charged on top of their prices)
        snprintf(tmp, sizeof tmp, "{\"path\": \"fused\", \"waves\": %u, \"nc\": %u, \"lds_bytes\": %u, \"window\": %u, \"first_task\": %u, \"tasks\": [",
                 plan.n_waves, plan.nc, plan.lds_bytes, (unsigned)WINDOW_W, (unsigned)FIRST_TASK);
        out = tmp;
        bool first = true;
        for (u32 w = 0; w < plan.n_waves; w++)
            for (u32 ti = plan.wave_begin[w]; ti < plan.wave_begin[w + 1]; ti++) {
                const prf_vtask &t = plan.tasks[ti];
                snprintf(tmp, sizeof tmp, "%s{\"wave\": %u, \"kind\": %u, \"k0\": %u, \"valid\": %u, \"stride\": %u, \"derive\": %u, \"price\": %u}",
                         first ? "" : ", ", w, (unsigned)t.kind, (unsigned)t.k0, (unsigned)t.valid, (unsigned)t.stride, (unsigned)(t.pad & 3u),
                         (unsigned)task_price(t));
                out += tmp;
                first = false;
            }
        out += "]}";
    }
    if (out.size() + 1 > buf_len) return -1;
    memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}
