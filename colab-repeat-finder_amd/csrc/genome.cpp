// genome.cpp -- genome residency: a genome is loaded (or generated on the device) once, packed into its linear and bit-sliced
// planes, and scanned many times; the selection of parts a rank scans, and what the genome holds on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "genome.h"

static const u64 PRF_FRONT_PAD = 8;  // readable words in front of every linear plane (X = all ones there)

int prf_genome_contig_view(const prf_genome *g, u32 contig, prf_contig_view *out) {
    if (!g || !out) return fail(PRF_EINVAL, "NULL genome");
    if (contig >= g->base.size()) return fail(PRF_EINVAL, "contig %u out of range (the genome holds %zu)", contig, g->base.size());
    out->ctx = g->ctx;
    out->planes = planes_of(g);
    out->base = g->base[contig];
    out->len = g->len[contig];
    out->kmax_hint = g->kmax_hint;
    return PRF_OK;
}

extern "C" {

void prf_genome_free(prf_genome *g) {
    if (!g) return;
    if (g->ctx) (void)hipSetDevice(g->ctx->dev);
    for (u64 *plane : {g->H, g->L, g->X, g->E[0], g->E[1], g->E[2], g->E[3], g->E[4]})
        if (plane) (void)hipFree(plane - PRF_FRONT_PAD);
    for (void *p : {(void *)g->d_E, (void *)g->d_base, (void *)g->d_tile_info, (void *)g->vp.VH, (void *)g->vp.VL,
                    (void *)g->vp.tile_class, (void *)g->vp.launch_list, (void *)g->d_sel_list})
        (void)hipFree(p);
    delete g;
}

uint64_t prf_genome_positions(const prf_genome *g) { return g ? g->positions : 0; }

// One linear plane of the genome: PRF_FRONT_PAD readable words in front of it, padw behind it, both filled with `pad`
static int alloc_plane(prf_ctx *c, const prf_genome *g, u64 **plane, int pad) {
    u64 *p = nullptr;
    HIPCHK(hipMalloc((void **)&p, (PRF_FRONT_PAD + g->nwords + g->padw) * 8));
    *plane = p + PRF_FRONT_PAD;
    HIPCHK(hipMemsetAsync(p, pad, PRF_FRONT_PAD * 8, c->stream));
    HIPCHK(hipMemsetAsync(*plane + g->nwords, pad, g->padw * 8, c->stream));
    return PRF_OK;
}

// The contig of every tile (contigs start on tile boundaries; the gap tiles behind a contig count as its own)
static int upload_tile_info(prf_genome *g) {
    const u64 ntiles = g->G / PRF_TILE;
    std::vector<uint4> info(ntiles, make_uint4(0, 0, 0, 0));
    for (size_t ci = 0; ci < g->base.size(); ci++) {
        const u64 t0 = g->base[ci] / PRF_TILE, t1 = ci + 1 < g->base.size() ? g->base[ci + 1] / PRF_TILE : ntiles;
        for (u64 t = t0; t < t1; t++) info[t] = make_uint4((u32)ci, 0u, (u32)g->base[ci], (u32)(g->base[ci] >> 32));
    }
    HIPCHK(hipMalloc((void **)&g->d_tile_info, sizeof(uint4) * ntiles));
    HIPCHK(hipMemcpy(g->d_tile_info, info.data(), sizeof(uint4) * ntiles, hipMemcpyHostToDevice));
    return PRF_OK;
}

// Letters other than A, C, G, T, N: the planes of their codes, and the tile ranges the generic kernels take
static int load_exotic(prf_ctx *c, prf_genome *g, const uint8_t *asc) {
    for (u64 *&plane : g->E) {
        const int rc = alloc_plane(c, g, &plane, 0);
        if (rc) return rc;
    }
    HIPCHK(prf_launch_pack_exotic(c->stream, asc, g->nwords, g->E));
    HIPCHK(hipMalloc((void **)&g->d_E, 5 * sizeof(u64 *)));
    HIPCHK(hipMemcpyAsync(g->d_E, g->E, 5 * sizeof(u64 *), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const std::vector<unsigned char> &cls = g->vp.h_class;
    for (u64 t = 0; t + 1 < cls.size(); t++) {
        if (cls[t] != 3) continue;
        if (!g->exotic_tiles.empty() && g->exotic_tiles.back().second == t) g->exotic_tiles.back().second = t + 1;
        else g->exotic_tiles.emplace_back(t, t + 1);
    }
    return PRF_OK;
}

// contigs[i].ascii == nullptr with seeds != nullptr: contig i is generated on the device from seeds[i]
// recipe (with seeds): 1 = uniform background, 2 = stand-in recipe 2 (N blocks + planted repeats)
static int genome_load_impl(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmax_hint, prf_genome **out,
                            const uint64_t *seeds = nullptr, int recipe = 1) {
    if (!c || !out || n_contigs < 0 || (n_contigs > 0 && !contigs))
        return fail(PRF_EINVAL, "prf_genome_load: bad arguments");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->dev));
    if (kmax_hint < 1) kmax_hint = 1;
    if (kmax_hint > 60000) return fail(PRF_EUNSUPPORTED, "prf_genome_load: kmax_hint %u > 60000", kmax_hint);
    prf_genome *g = new (std::nothrow) prf_genome();
    if (!g) return fail(PRF_ENOMEM, "prf_genome_load: out of host memory");
    struct guard_t {
        prf_genome *g;
        ~guard_t() { if (g) prf_genome_free(g); }
    } guard{g};
    g->ctx = c;
    g->kmax_hint = kmax_hint;
    const u64 gap = (u64)kmax_hint + 64;
    u64 cur = 0;
    for (int i = 0; i < n_contigs; i++) {
        if (contigs[i].len && !contigs[i].ascii && !seeds) return fail(PRF_EINVAL, "prf_genome_load: contig %d has NULL data", i);
        g->base.push_back(cur);
        g->len.push_back(contigs[i].len);
        g->positions += contigs[i].len;
        cur = (cur + contigs[i].len + gap + PRF_TILE - 1) / PRF_TILE * PRF_TILE;
    }
    if (cur == 0) cur = PRF_TILE;
    g->G = cur + PRF_TILE;  // one all-gap sentinel tile: every walk to the right ends inside the arrays
    if (g->G >= (1ull << 40)) return fail(PRF_EUNSUPPORTED, "prf_genome_load: input too large (2^40 positions)");  // row keys: 40-bit offsets
    g->nwords = g->G / 64;
    g->padw = kmax_hint / 64 + 8;

    dev_array<uint8_t> asc_bytes;
    if (const int rc = asc_bytes.alloc(g->G)) return rc;
    uint8_t *const asc = asc_bytes.p;
    HIPCHK(prf_launch_fill_u64(c->stream, (u64 *)asc, g->G / 8, 0x4E4E4E4E4E4E4E4Eull));  // 'N' everywhere
    for (int i = 0; i < n_contigs; i++) {
        if (!contigs[i].len) continue;
        if (seeds && recipe == 2)
            HIPCHK(prf_launch_standin2(c->stream, asc + g->base[i], contigs[i].len, seeds[i]));
        else if (seeds)  // the generator writes whole 16-byte groups; the tail beyond len is 'N' again, like the gap
            HIPCHK(prf_launch_synth(c->stream, asc + g->base[i], contigs[i].len, seeds[i]));
        else
            HIPCHK(hipMemcpyAsync(asc + g->base[i], contigs[i].ascii, contigs[i].len, hipMemcpyHostToDevice, c->stream));
    }
    int rc = alloc_plane(c, g, &g->H, 0);
    if (!rc) rc = alloc_plane(c, g, &g->L, 0);
    if (!rc) rc = alloc_plane(c, g, &g->X, 0xFF);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_counters, 0xFF, PRF_CNT_N * sizeof(u64), c->stream));
    HIPCHK(hipMemsetAsync(c->d_counters + PRF_CNT_EXOTIC, 0, sizeof(u64), c->stream));
    HIPCHK(prf_launch_pack_linear(c->stream, asc, g->nwords, g->H, g->L, g->X, c->d_counters + PRF_CNT_BADPOS,
                                  c->d_counters + PRF_CNT_EXOTIC));
    HIPCHK(hipMalloc((void **)&g->d_base, sizeof(u64) * (size_t)(n_contigs > 0 ? n_contigs : 1)));
    if (n_contigs > 0)
        HIPCHK(hipMemcpyAsync(g->d_base, g->base.data(), sizeof(u64) * (size_t)n_contigs, hipMemcpyHostToDevice, c->stream));
    if ((rc = upload_tile_info(g))) return rc;
    // bit-sliced copy for the vertical kernel (built from the ASCII while it is still resident)
    rc = prf_vertical_pack(c->stream, asc, g->G, &g->vp);
    if (rc != hipSuccess)
        return fail(rc == (int)hipErrorOutOfMemory ? PRF_ENOMEM : PRF_EHIP, "vertical pack failed: %s", hipGetErrorString((hipError_t)rc));
    HIPCHK(hipMemcpyAsync(c->h_counters, c->d_counters, PRF_CNT_N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const u64 bad = c->h_counters[PRF_CNT_BADPOS];
    if (bad != ~0ull) {
        size_t ci = std::upper_bound(g->base.begin(), g->base.end(), bad) - g->base.begin() - 1;
        return fail(PRF_ESYMBOL,
                    "unsupported symbol at contig %zu position %llu: only letters can be packed (A, C, G, T, N and -- as ordinary "
                    "symbols, like the reference -- any other letter, in either case); libprf refuses other bytes instead of guessing",
                    ci, (unsigned long long)(bad - g->base[ci]));
    }
    if (c->h_counters[PRF_CNT_EXOTIC] && (rc = load_exotic(c, g, asc))) return rc;
    guard.g = nullptr;
    *out = g;
    return PRF_OK;
}

int prf_genome_load(prf_ctx *c, const prf_contig *contigs, int n_contigs, uint32_t kmax_hint, prf_genome **out) {
    return guarded("prf_genome_load", [&] { return genome_load_impl(c, contigs, n_contigs, kmax_hint, out); });
}

// contigs generated on the device from seeds (recipe 1: uniform background, 2: stand-in recipe 2)
static int genome_generate(const char *name, prf_ctx *c, const uint64_t *lens, const uint64_t *seeds, int n_contigs,
                           uint32_t kmax_hint, prf_genome **out, int recipe) {
    if (n_contigs < 0 || (n_contigs > 0 && (!lens || !seeds))) return fail(PRF_EINVAL, "%s: bad arguments", name);
    return guarded(name, [&] {
        std::vector<prf_contig> cs((size_t)(n_contigs > 0 ? n_contigs : 1));
        for (int i = 0; i < n_contigs; i++) cs[i] = prf_contig{nullptr, lens[i]};
        return genome_load_impl(c, cs.data(), n_contigs, kmax_hint, out, seeds, recipe);
    });
}

int prf_genome_synth(prf_ctx *c, const uint64_t *lens, const uint64_t *seeds, int n_contigs, uint32_t kmax_hint, prf_genome **out) {
    return genome_generate("prf_genome_synth", c, lens, seeds, n_contigs, kmax_hint, out, 1);
}

int prf_genome_standin(prf_ctx *c, const uint64_t *lens, const uint64_t *seeds, int n_contigs, uint32_t kmax_hint, prf_genome **out) {
    return genome_generate("prf_genome_standin", c, lens, seeds, n_contigs, kmax_hint, out, 2);
}

int prf_genome_tile_classes(const prf_genome *g, uint32_t contig, uint8_t *dst, uint64_t capacity, uint64_t *n_tiles) {
    if (!g || !n_tiles || contig >= g->base.size() || (capacity && !dst)) return fail(PRF_EINVAL, "prf_genome_tile_classes: bad arguments");
    const u64 t0 = g->base[contig] / PRF_TILE, n = (g->len[contig] + PRF_TILE - 1) / PRF_TILE;
    *n_tiles = n;
    for (u64 i = 0; i < n && i < capacity; i++) dst[i] = g->vp.h_class[t0 + i];
    return PRF_OK;
}

static int genome_select_impl(prf_genome *g, const prf_part *parts, int n_parts) {
    if (!g || n_parts < 0 || (n_parts > 0 && !parts)) return fail(PRF_EINVAL, "prf_genome_select: bad arguments");
    prf_ctx *c = g->ctx;
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipStreamSynchronize(c->stream));  // no scan of this genome may be reading the old selection
    if (n_parts == 0) {
        g->sel_on = false;
        return PRF_OK;
    }
    tile_ranges tr;
    u64 positions = 0;
    for (int i = 0; i < n_parts; i++) {
        const prf_part &p = parts[i];
        if (p.contig >= g->base.size()) return fail(PRF_EINVAL, "prf_genome_select: part %d names contig %u of %zu", i, p.contig, g->base.size());
        const u64 len = g->len[p.contig];
        const u64 end = std::min<u64>(p.end, len);
        if (p.begin % PRF_TILE != 0 || (end % PRF_TILE != 0 && end != len) || p.begin > end)
            return fail(PRF_EINVAL, "prf_genome_select: part %d [%llu, %llu) of contig %u must begin on a multiple of %u and end on one or at "
                        "the contig's end", i, (unsigned long long)p.begin, (unsigned long long)p.end, p.contig, PRF_TILE);
        if (end == p.begin) continue;
        const u64 t0 = g->base[p.contig] / PRF_TILE;
        tr.emplace_back(t0 + p.begin / PRF_TILE, t0 + (end + PRF_TILE - 1) / PRF_TILE);
        positions += end - p.begin;
    }
    std::sort(tr.begin(), tr.end());
    tile_ranges merged;
    for (const auto &r : tr) {
        if (!merged.empty() && r.first < merged.back().second)
            return fail(PRF_EINVAL, "prf_genome_select: parts overlap");
        if (!merged.empty() && r.first == merged.back().second) merged.back().second = r.second;
        else merged.push_back(r);
    }
    std::vector<u32> list;
    {
        const std::vector<u32> &all = g->vp.h_list;  // ascending by tile
        size_t i = 0;
        for (const auto &r : merged) {
            while (i < all.size() && (all[i] & ~PRF_LAUNCH_MIXED) < r.first) i++;
            while (i < all.size() && (all[i] & ~PRF_LAUNCH_MIXED) < r.second) list.push_back(all[i++]);
        }
    }
    if (!g->d_sel_list) HIPCHK(hipMalloc((void **)&g->d_sel_list, sizeof(u32) * std::max<size_t>(1, g->vp.h_list.size())));
    if (!list.empty()) HIPCHK(hipMemcpy(g->d_sel_list, list.data(), sizeof(u32) * list.size(), hipMemcpyHostToDevice));
    g->sel_n = (u32)list.size();
    g->sel_flat = prf_flat_base(list.data(), list.size());
    g->sel_positions = positions;
    g->sel_tiles = std::move(merged);
    g->sel_on = true;
    return PRF_OK;
}

int prf_genome_select(prf_genome *g, const prf_part *parts, int n_parts) {
    return guarded("prf_genome_select", [&] { return genome_select_impl(g, parts, n_parts); });
}

int prf_genome_contig_bases(const prf_genome *g, uint64_t *bases, uint64_t capacity, uint64_t *n_contigs) {
    if (!g || !n_contigs || (capacity && !bases)) return fail(PRF_EINVAL, "prf_genome_contig_bases: bad arguments");
    *n_contigs = g->base.size();
    for (size_t i = 0; i < g->base.size() && i < capacity; i++) bases[i] = g->base[i];
    return PRF_OK;
}

int prf_genome_footprint(const prf_genome *g, uint64_t *device_bytes, uint64_t *positions) {
    if (!g || !device_bytes || !positions) return fail(PRF_EINVAL, "prf_genome_footprint: bad arguments");
    const u64 tot = PRF_FRONT_PAD + g->nwords + g->padw;      // words of one linear plane (alloc_plane)
    const u64 ntiles = g->G / PRF_TILE;
    u64 bytes = 3 * tot * 8;                                   // H, L, X
    if (g->d_E) bytes += 5 * tot * 8 + 5 * sizeof(u64 *);      // the code planes of the letters outside ACGTN
    bytes += 2 * ntiles * (PRF_TILE / 8);                      // VH, VL
    bytes += 2 * ntiles + sizeof(u32) * ntiles;                // tile classes (+ scratch), launch list
    bytes += sizeof(uint4) * ntiles + sizeof(u64) * std::max<size_t>(1, g->base.size());  // tile table, contig bases
    if (g->d_sel_list) bytes += sizeof(u32) * std::max<size_t>(1, g->vp.h_list.size());
    *device_bytes = bytes;
    *positions = g->G;
    return PRF_OK;
}

}  // extern "C"
