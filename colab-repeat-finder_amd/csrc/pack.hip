// pack.hip -- ASCII -> bit planes (linear and bit-sliced), on the device.
//
// Replaces the reference's input_sequence.upper() plus its two further whole-sequence copies
// (reference perfect_repeat_finder.py:33, :46): the ASCII bytes are read once, case-folded in
// registers and written as three 1-bit planes (H, L = base code, X = not-ACGT).
#include "prf_device.h"
#include "prf_host.h"
#include "scan_vertical.h"

// One thread packs one 64-position word: 64 bytes in (4 x 16-B loads), 3 x 8 bytes out.
// Symbols: A, C, G, T -> code; N -> X; any other LETTER is an ordinary symbol to the reference (R == R matches,
// utils/perfect_repeat_tracker.py:53): X is set for it here and *exotic is raised, so that the planes of its code are built
// (prf_pack_exotic_kernel); a byte that is no letter at all is refused (bad_pos).
__global__ __launch_bounds__(256) void prf_pack_linear_kernel(const uint8_t *__restrict__ asc, u64 nwords,
                                                              u64 *__restrict__ H, u64 *__restrict__ L,
                                                              u64 *__restrict__ X, u64 *__restrict__ bad_pos, u64 *__restrict__ exotic) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(asc + w * 64);
    u64 h = 0, l = 0, x = 0, bad = 0, exo = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = src[q];
        const u32 d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const u32 c = ((d[j] >> (8 * b)) & 0xFFu);
                const u32 f = c & 0xDFu;  // ASCII case fold for letters (str.upper(), reference :33)
                const u32 is_acgt = (f == 'A') | (f == 'C') | (f == 'G') | (f == 'T');
                // only letters fold onto letters, so comparing the folded byte is exact for a-z/A-Z;
                // bytes outside both letter ranges can never equal 'A','C','G','T','N' after the fold
                // except 0x41..0x5A themselves.
                const u32 is_n = (f == 'N');
                const u32 is_letter = (f >= 'A') & (f <= 'Z');
                const int bit = q * 16 + j * 4 + b;
                h |= (u64)((f >> 2) & 1u & is_acgt) << bit;
                l |= (u64)((f >> 1) & 1u & is_acgt) << bit;
                x |= (u64)(is_acgt ^ 1u) << bit;
                bad |= (u64)(is_letter ^ 1u) << bit;
                exo |= (u64)(is_letter & ((is_acgt | is_n) ^ 1u)) << bit;
            }
        }
    }
    H[w] = h;
    L[w] = l;
    X[w] = x;
    if (bad) atomicMin(bad_pos, w * 64 + (u64)__builtin_ctzll(bad));
    if (exo) atomicMax(exotic, 1ull);
}

// the five code planes of the symbols outside ACGTN (prf_planes::E): low five bits of the upper-cased letter
__global__ __launch_bounds__(256) void prf_pack_exotic_kernel(const uint8_t *__restrict__ asc, u64 nwords, u64 *__restrict__ E0,
                                                              u64 *__restrict__ E1, u64 *__restrict__ E2, u64 *__restrict__ E3,
                                                              u64 *__restrict__ E4) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(asc + w * 64);
    u64 e[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = src[q];
        const u32 d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const u32 f = ((d[j] >> (8 * b)) & 0xFFu) & 0xDFu;
                const u32 plain = (f == 'A') | (f == 'C') | (f == 'G') | (f == 'T') | (f == 'N');
                const u32 code = ((f >= 'A') & (f <= 'Z') & (plain ^ 1u)) ? (f & 31u) : 0u;
                const int bit = q * 16 + j * 4 + b;
#pragma unroll
                for (int i = 0; i < 5; i++) e[i] |= (u64)((code >> i) & 1u) << bit;
            }
        }
    }
    E0[w] = e[0]; E1[w] = e[1]; E2[w] = e[2]; E3[w] = e[3]; E4[w] = e[4];
}

hipError_t prf_launch_pack_exotic(hipStream_t s, const uint8_t *asc, u64 nwords, u64 *const *E) {
    const u32 bs = 256;
    const u64 nb = (nwords + bs - 1) / bs;
    hipLaunchKernelGGL(prf_pack_exotic_kernel, dim3((u32)nb), dim3(bs), 0, s, asc, nwords, E[0], E[1], E[2], E[3], E[4]);
    return hipGetLastError();
}

// fill value for guard gaps and padding: N
__global__ void prf_fill_u64_kernel(u64 *__restrict__ p, u64 n, u64 v) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

// SURVEY 8(d) counter-based generator, 16 bases per lane (one 16-byte store)
__global__ __launch_bounds__(256) void prf_synth_kernel(uint8_t *__restrict__ asc, u64 n, u64 seed) {
    const u64 chunk = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 j0 = chunk * 16;
    if (j0 >= n) return;
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        u64 z = seed + (j0 + (u64)i + 1ull) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const u32 code = (u32)(z >> 62);
        const u32 ch = (0x54474341u >> (8 * code)) & 0xFFu;  // "ACGT"[code]
        w[i >> 2] |= (j0 + (u64)i < n ? ch : (u32)'N') << (8 * (i & 3));
    }
    *reinterpret_cast<uint4 *>(asc + j0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- stand-in recipe 2 (colab-repeat-finder_amd/synth.py::standin2, integer arithmetic only, so that numpy and this kernel
// agree bit for bit): uniform background; N at [0, n_head), [n - n_tail, n) and [gap_lo, gap_hi); the body
// [n_head, n - n_tail) is cut into slots of 588 positions, each with ONE planted perfect tandem repeat whose motif is the
// background at the repeat's own first k positions.
__device__ __forceinline__ u64 prf_splitmix(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ u32 prf_background(u64 seed, u64 j) { return (u32)(prf_splitmix(seed + (j + 1ull) * 0x9E3779B97F4A7C15ull) >> 62); }

struct prf_slot_repeat {
    u64 p;       // first position
    u32 k, span;
};
__device__ __forceinline__ prf_slot_repeat prf_slot_params(u64 seed, u64 body_lo, u64 slot) {
    const u64 d = prf_splitmix((seed ^ 0xD1B54A32D192ED03ull) + (slot + 1ull) * 0x9E3779B97F4A7C15ull);
    const u64 d2 = prf_splitmix(d + 0x9E3779B97F4A7C15ull);
    const u32 u = (u32)(d >> 48), v = (u32)(d >> 24) & 0xFFFFFFu, w = (u32)d & 0xFFFFFFu, x = (u32)(d2 >> 32);
    // motif size: the reference's golden chr22 BED histogram for 1..6 (95 %), a thin tail up to 50
    u32 k;
    if (u < 18412u) k = 1; else if (u < 29561u) k = 2; else if (u < 49738u) k = 3; else if (u < 58461u) k = 4;
    else if (u < 61413u) k = 5; else if (u < 62268u) k = 6;
    else { const u32 t = u - 62268u; k = 7u + (t * t * 44u) / (3268u * 3268u); }
    // copies: 3 + geometric(0.67); thresholds floor(2^24 * 0.67^(i+1))
    const u32 th[16] = {11240734u, 7531292u, 5045965u, 3380797u, 2265134u, 1517639u, 1016818u, 681268u,
                        456449u, 305821u, 204900u, 137283u, 91979u, 61626u, 41289u, 27664u};
    u32 copies = 3;
#pragma unroll
    for (int i = 0; i < 16; i++) copies += v < th[i] ? 1u : 0u;
    u32 span = k * copies + w % k;
    span = span > 500u ? 500u : span;
    span = span < 10u ? 10u : span;
    prf_slot_repeat r;
    r.k = k;
    r.span = span;
    r.p = body_lo + slot * 588ull + (u64)(x % (588u - span));
    return r;
}

__global__ __launch_bounds__(256) void prf_standin2_kernel(uint8_t *__restrict__ asc, u64 n, u64 seed, u64 n_head, u64 n_tail,
                                                            u64 gap_lo, u64 gap_hi) {
    const u64 chunk = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 j0 = chunk * 16;
    if (j0 >= n) return;
    const u64 body_lo = n_head, body_hi = n - n_tail;
    const u64 n_slots = (body_hi - body_lo) / 588ull;
    // 16 consecutive positions touch at most two slots
    u64 cur_slot = ~0ull;
    prf_slot_repeat rep = {0, 1, 0};
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const u64 j = j0 + (u64)i;
        u32 ch = (u32)'N';
        if (j < n && j >= n_head && j < body_hi && !(j >= gap_lo && j < gap_hi)) {
            u64 src = j;
            const u64 slot = (j - body_lo) / 588ull;
            if (slot < n_slots) {
                if (slot != cur_slot) {
                    cur_slot = slot;
                    rep = prf_slot_params(seed, body_lo, slot);
                }
                if (j >= rep.p && j < rep.p + rep.span) src = rep.p + (j - rep.p) % rep.k;
            }
            ch = (0x54474341u >> (8 * prf_background(seed, src))) & 0xFFu;  // "ACGT"[code]
        }
        w[i >> 2] |= ch << (8 * (i & 3));
    }
    *reinterpret_cast<uint4 *>(asc + j0) = make_uint4(w[0], w[1], w[2], w[3]);
}

hipError_t prf_launch_standin2(hipStream_t s, uint8_t *asc, u64 n, u64 seed) {
    if (n == 0) return hipSuccess;
    const u64 n_head = n / 100 < 10000 ? n / 100 : 10000, n_tail = n_head;
    u64 gap_lo = 0, gap_hi = 0;
    if (n >= 1000000) {
        gap_lo = n / 8 * 3 + 12345;
        gap_hi = gap_lo + n / 25;
    }
    const u64 chunks = (n + 15) / 16;
    hipLaunchKernelGGL(prf_standin2_kernel, dim3((u32)((chunks + 255) / 256)), dim3(256), 0, s, asc, n, seed, n_head, n_tail, gap_lo,
                       gap_hi);
    return hipGetLastError();
}

hipError_t prf_launch_synth(hipStream_t s, uint8_t *asc, u64 n, u64 seed) {
    if (n == 0) return hipSuccess;
    const u64 chunks = (n + 15) / 16;
    hipLaunchKernelGGL(prf_synth_kernel, dim3((u32)((chunks + 255) / 256)), dim3(256), 0, s, asc, n, seed);
    return hipGetLastError();
}

hipError_t prf_launch_pack_linear(hipStream_t s, const uint8_t *asc, u64 nwords, u64 *H, u64 *L, u64 *X,
                                  u64 *bad_pos, u64 *exotic) {
    const u32 bs = 256;
    const u64 nb = (nwords + bs - 1) / bs;
    hipLaunchKernelGGL(prf_pack_linear_kernel, dim3((u32)nb), dim3(bs), 0, s, asc, nwords, H, L, X, bad_pos, exotic);
    return hipGetLastError();
}

hipError_t prf_launch_fill_u64(hipStream_t s, u64 *p, u64 n, u64 v) {
    if (n == 0) return hipSuccess;
    u64 nb = (n + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(prf_fill_u64_kernel, dim3((u32)nb), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// The bit-sliced ("vertical") planes of the fused scan kernel (layout: scan_vertical.hip), their tile classes and launch list.
namespace {

using prf_layout::T; using prf_layout::RG;  // (prf_plan.h)

// ASCII -> bit-sliced planes.  One wave per tile; lane l, for bit b = 0..31, reads the 32 consecutive
// bytes of stream b*64+l (a wave reads 2 KiB contiguous per b) and spreads them over its 32 row words.
__global__ __launch_bounds__(64) void prf_pack_vertical_kernel(const uint8_t *__restrict__ asc, u32 *__restrict__ VH,
                                                               u32 *__restrict__ VL,
                                                               unsigned char *__restrict__ any_all) {
    const u64 tile = blockIdx.x;
    const int lane = (int)threadIdx.x;
    u32 h[T], l[T], x[T];
    u32 exo = 0;  // any letter other than A, C, G, T, N
#pragma unroll
    for (int t = 0; t < T; t++) h[t] = l[t] = x[t] = 0;
    const uint8_t *base = asc + tile * PRF_TILE + (u64)lane * T;
    for (int b = 0; b < 32; b++) {
        const uint4 *src = reinterpret_cast<const uint4 *>(base + (u64)b * (64 * T));
        const uint4 v0 = src[0], v1 = src[1];
        const u32 d[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int t = 0; t < T; t++) {
            const u32 f = (d[t >> 2] >> (8 * (t & 3))) & 0xDFu;
            const u32 ok = (f == 'A') | (f == 'C') | (f == 'G') | (f == 'T');
            h[t] |= ((f >> 2) & 1u & ok) << b;
            l[t] |= ((f >> 1) & 1u & ok) << b;
            x[t] |= (ok ^ 1u) << b;
            exo |= (ok | (f == 'N')) ^ 1u;
        }
    }
    u32 any = 0, all = ~0u;
#pragma unroll
    for (int t = 0; t < T; t++) {
        any |= x[t];
        all &= x[t];
    }
    uint4 *oh = reinterpret_cast<uint4 *>(VH) + tile * RG * 64 + lane;
    uint4 *ol = reinterpret_cast<uint4 *>(VL) + tile * RG * 64 + lane;
#pragma unroll
    for (int rg = 0; rg < RG; rg++) {
        oh[rg * 64] = make_uint4(h[4 * rg], h[4 * rg + 1], h[4 * rg + 2], h[4 * rg + 3]);
        ol[rg * 64] = make_uint4(l[4 * rg], l[4 * rg + 1], l[4 * rg + 2], l[4 * rg + 3]);
    }
    const bool w_any = __builtin_amdgcn_ballot_w64(any != 0) != 0;
    const bool w_all = __builtin_amdgcn_ballot_w64(all != ~0u) == 0;
    const bool w_exo = __builtin_amdgcn_ballot_w64(exo != 0) != 0;
    if (lane == 0) any_all[tile] = (unsigned char)((w_any ? 1 : 0) | (w_all ? 2 : 0) | (w_exo ? 4 : 0));
}

// class: 3 = a symbol outside ACGTN in this tile, the one before or the one after (such tiles are scanned by the generic
// kernels, with the symbols' own planes); 2 = only not-ACGT; 1 = some not-ACGT in this tile or the next (whose first lanes
// are this tile's virtual lanes 64..); 0 = clean
__global__ void prf_tile_class_kernel(const unsigned char *__restrict__ any_all, unsigned char *__restrict__ cls, u64 ntiles) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntiles) return;
    const unsigned char a = any_all[i];
    const unsigned char b = (i + 1 < ntiles) ? any_all[i + 1] : (unsigned char)3;
    const unsigned char p = i ? any_all[i - 1] : (unsigned char)0;
    cls[i] = ((a | b | p) & 4) ? 3 : ((a & 2) ? 2 : (((a | b) & 1) ? 1 : 0));
}

}  // namespace

// first tile if the list is one contiguous range of clean tiles, else ~0u
u32 prf_flat_base(const u32 *list, size_t n) {
    if (n == 0 || (list[0] & PRF_LAUNCH_MIXED)) return ~0u;
    for (size_t i = 1; i < n; i++)
        if (list[i] != list[0] + (u32)i) return ~0u;
    return list[0];
}

int prf_vertical_pack(hipStream_t s, const uint8_t *asc, u64 G, prf_vplanes *vp) {
    const u64 ntiles = G / PRF_TILE;  // includes the sentinel tile
    hipError_t e;
    const size_t plane_bytes = (size_t)ntiles * RG * 64 * sizeof(uint4);
    if ((e = hipMalloc((void **)&vp->VH, plane_bytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void **)&vp->VL, plane_bytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void **)&vp->tile_class, 2 * ntiles)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void **)&vp->launch_list, sizeof(u32) * ntiles)) != hipSuccess) return (int)e;
    vp->ntiles_alloc = ntiles;
    unsigned char *any_all = vp->tile_class + ntiles;
    hipLaunchKernelGGL(prf_pack_vertical_kernel, dim3((u32)ntiles), dim3(64), 0, s, asc, vp->VH, vp->VL, any_all);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(prf_tile_class_kernel, dim3((u32)((ntiles + 255) / 256)), dim3(256), 0, s, any_all, vp->tile_class, ntiles);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    // launch list (host side: one byte per 65536 positions)
    vp->h_class.resize(ntiles);
    if ((e = hipMemcpyAsync(vp->h_class.data(), vp->tile_class, ntiles, hipMemcpyDeviceToHost, s)) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
    vp->h_list.clear();
    vp->h_list.reserve(ntiles);
    for (u64 t = 0; t + 1 < ntiles; t++) {  // the sentinel tile is never scanned
        if (vp->h_class[t] == 0) vp->h_list.push_back((u32)t);
        else if (vp->h_class[t] == 1) vp->h_list.push_back((u32)t | PRF_LAUNCH_MIXED);
    }
    vp->n_launch = (u32)vp->h_list.size();
    vp->flat_base = prf_flat_base(vp->h_list.data(), vp->h_list.size());
    if (!vp->h_list.empty()) {
        if ((e = hipMemcpyAsync(vp->launch_list, vp->h_list.data(), sizeof(u32) * vp->h_list.size(), hipMemcpyHostToDevice, s)) != hipSuccess)
            return (int)e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
    }
    return 0;
}
