// vscan_common.h -- a section of scan_vertical.hip, included exactly once inside its anonymous namespace; not an interface.
// Layout constants, LDS header and address-space types, the tile context and the cofactor table: what the verification
// routines (vscan_verify.h), the scan tasks (vscan_tasks.h) and the kernel share.  (static_for: prf_static_for.h.)

using prf_layout::T; using prf_layout::RG; using prf_layout::LIN_PRE; using prf_layout::LIN_POST; using prf_layout::LW;  // (prf_plan.h)
static_assert(prf_layout::TILE_WORDS == (int)PRF_TILE_WORDS, "tile size");
static_assert(LW % 2 == 0, "the window travels in 16-byte pieces");
constexpr u32 WIN_LEAD = 64u * (u32)LIN_PRE;                  // window positions in front of the tile
using prf_layout::REC_CAP; using prf_layout::FLAG_CAP; using prf_layout::SLOW_CAP;
constexpr int MAX_WAVES = PRF_VMAX_WAVES;
constexpr int NTH = 64 * MAX_WAVES;                           // threads per workgroup, always
using prf_layout::SMALL_M;
using prf_layout::ROW_CAP_LDS; using prf_layout::QCAP;
static_assert(QCAP % 16 == 0 && ROW_CAP_LDS == 4 * QCAP, "a wave ranks one sublist in 16-byte reads, batches of up to four per lane, that stay inside it");

// ---- group-task candidate records: [5:0] lane, [14:6] k, [16:15] 1/2/3 = every 1st/2nd/4th group examined,
// [48:17] stream word (bit b = stream b*64 + lane may hold a candidate) ----
__device__ __forceinline__ u64 make_rec(u32 lane, u32 k, u32 sc, u32 word) {
    return (u64)(lane | (k << 6) | (sc << 15)) | ((u64)word << 17);
}

// The same record as the two dwords that are stored, for a tag = make_rec_tag(lane, k, sc) -- or that of the task's first motif size
// plus (i << 6) for size k0 + i, which cannot carry out of the k field while k0 + i <= PRF_VMAX_K.
typedef u32 prf_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) prf_u32x2 prf_lds_u32x2;
static_assert(PRF_VMAX_K < (1 << 9), "k is a 9-bit field of a record");
__device__ __forceinline__ u32 make_rec_tag(u32 lane, u32 k, u32 sc) { return lane | (k << 6) | (sc << 15); }
__device__ __forceinline__ prf_u32x2 make_rec_halves(u32 tag, u32 word) {
    prf_u32x2 r = {tag | (word << 17), word >> 15};
    return r;
}

// dynamic LDS: [header][R1: image / window][recs][row keys][row motif sizes][all-N stream masks][flag lists, counts][boundary items][cofactors]
extern __shared__ __attribute__((aligned(16))) unsigned char prf_smem[];
using prf_layout::SMEM_HDR;
// header words: 128.. two sets of tile counters used alternately (a set is reset while the other one is still read)
constexpr int HDR_CNT = 128;       // [parity][CNT_N] u32
constexpr int HDR_NEXT = 256;      // {next launch slot, its entry}
constexpr int HDR_LONG = 264;      // [PRF_LONG_PER_TILE] u64: true ends of the rows whose span is clipped
constexpr int HDR_STATS = 296;     // {candidates looked at, of which verified on the spot} by this workgroup so far (thread 0's)
static_assert(HDR_LONG + 8 * (int)PRF_LONG_PER_TILE <= HDR_STATS && HDR_STATS + 8 <= SMEM_HDR, "LDS header layout");
// CNT_ROWS + q: rows that start in quarter q of the tile (key >> 30), those behind the sublist's QCAP included; CNT_OVF: the latter
// over all quarters = their slots in the slab.  The tile's row count is the sum of the four.
constexpr u32 CNT_N = 16, CNT_ROWS = 0, CNT_RECS = 4, CNT_EARLY = 5, CNT_LONG = 6, CNT_FLAGS = 7, CNT_SLOW = 8, CNT_OVF = 9,
              CNT_ROWS0 = 10, CNT_OVF0 = 14, CNT_LONG0 = 15;  // rows / long rows listed before the verification began (the scan's overflow paths)
static_assert(HDR_CNT % 16 == 0 && CNT_ROWS % 4 == 0 && HDR_CNT + 2 * 4 * (int)CNT_N <= HDR_NEXT, "the four row counters are one 16-byte read");
// sublist q is padded with the largest key of its quarter: differences of two keys of a sublist keep their sign
__device__ __forceinline__ u32 quarter_pad(u32 q) { return ((q + 1u) << 30) - 1u; }

// LDS is addressed through explicit address-space pointers everywhere: a generic pointer that the compiler cannot trace back
// to prf_smem becomes a flat_load, which is slower and waits on both memory counters.
typedef u32 prf_u32x4 __attribute__((ext_vector_type(4)));  // (HIP's uint4 class cannot be copied out of an explicit address space)
typedef __attribute__((address_space(3))) const prf_u32x4 prf_lds_cu4;
typedef __attribute__((address_space(3))) prf_u32x4 prf_lds_u4;
typedef __attribute__((address_space(3))) u64 prf_lds_u64;
typedef __attribute__((address_space(3))) u32 prf_lds_u32;
typedef __attribute__((address_space(3))) const u32 prf_lds_cu32;
typedef __attribute__((address_space(3))) void prf_lds_void;
typedef __attribute__((address_space(1))) const void prf_glb_cvoid;
typedef __attribute__((address_space(1))) const u32 prf_glb_cu32;
typedef __attribute__((address_space(1))) u64 prf_glb_u64;

// Diagnostic build only (make STAMPS=1 -> libprf_stamps.so): per-wave s_memtime stamps at the phase boundaries, written
// to a debug buffer that nothing else reads.  The product build has no stamp.
#ifdef PRF_STAMPS
#define PRF_STAMP(i)                                                                                               \
    do {                                                                                                           \
        if (g.dbg && lane == 0) g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// Slot 16: cycles of the tile's rows phase that the wave spent ranking (key reads, compares, DPP adds), summed over its passes;
// the staging issue in front of it and the slab stores behind it are outside.  (The asm pins the rank in front of the second stamp.)
#define PRF_RANK_DECL() u64 rank_cyc = 0, rank_t0 = 0
#define PRF_RANK_T0() do { rank_t0 = __builtin_amdgcn_s_memtime(); } while (0)
#define PRF_RANK_T1(v)                                            \
    do {                                                          \
        asm volatile("" : "+v"(v));                               \
        rank_cyc += __builtin_amdgcn_s_memtime() - rank_t0;       \
    } while (0)
#define PRF_RANK_STORE()                                                                                    \
    do {                                                                                                    \
        if (g.dbg && lane == 0) g.dbg[((u64)slot * MAX_WAVES + wave) * PRF_STAMP_SLOTS + 16] = rank_cyc; \
    } while (0)
#else
#define PRF_STAMP(i) do { } while (0)
#define PRF_RANK_DECL() do { } while (0)
#define PRF_RANK_T0() do { } while (0)
#define PRF_RANK_T1(v) do { } while (0)
#define PRF_RANK_STORE() do { } while (0)
#endif

// what the verification step needs about the tile; lives at the start of LDS
struct TileCtx {
    u64 w0;                   // first word of the linear window
    u64 xz_lo, xz_hi;         // positions known to hold no not-ACGT symbol
    const u64 *H, *L, *X;     // linear planes in HBM
    const u64 *const *E;      // device array of the five planes of the symbols outside ACGTN, or nullptr (prf_planes::E)
    prf_glb_u64 *slab;        // this tile's row slab in HBM (explicitly global: a generic pointer read back from LDS becomes FLAT stores)
    u64 tile_base;            // first position of the tile
    u32 slab_cap;
    u32 min_repeats, min_span;
    u32 lin_off;              // byte offset of R1 (the linear window, once staged) in LDS
    u32 has_lin;              // the linear window is staged (after the scan)
    u32 keys_off;             // byte offset of the row list (keys, then motif sizes) in LDS
    u32 cof_off;              // byte offset of the cofactor table in LDS
    u32 slow_off;             // byte offset of the list of deferred candidates in LDS
    u32 k_exact0;             // exact tasks of the plan: motif sizes k_exact0 ..., task index = k - k_exact0
    u32 cnt_off;              // byte offset of this tile's counter set in LDS
};
static_assert(sizeof(TileCtx) <= 128, "TileCtx must fit its LDS header slot");

// cof[k]: the cofactors k/p of the distinct primes p | k, one per byte, largest first (k <= 480 has at most 4
// distinct primes and k/p <= 240).  The motif seq[a:a+k] is primitive iff it has none of these periods
// (reference consists_of_perfect_repeats, utils/perfect_repeat_tracker.py:108-142, tries every divisor).
// Entries 0 .. kmax of the scan are copied to LDS once per workgroup: a table look, not a run-time division, per candidate.
struct CofTable {
    u32 v[PRF_VMAX_K + 4];
    constexpr CofTable() : v{} {
        for (u32 k = 2; k <= PRF_VMAX_K; k++) {
            u32 rest = k, packed = 0, n = 0;
            for (u32 p = 2; p <= rest; p++) {
                if (rest % p) continue;
                packed |= (k / p) << (8 * n++);
                while (rest % p == 0) rest /= p;
            }
            v[k] = packed;
        }
    }
};
__constant__ const CofTable prf_cof_table{};
