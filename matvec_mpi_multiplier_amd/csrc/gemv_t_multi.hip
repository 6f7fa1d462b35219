// fp64 transposed product for a block of vectors on gfx950 (MI355X): Y = A^T Z in one pass over
// the row-major A per group of vectors (the mirror image of mvg_gemv_multi; no counterpart in the
// reference).
//
//   Y[j + v*ldy] = sum_i A[i*lda + j] * Z[i + v*ldz]      j < k, i < m, v < nv
//
// Geometry (gemvtm_strip): gemv_t.hip's, with NV sums per column. A workgroup of NW waves owns a
// band of band_rows rows and a strip of 64*CPL columns; a lane owns CPL columns of the strip (8-B
// non-temporal loads, a lane per 64-column stride: the form that won the one-vector sweep, any lda
// and any 8-B alignment) and keeps NV*CPL sums. The band is walked in blocks of NW*UNR rows; wave w
// takes the UNR consecutive rows w*UNR.. of a block, so the UNR values of one vector that it needs
// are contiguous in the column-major Z and wave-uniform: scalar loads, UNR*NV doubles per step.
// Each loaded A value feeds NV FMAs. The NW per-wave sums meet in LDS, four vectors at a time, and
// are added in wave order; the workgroup stores into Y (one band) or into partial[v][band][j] in
// the per-(device, stream) workspace, and gemvtm_reduce adds the bands of all vectors of the group
// in one launch, in gemvt_reduce's order. No atomics: every sum has one fixed order.
//
// A group shorter than NV: the spare chains read the group's last vector again and are never
// stored, so no chain sees memory the caller did not pass and a special value in Z[i, v] stays in
// column v. Rows beyond m are never read (the last rows of a band go one at a time), columns beyond
// k are not loaded (+0.0) and not stored.
#include "common.h"

namespace mvg {

// One row's CPL values of a lane: p = the row at the strip's first column, cols = columns of A
// left from there (EDGE: the strip is cut by k and every load is guarded).
template <int CPL, bool EDGE>
__device__ __forceinline__ void tm_load_row(const double* __restrict__ p, int lane, int64_t cols, double (&v)[CPL]) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = j * 64 + lane;
        v[j] = (!EDGE || c < cols) ? __builtin_nontemporal_load(p + c) : 0.0;
    }
}

// Rows rs .. rs + NR - 1 (wave-uniform) into the NV chains. FULL: the group has NV vectors; else g
// of them, and the chains from g on read vector g - 1 again. The offset into Z walks from vector
// to vector and is hidden from the optimiser between two chains (an empty asm on its SGPR pair):
// left alone it keeps NV loop-invariant vector offsets in SGPRs beside the UNR * NV values of Z,
// which does not fit the 102 a wave has.
template <int CPL, int NR, int NV, bool EDGE, bool FULL>
__device__ __forceinline__ void tm_step(const double* __restrict__ a, int64_t lda, const double* __restrict__ z,
                                        int64_t ldz, int g, int64_t rs, int lane, int64_t cols,
                                        double (&acc)[NV][CPL]) {
    double v[NR][CPL];
#pragma unroll
    for (int u = 0; u < NR; ++u) tm_load_row<CPL, EDGE>(a + (rs + u) * lda, lane, cols, v[u]);
    // All NR rows of one chain's Z come in one scalar load of 8 * NR bytes, CB chains at
    // a time, so that at most 32 doubles of Z (64 SGPRs) are live: the scheduler may not move the next
    // block's loads over this block's FMAs. Few wide scalar loads matter: the 16-chain forms that
    // fetched two rows per load ran at the pace of their scalar loads, not of A (MEASUREMENTS §18).
    constexpr int CB = NR * NV <= 32 ? NV : (NR >= 32 ? 1 : 32 / NR);
    if constexpr (!FULL) asm volatile("" : "+s"(g));  // the selects below stay in the loop
    int64_t zo = rs;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        if (c > 0 && c % CB == 0) __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+s"(zo));
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const double zz = z[zo + u];
#pragma unroll
            for (int j = 0; j < CPL; ++j) acc[c][j] = __builtin_fma(v[u][j], zz, acc[c][j]);
        }
        zo += (FULL || c + 1 < g) ? ldz : 0;
    }
}

// The band's rows [r0, r1) in blocks of NW * UNR: wave w's rows of a block are w*UNR .. w*UNR + UNR - 1,
// in that order; the rows of a block cut by r1 (the band's last block only) go one at a time.
template <int NW, int CPL, int UNR, int NV, bool EDGE, bool FULL>
__device__ __forceinline__ void tm_rows(const double* __restrict__ a, int64_t lda, const double* __restrict__ z,
                                        int64_t ldz, int g, int64_t r0, int64_t r1, int w, int lane, int64_t cols,
                                        double (&acc)[NV][CPL]) {
    int64_t rs = r0 + (int64_t)w * UNR;
    for (; rs + UNR <= r1; rs += (int64_t)NW * UNR) tm_step<CPL, UNR, NV, EDGE, FULL>(a, lda, z, ldz, g, rs, lane, cols, acc);
    for (; rs < r1; ++rs) tm_step<CPL, 1, NV, EDGE, FULL>(a, lda, z, ldz, g, rs, lane, cols, acc);
}

// out[v * out_vs + band * out_bs + j]: Y itself when there is one band (out_vs = ldy), else the
// workspace partial[v][band][j] (out_vs = bands * K, out_bs = K).
template <int NW, int CPL, int UNR, int NV>
__global__ __launch_bounds__(NW * 64) void gemvtm_strip(const double* __restrict__ A, int64_t lda,
                                                         const double* __restrict__ Z, int64_t ldz,
                                                         double* __restrict__ out, int64_t out_vs, int64_t out_bs,
                                                         int64_t M, int64_t K, int64_t band_rows, unsigned nstrips,
                                                         int g) {
    constexpr int SC = 64 * CPL;
    constexpr int VC = NV < 4 ? NV : 4;  // vectors per LDS round
    __shared__ double part[NW][VC][SC];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: rows and Z stay scalar
    const unsigned band = blockIdx.x / nstrips;
    const unsigned strip = blockIdx.x - band * nstrips;
    const int64_t c0 = (int64_t)strip * SC;
    const int64_t r0 = (int64_t)band * band_rows;
    const int64_t r1 = r0 + band_rows < M ? r0 + band_rows : M;

    double acc[NV][CPL];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[c][j] = 0.0;
    const bool whole = c0 + SC <= K;
    if (g == NV) {
        if (whole)
            tm_rows<NW, CPL, UNR, NV, false, true>(A + c0, lda, Z, ldz, g, r0, r1, w, lane, K - c0, acc);
        else
            tm_rows<NW, CPL, UNR, NV, true, true>(A + c0, lda, Z, ldz, g, r0, r1, w, lane, K - c0, acc);
    } else {
        if (whole)
            tm_rows<NW, CPL, UNR, NV, false, false>(A + c0, lda, Z, ldz, g, r0, r1, w, lane, K - c0, acc);
        else
            tm_rows<NW, CPL, UNR, NV, true, false>(A + c0, lda, Z, ldz, g, r0, r1, w, lane, K - c0, acc);
    }

#pragma unroll
    for (int vb = 0; vb < NV; vb += VC) {
        if (vb) __syncthreads();  // the round before has been read
#pragma unroll
        for (int c = 0; c < VC; ++c)
#pragma unroll
            for (int j = 0; j < CPL; ++j) part[w][c][j * 64 + lane] = acc[vb + c][j];
        __syncthreads();
        for (int e = threadIdx.x; e < VC * SC; e += NW * 64) {
            const int c = e / SC, col = e - c * SC;
            double s = part[0][c][col];
#pragma unroll
            for (int ww = 1; ww < NW; ++ww) s += part[ww][c][col];
            if (vb + c < g && c0 + col < K) out[(int64_t)(vb + c) * out_vs + (int64_t)band * out_bs + c0 + col] = s;
        }
    }
}

// Y[j + v*ldy] = sum_b partial[v*vs + b*K + j], v = blockIdx.y: gemvt_reduce (gemv_t.hip) per
// vector of the group, in its order: a workgroup owns 64 columns, its 16 waves split the bands
// into runs of consecutive bands, each adds its run in band order and the runs are added in run order.
constexpr int kMReduceGroups = 16;
__global__ __launch_bounds__(kMReduceGroups * 64) void gemvtm_reduce(const double* __restrict__ partial, int64_t vs,
                                                                      int64_t bands, double* __restrict__ Y,
                                                                      int64_t ldy, int64_t K) {
    __shared__ double sums[kMReduceGroups][64];
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t per = (bands + kMReduceGroups - 1) / kMReduceGroups;
    const int64_t runs = (bands + per - 1) / per;  // runs that hold a band
    const int64_t b0 = g * per;
    const int64_t b1 = b0 + per < bands ? b0 + per : bands;
    partial += (int64_t)blockIdx.y * vs;
    double* __restrict__ y = Y + (int64_t)blockIdx.y * ldy;
    // column blocks beyond the grid (its size is capped on the host) are walked in a stride
    for (int64_t j0 = (int64_t)blockIdx.x * 64; j0 < K; j0 += (int64_t)gridDim.x * 64) {
        const int64_t j = j0 + lane;
        double s = 0.0;
        if (j < K) {
            const double* p = partial + j;
            int64_t b = b0;
            for (; b + 7 < b1; b += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(b + u) * K];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; b < b1; ++b) s += p[b * K];
        }
        sums[g][lane] = s;
        __syncthreads();
        if (g == 0 && j < K) {
            double t = sums[0][lane];
            for (int gg = 1; gg < runs; ++gg) t += sums[gg][lane];
            y[j] = t;
        }
        __syncthreads();
    }
}

int launch_band_reduce_multi(const double* partial, int64_t vs, int64_t bands, double* Y, int64_t ldy, int64_t k, int g,
                             hipStream_t s) {
    const int64_t rblocks = (k + 63) / 64 < (1 << 20) ? (k + 63) / 64 : (1 << 20);
    hipLaunchKernelGGL(gemvtm_reduce, dim3((unsigned)rblocks, (unsigned)g), dim3(kMReduceGroups * 64), 0, s, partial, vs,
                       bands, Y, ldy, k);
    MVG_HIP(hipGetLastError());
    return MVG_OK;
}

// ------------------------------------------------------------------ variant table
typedef void (*gemvtm_fn)(const double*, int64_t, const double*, int64_t, double*, int64_t, int64_t, int64_t, int64_t,
                          int64_t, unsigned, int);

struct MVariant {
    const char* name;
    gemvtm_fn fn;    // nullptr: auto, separate
    int threads;     // workgroup size (NW * 64)
    int strip_cols;  // columns one workgroup covers (64 * CPL)
    int nv;          // chains: vectors per pass over A
};

#define MVG_TM(NW, CPL, UNR, NV) gemvtm_strip<NW, CPL, UNR, NV>, NW * 64, 64 * CPL, NV
// VGPRs / SGPRs per kernel (-Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2) beside each
// entry, none with scratch; LDS is NW * min(NV, 4) * 64 * CPL * 8 bytes. gemvtm_reduce: 38 VGPRs,
// 8 KiB.
static constexpr MVariant kMVariants[] = {
    {"auto", nullptr, 0, 0, 0},
    {"separate", nullptr, 0, 0, 1},  // one mvg_gemv_t per vector
    {"tstripm_w4_c1_u8_v2", MVG_TM(4, 1, 8, 2)},  // 28 VGPRs, 92 SGPRs
    {"tstripm_w4_c1_u4_v4", MVG_TM(4, 1, 4, 4)},  // 32, 83
    {"tstripm_w4_c1_u4_v8", MVG_TM(4, 1, 4, 8)},  // 40, 104
    {"tstripm_w4_c1_u2_v16", MVG_TM(4, 1, 2, 16)},  // 48, 100
    {"tstripm_w4_c2_u4_v2", MVG_TM(4, 2, 4, 2)},  // 36, 74
    {"tstripm_w4_c2_u4_v4", MVG_TM(4, 2, 4, 4)},  // 44, 90
    {"tstripm_w4_c2_u2_v8", MVG_TM(4, 2, 2, 8)},  // 52, 82
    {"tstripm_w4_c2_u2_v16", MVG_TM(4, 2, 2, 16)},  // 84, 100
    {"tstripm_w4_c1_u8_v8", MVG_TM(4, 1, 8, 8)},  // 46, 99
    {"tstripm_w4_c1_u4_v16", MVG_TM(4, 1, 4, 16)},  // 48, 106
    {"tstripm_w4_c1_u8_v16", MVG_TM(4, 1, 8, 16)},  // 62, 99
    {"tstripm_w4_c2_u4_v16", MVG_TM(4, 2, 4, 16)},  // 92, 86
};
#undef MVG_TM
constexpr int kNumMVariants = (int)(sizeof(kMVariants) / sizeof(kMVariants[0]));
constexpr int kMSeparate = variant_id(kMVariants, "separate");
static_assert(kMSeparate == 1, "separate is variant 1 (include/matvec_gpu.h)");

constexpr int64_t kMMinBandRows = 32;    // one unrolled step of every wave
constexpr int64_t kMRowsPerChain = 128;  // band_rows = 128 * NV: workspace traffic 2 * NV / band_rows = 1.6 % of A's
constexpr int64_t kMFillBlocks = 512;    // two workgroups per CU: the grid fills the chip

constexpr int kM2Wide = variant_id(kMVariants, "tstripm_w4_c2_u4_v2"), kM2 = variant_id(kMVariants, "tstripm_w4_c1_u8_v2");
constexpr int kM4Wide = variant_id(kMVariants, "tstripm_w4_c2_u4_v4"), kM4 = variant_id(kMVariants, "tstripm_w4_c1_u4_v4");
constexpr int kM8Narrow = variant_id(kMVariants, "tstripm_w4_c1_u8_v8"), kM8 = variant_id(kMVariants, "tstripm_w4_c1_u4_v8");
constexpr int kM16Wide = variant_id(kMVariants, "tstripm_w4_c2_u4_v16"), kM16Tall = variant_id(kMVariants, "tstripm_w4_c1_u8_v16");
constexpr int kM16 = variant_id(kMVariants, "tstripm_w4_c2_u2_v16");
static_assert(kM2Wide > 0 && kM2 > 0 && kM4Wide > 0 && kM4 > 0 && kM8Narrow > 0 && kM8 > 0 && kM16Wide > 0 &&
                  kM16Tall > 0 && kM16 > 0,
              "dispatch names a missing variant");

constexpr int64_t kMSweptRows = 16384;      // the shortest swept shape
constexpr int64_t kMSweptCols = 64;         // the narrowest
constexpr int64_t kMSweptSize = 1ll << 28;  // the smallest: 16384^2, 524288 x 512, 4194304 x 64

// The variant for the group that opens a run of `rem` vectors: one with at most rem chains, so auto
// only ever launches full groups, or separate. From the sweeps kept under profiles/r07/gemv_t_multi/
// (MEASUREMENTS §18; six shapes, nv = 2, 4, 8, 16; two runs with every kernel in its final form,
// a third with the first eight): inside the swept range (m >= 16384, k >= 64, m * k >= 2^28) every
// pick takes 0.08-0.65 of separate's time at its own nv in every run, nowhere near the 2 % bar, so
// the choice is among the fused forms, each time the one ahead in both full runs:
//   16 chains, k >= 128: 128 <= k < 1024 c2_u4_v16 (524288 x 512: 826 us against 993-1001 for two
//     groups of 8); wider, from 65536 rows c1_u8_v16 (65536 x 8192: 841-853 against 1278-1395;
//     65536 x 32768: 2956-3030 against 3912-3917 for c2_u2_v16), below c2_u2_v16 (16384^2: 406
//     against 491 for c1_u8_v16)
//   8 chains, k >= 128: k < 1024 c1_u8_v8 (524288 x 512: 497-501 against 562-563 for c2_u2_v8), else
//     c1_u4_v8 (level with c1_u8_v8, 0.5-3 %); k < 128: no more than 4 chains (4194304 x 64, 16
//     vectors: four groups of 4 in 1793-1906 against 1957-1958 for two of 8; 8 vectors: 851-902
//     against 834-837, which is not ahead by 2 % of the better side in every run)
//   4 and 2 chains: 128 <= k < 1024 the 128-column strips (524288 x 512: 0.5-3 % ahead), else 64 columns
// Outside the swept range nothing was measured: separate, not tuned.
static int pick_tm_variant(int64_t /*lda*/, int64_t /*ldz*/, int64_t m, int64_t k, int rem) {
    if (rem < 2 || m < kMSweptRows || k < kMSweptCols || m < (kMSweptSize + k - 1) / k) return kMSeparate;
    const bool wide = k >= 128 && k < 1024;
    if (rem >= 16 && k >= 128) return wide ? kM16Wide : m >= 65536 ? kM16Tall : kM16;
    if (rem >= 8 && k >= 128) return k < 1024 ? kM8Narrow : kM8;
    if (rem >= 4) return wide ? kM4Wide : kM4;
    return wide ? kM2Wide : kM2;
}

// How a fused variant cuts an m x k problem, from the arguments alone (never from nv, so a
// column's bits do not depend on its group's size):
//  (a) bands of 128 rows per chain (256 .. 2048 rows): the partials of NV vectors cost
//      16 * bands * k * NV bytes, at most 1.6 % of A's 8 * m * k;
//  (b) they shrink (down to 32 rows) until the grid has 512 workgroups, so a short or narrow
//      problem still fills the chip; the four swept shapes keep (a) at strips of 64 and 128 columns;
//  (c) the grid cap (gridDim.x * blockDim.x < 2^32): bands grow until the grid fits; more strips
//      than one launch holds is refused.
struct MPlan {
    int64_t band_rows, bands, nstrips;
};
static int plan_tm(const MVariant& var, int64_t m, int64_t k, MPlan* out) {
    const int64_t max_blocks = (1ll << 31) / var.threads;
    const int64_t nstrips = (k + var.strip_cols - 1) / var.strip_cols;
    if (nstrips > max_blocks) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: too many column strips for one grid");
    auto bands_of = [&](int64_t b) { return (m + b - 1) / b; };
    int64_t b = kMRowsPerChain * var.nv;
    while (b > kMMinBandRows && bands_of(b) * nstrips < kMFillBlocks) b /= 2;
    if (nstrips > 0 && bands_of(b) * nstrips > max_blocks) {
        const int64_t max_bands = max_blocks / nstrips;
        b = ((m + max_bands - 1) / max_bands + kMMinBandRows - 1) / kMMinBandRows * kMMinBandRows;
    }
    out->band_rows = b;
    out->bands = bands_of(b);
    out->nstrips = nstrips;
    return MVG_OK;
}

// one group of g <= var.nv vectors (m, k > 0)
static int launch_tm(const MVariant& var, const MPlan& p, const double* A, int64_t lda, const double* Z, int64_t ldz,
                     double* Y, int64_t ldy, int64_t m, int64_t k, int g, hipStream_t s) {
    double* out = Y;
    int64_t out_vs = ldy, out_bs = 0;
    if (p.bands > 1) {
        int rc = workspace(s, (size_t)(p.bands * k * g), &out);
        if (rc != MVG_OK) return rc;
        out_vs = p.bands * k;
        out_bs = k;
    }
    hipLaunchKernelGGL(var.fn, dim3((unsigned)(p.bands * p.nstrips)), dim3(var.threads), 0, s, A, lda, Z, ldz, out,
                       out_vs, out_bs, m, k, p.band_rows, (unsigned)p.nstrips, g);
    MVG_HIP(hipGetLastError());
    if (p.bands > 1) return launch_band_reduce_multi(out, out_vs, p.bands, Y, ldy, k, g, s);
    return MVG_OK;
}

// Argument checks shared by the launch and the plan.
static int check_tm_shape(int64_t lda, int64_t ldz, int64_t m, int64_t k, int nv, int variant) {
    if (m < 0 || k < 0 || nv < 0) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: negative size or nv");
    if (variant < 0 || variant >= kNumMVariants) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: bad variant");
    if (k > 0 && lda < k) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: lda < k");
    if (k > 0 && nv > 0 && ldz < m) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: ldz < m");
    return MVG_OK;
}

// The group that opens a run of `rem` vectors. auto asks the dispatch group by group (it names a
// variant with at most rem chains, or separate), so every group it launches is a full one; an
// explicit fused variant takes min(rem, NV) vectors while at least two are left. *v == kMSeparate
// comes with *g == 1: one vector through mvg_gemv_t.
static void next_group(int variant, int64_t lda, int64_t ldz, int64_t m, int64_t k, int rem, int* v, int* g) {
    *v = variant == 0 ? pick_tm_variant(lda, ldz, m, k, rem) : variant;
    const MVariant& var = kMVariants[*v];
    if (!var.fn || rem < 2) {
        *v = kMSeparate;
        *g = rem < 1 ? rem : 1;
        return;
    }
    *g = rem < var.nv ? rem : var.nv;
}

// The grid limits of everything a call launches, group by group: a fused group's strips, and
// mvg_gemv_t's own for a vector that goes through it.
static int check_tm_grids(int variant, int64_t lda, int64_t ldz, int64_t m, int64_t k, int nv) {
    bool seen[kNumMVariants] = {};
    for (int rem = nv; rem > 0;) {
        int v, g;
        next_group(variant, lda, ldz, m, k, rem, &v, &g);
        if (!seen[v]) {
            seen[v] = true;
            MPlan p;
            int64_t b, n, sc;
            if (v != kMSeparate) {
                if (int rc = plan_tm(kMVariants[v], m, k, &p); rc != MVG_OK) return rc;
            } else if (mvg_gemv_t_plan(lda, m, k, 0, &b, &n, &sc) != MVG_OK) {
                return fail(MVG_E_INVALID, "mvg_gemv_t_multi: too many column strips for one grid (mvg_gemv_t)");
            }
        }
        rem -= g;
    }
    return MVG_OK;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_gemv_t_multi_variant_count(void) { return kNumMVariants; }

int mvg_gemv_t_multi_auto_variant(int64_t lda, int64_t ldz, int64_t m, int64_t k, int nv) {
    return pick_tm_variant(lda, ldz, m, k, nv);
}

const char* mvg_gemv_t_multi_variant_name(int v) {
    if (v < 0 || v >= kNumMVariants) return "invalid";
    return kMVariants[v].name;
}

int mvg_gemv_t_multi_plan(int64_t lda, int64_t m, int64_t k, int nv, int variant, int64_t* band_rows, int64_t* bands,
                          int64_t* strip_cols, int* group) {
    if (int rc = check_tm_shape(lda, m, m, k, nv, variant); rc != MVG_OK) return rc;
    if (!band_rows || !bands || !strip_cols || !group) return fail(MVG_E_INVALID, "mvg_gemv_t_multi_plan: null");
    if (int rc = check_tm_grids(variant, lda, m, m, k, nv > 0 ? nv : 1); rc != MVG_OK) return rc;
    int v;
    next_group(variant, lda, m, m, k, nv, &v, group);
    if (v == kMSeparate) return mvg_gemv_t_plan(lda, m, k, 0, band_rows, bands, strip_cols);  // mvg_gemv_t's own cut
    MPlan p;
    if (int rc = plan_tm(kMVariants[v], m, k, &p); rc != MVG_OK) return rc;
    *band_rows = p.band_rows;
    *bands = p.bands;
    *strip_cols = kMVariants[v].strip_cols;
    return MVG_OK;
}

int mvg_gemv_t_multi_variant(const double* A, int64_t lda, const double* Z, int64_t ldz, double* Y, int64_t ldy,
                             int64_t m, int64_t k, int nv, int variant, void* stream) {
    if (int rc = check_tm_shape(lda, ldz, m, k, nv, variant); rc != MVG_OK) return rc;
    if (nv > 0 && ldy < k) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: ldy < k");
    if (k == 0 || nv == 0) return MVG_OK;
    if (!Y) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: null Y");
    if (m > 0 && (!A || !Z)) return fail(MVG_E_INVALID, "mvg_gemv_t_multi: null A or Z");
    if (m == 0) variant = kMSeparate;  // the empty sum: mvg_gemv_t writes the zeros
    if (int rc = check_tm_grids(variant, lda, ldz, m, k, nv); rc != MVG_OK) return rc;
    bool taken = false;
    for (int done = 0; done < nv;) {
        int v, g;
        next_group(variant, lda, ldz, m, k, nv - done, &v, &g);
        const double* Zg = Z ? Z + (int64_t)done * ldz : Z;
        double* Yg = Y + (int64_t)done * ldy;
        if (v == kMSeparate) {  // mvg_gemv_t takes a pending error before its own first HIP call
            if (int rc = mvg_gemv_t(A, lda, Zg, Yg, m, k, stream); rc != MVG_OK) return rc;
        } else {
            if (!taken)  // before our first HIP call
                if (int rc = take_pending_error("mvg_gemv_t_multi"); rc != MVG_OK) return rc;
            taken = true;
            MPlan p;
            if (int rc = plan_tm(kMVariants[v], m, k, &p); rc != MVG_OK) return rc;
            if (int rc = launch_tm(kMVariants[v], p, A, lda, Zg, ldz, Yg, ldy, m, k, g, (hipStream_t)stream); rc != MVG_OK)
                return rc;
        }
        done += g;
    }
    return MVG_OK;
}

int mvg_gemv_t_multi(const double* A, int64_t lda, const double* Z, int64_t ldz, double* Y, int64_t ldy, int64_t m,
                     int64_t k, int nv, void* stream) {
    return mvg_gemv_t_multi_variant(A, lda, Z, ldz, Y, ldy, m, k, nv, 0, stream);
}

}  // extern "C"
