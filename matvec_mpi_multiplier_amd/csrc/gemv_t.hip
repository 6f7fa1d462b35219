// fp64 transposed GEMV for gfx950 (MI355X): y = A^T z on the same row-major A that gemv.hip
// multiplies from the right (no counterpart in the reference, whose drivers only form A x).
//
//   y[j] = sum_i A[i*lda + j] * z[i]      j < k, i < m
//
// The same A is streamed once, HBM-bound, with the opposite reduction geometry: columns are summed
// down the rows, so a lane that owns a column needs no cross-lane step at all.
//
// Mapping (gemvt_strip): a workgroup of NW waves owns a band of band_rows rows and a strip of
// 64*CPL columns. Wave w takes rows w, w + NW, ... of the band; a lane owns CPL columns of the
// strip and keeps UNR rows of loads in flight behind the FMAs (16-B global_load_dwordx4 with the
// non-temporal hint, CPL/2 per row; z[i] is wave-uniform). The NW per-wave partials meet in LDS and
// are added in wave order; the workgroup stores its 64*CPL sums into y (one band) or into
// partial[band][j], and gemvt_reduce adds the bands (below). The block index runs strip-fastest:
// the resident workgroups read whole contiguous rows of one band, the sliding window the tree
// kernels rely on. No atomics anywhere: every sum has one fixed order, so y is deterministic from
// run to run and independent of what the workspace held.
//
// The last strip of a k that is no multiple of 64*CPL, and the scalar form (any lda, any 8-B
// alignment), read with guarded 8-B loads: nothing is read outside A[i, 0..k) and z[0..m), nothing
// stored outside y[0..k). A column's sum only ever sees its own column of A (times z), so a
// special value in column j reaches y[j] alone (per column here).
#include "common.h"

namespace mvg {

typedef double dbl2 __attribute__((ext_vector_type(2)));
// promises only 8-B alignment; still one global_load_dwordx4 (gemv.hip)
typedef double dbl2u __attribute__((ext_vector_type(2), aligned(8)));

// The strip column of a lane's j-th sum. 16-B form: load q covers 128 consecutive columns of the
// wave (two per lane); 8-B form: load j covers 64.
template <bool VEC>
__device__ __forceinline__ int strip_col(int lane, int j) {
    return VEC ? (j >> 1) * 128 + 2 * lane + (j & 1) : j * 64 + lane;
}

// One row's CPL values of a lane: p = the row at the strip's first column, cols = columns of A
// left from there (EDGE: the strip is cut by k and every load is guarded).
template <int CPL, bool VEC, bool EDGE>
__device__ __forceinline__ void load_row(const double* __restrict__ p, int lane, int64_t cols, double (&v)[CPL]) {
    if constexpr (VEC && !EDGE) {
#pragma unroll
        for (int q = 0; q < CPL / 2; ++q) {
            const dbl2 t = __builtin_nontemporal_load(reinterpret_cast<const dbl2u*>(p + q * 128 + 2 * lane));
            v[2 * q] = t.x;
            v[2 * q + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = strip_col<VEC>(lane, j);
            v[j] = (!EDGE || c < cols) ? __builtin_nontemporal_load(p + c) : 0.0;
        }
    }
}

// Wave w's rows r0 + w, r0 + w + NW, ... < r1 of the band, in that order, UNR at a time.
template <int NW, int CPL, int UNR, bool VEC, bool EDGE>
__device__ __forceinline__ void strip_rows(const double* __restrict__ a, int64_t lda, const double* __restrict__ z,
                                           int64_t r0, int64_t r1, int w, int lane, int64_t cols,
                                           double (&acc)[CPL]) {
    int64_t r = r0 + w;
    for (; r + (int64_t)(UNR - 1) * NW < r1; r += (int64_t)UNR * NW) {
        double v[UNR][CPL];
        double zz[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t ru = r + (int64_t)u * NW;
            zz[u] = z[ru];
            load_row<CPL, VEC, EDGE>(a + ru * lda, lane, cols, v[u]);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int j = 0; j < CPL; ++j) acc[j] = __builtin_fma(v[u][j], zz[u], acc[j]);
    }
    for (; r < r1; r += NW) {
        double v[CPL];
        const double zr = z[r];
        load_row<CPL, VEC, EDGE>(a + r * lda, lane, cols, v);
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] = __builtin_fma(v[j], zr, acc[j]);
    }
}

// out: y when there is one band (out_ld unused), else the workspace partial[band * out_ld + j].
template <int NW, int CPL, int UNR, bool VEC>
__global__ __launch_bounds__(NW * 64) void gemvt_strip(const double* __restrict__ A, int64_t lda,
                                                        const double* __restrict__ z, double* __restrict__ out,
                                                        int64_t M, int64_t K, int64_t band_rows, unsigned nstrips,
                                                        int64_t out_ld) {
    constexpr int SC = 64 * CPL;
    __shared__ double part[NW][SC];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: rows and z stay scalar
    const unsigned band = blockIdx.x / nstrips;
    const unsigned strip = blockIdx.x - band * nstrips;
    const int64_t c0 = (int64_t)strip * SC;
    const int64_t r0 = (int64_t)band * band_rows;
    const int64_t r1 = r0 + band_rows < M ? r0 + band_rows : M;

    double acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] = 0.0;
    if (c0 + SC <= K)
        strip_rows<NW, CPL, UNR, VEC, false>(A + c0, lda, z, r0, r1, w, lane, K - c0, acc);
    else
        strip_rows<NW, CPL, UNR, VEC, true>(A + c0, lda, z, r0, r1, w, lane, K - c0, acc);

#pragma unroll
    for (int j = 0; j < CPL; ++j) part[w][strip_col<VEC>(lane, j)] = acc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < SC; c += NW * 64) {
        double s = part[0][c];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) s += part[ww][c];
        if (c0 + c < K) out[(int64_t)band * out_ld + c0 + c] = s;
    }
}

// y[j] = sum_b partial[b*K + j]. A workgroup owns 64 columns; its kReduceGroups waves split the
// bands into that many runs of consecutive bands, each wave adds its run in band order (8 loads in
// flight), and the run sums are added in run order: one fixed order for a given band count, and
// no lane waits on bands * memory latency (524288 x 512 has 2048 bands and 512 columns).
constexpr int kReduceGroups = 16;
__global__ __launch_bounds__(kReduceGroups * 64) void gemvt_reduce(const double* __restrict__ partial,
                                                                    int64_t bands, double* __restrict__ y,
                                                                    int64_t K) {
    __shared__ double sums[kReduceGroups][64];
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t per = (bands + kReduceGroups - 1) / kReduceGroups;
    const int64_t runs = (bands + per - 1) / per;  // runs that hold a band
    const int64_t b0 = g * per;
    const int64_t b1 = b0 + per < bands ? b0 + per : bands;
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

__global__ void gemvt_zero(double* y, int64_t k) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = 0.0;
}

// ------------------------------------------------------------------ variant table
typedef void (*gemvt_fn)(const double*, int64_t, const double*, double*, int64_t, int64_t, int64_t, unsigned,
                         int64_t);

struct TVariant {
    const char* name;
    gemvt_fn fn;
    int threads;       // workgroup size (NW * 64)
    int strip_cols;    // columns one workgroup covers (64 * CPL)
    int64_t band_cap;  // tallest band the host picks for it
    bool vec;          // 16-B loads on whole strips
};

#define MVG_T(NW, CPL, UNR, VEC) gemvt_strip<NW, CPL, UNR, VEC>, NW * 64, 64 * CPL
// VGPRs / scratch per kernel (-Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2): beside
// each entry, none with scratch; LDS is NW * 64 * CPL * 8 bytes. gemvt_reduce: 38 VGPRs, 8 KiB.
static constexpr TVariant kTVariants[] = {
    {"auto", nullptr, 0, 0, 0, false},
    {"strip_w8_c4_u4_b256", MVG_T(8, 4, 4, true), 256, true},    // 50 VGPRs, no scratch
    {"strip_w8_c4_u4_b2048", MVG_T(8, 4, 4, true), 2048, true},  // the same kernel, taller bands
    {"strip_w8_c2_u8_b256", MVG_T(8, 2, 8, true), 256, true},    // 44
    {"strip_w4_c2_u8_b256", MVG_T(4, 2, 8, true), 256, true},    // 44
    {"strip_w4_c2_u4_b256", MVG_T(4, 2, 4, true), 256, true},    // 34
    {"scalar_w4_c2_u4", MVG_T(4, 2, 4, false), 256, false},      // 32
    {"scalar_w4_c2_u4_b2048", MVG_T(4, 2, 4, false), 2048, false},  // the same kernel, taller bands
    {"scalar_w4_c2_u8", MVG_T(4, 2, 8, false), 256, false},      // 46
    {"scalar_w8_c2_u4", MVG_T(8, 2, 4, false), 256, false},      // 32
    {"scalar_w4_c1_u8", MVG_T(4, 1, 8, false), 256, false},      // 28
};
#undef MVG_T
constexpr int kNumTVariants = (int)(sizeof(kTVariants) / sizeof(kTVariants[0]));
constexpr int kTTall = variant_id(kTVariants, "scalar_w4_c2_u4_b2048");
constexpr int kTShort = variant_id(kTVariants, "scalar_w4_c1_u8");
static_assert(kTTall > 0 && kTShort > 0 && !kTVariants[kTTall].vec && !kTVariants[kTShort].vec,
              "dispatch names a missing variant, or one that needs 16-B loads");

constexpr int64_t kMinBandRows = 32;   // one unrolled step of every wave
constexpr int64_t kBandRows = 256;     // workspace traffic 16*bands*k <= 0.8 % of 8*m*k
constexpr int64_t kTallRows = 25600;   // from here on bands never get shorter than kBandRows
constexpr int64_t kFillBlocks = 512;   // two workgroups per CU: the grid fills the chip
constexpr int64_t kTallBlocks = 4096;  // a taller band must still leave this many workgroups

// From two sweeps on two MI355X boxes (profiles/r07/gemv_t/sweep.jsonl and
// sweep_before_pick.jsonl, MEASUREMENTS §16), the four shapes 16384^2, 65536 x 8192,
// 65536 x 32768, 524288 x 512: the 8-B forms with 64- or 128-column strips beat every 16-B form
// swept (256-column strips take 13-27 % longer, and 8-10 % of that comes from rows a power of two
// apart; the 8-B forms lose nothing there), so both picks read 8 bytes per lane and serve any lda
// and any 8-B alignment alike.
//   m >= 25600   4 waves x 128 columns, bands of up to 2048 rows while 4096 workgroups remain:
//                the best form at 65536 x 32768 (2436 / 2450 us in the two runs) and
//                524288 x 512 (318 / 321 us, 4-8 % ahead of the next), at most 0.5 % off the best
//                at 65536 x 8192
//   m <  25600   4 waves x 64 columns, 8 rows in flight: 16384^2 in 306.9 / 316.8 us, 2.6 % / 1.9 %
//                ahead of the form above (which runs 256-row bands there): at the 2 % house bar
// Everything else, k < 128 included, is not tuned: it takes the pick of its m.
static int pick_t_variant(int64_t /*lda*/, int64_t m, int64_t /*k*/) { return m >= kTallRows ? kTTall : kTShort; }


// How variant v cuts an m x k problem: decided from the arguments alone.
//  (a) m < 25600: bands shrink from 256 rows down to 32 until the grid has 512 workgroups, so a
//      short problem still fills the chip (its workspace share grows to at most 16/(8*32));
//  (b) m >= 25600: 256-row bands, or taller ones (up to the variant's cap) while 4096 workgroups
//      remain, so the workspace traffic stays at or below 0.8 % of A's;
//  (c) the grid cap (gridDim.x * blockDim.x < 2^32): bands grow until the grid fits; more strips
//      than one launch holds is refused.
struct TPlan {
    int64_t band_rows, bands, nstrips;
};
static int plan_t(const TVariant& var, int64_t m, int64_t k, TPlan* out) {
    const int64_t max_blocks = (1ll << 31) / var.threads;
    const int64_t nstrips = (k + var.strip_cols - 1) / var.strip_cols;
    if (nstrips > max_blocks) return fail(MVG_E_INVALID, "mvg_gemv_t: too many column strips for one grid");
    auto bands_of = [&](int64_t b) { return (m + b - 1) / b; };
    int64_t b = kBandRows;
    if (m < kTallRows) {
        while (b > kMinBandRows && bands_of(b) * nstrips < kFillBlocks) b /= 2;
    } else {
        while (b < var.band_cap && bands_of(2 * b) * nstrips >= kTallBlocks) b *= 2;
    }
    if (nstrips > 0 && bands_of(b) * nstrips > max_blocks) {
        const int64_t max_bands = max_blocks / nstrips;
        b = ((m + max_bands - 1) / max_bands + kMinBandRows - 1) / kMinBandRows * kMinBandRows;
    }
    out->band_rows = b;
    out->bands = bands_of(b);
    out->nstrips = nstrips;
    return MVG_OK;
}

// y[j] = sum_b partial[b*k + j] on s (declared in common.h: gemv_ata.hip adds its bands with it too)
int launch_band_reduce(const double* partial, int64_t bands, double* y, int64_t k, hipStream_t s) {
    const int64_t rblocks = (k + 63) / 64 < (1 << 20) ? (k + 63) / 64 : (1 << 20);
    hipLaunchKernelGGL(gemvt_reduce, dim3((unsigned)rblocks), dim3(kReduceGroups * 64), 0, s, partial, bands, y, k);
    MVG_HIP(hipGetLastError());
    return MVG_OK;
}

static int launch_t(int v, const double* A, int64_t lda, const double* z, double* y, int64_t m, int64_t k,
                    hipStream_t s) {
    const TVariant& var = kTVariants[v];
    TPlan p;
    if (int rc = plan_t(var, m, k, &p); rc != MVG_OK) return rc;
    if (int rc = take_pending_error("mvg_gemv_t"); rc != MVG_OK) return rc;  // before our first HIP call
    double* out = y;
    if (p.bands > 1) {
        int rc = workspace(s, (size_t)(p.bands * k), &out);
        if (rc != MVG_OK) return rc;
    }
    hipLaunchKernelGGL(var.fn, dim3((unsigned)(p.bands * p.nstrips)), dim3(var.threads), 0, s, A, lda, z, out, m, k,
                       p.band_rows, (unsigned)p.nstrips, k);
    MVG_HIP(hipGetLastError());
    if (p.bands > 1) return launch_band_reduce(out, p.bands, y, k, s);
    return MVG_OK;
}

// argument checks shared by the launch and the plan: sizes, variant
static int check_t_shape(int64_t lda, int64_t m, int64_t k, int variant) {
    if (m < 0 || k < 0) return fail(MVG_E_INVALID, "mvg_gemv_t: negative size");
    if (variant < 0 || variant >= kNumTVariants) return fail(MVG_E_INVALID, "mvg_gemv_t: bad variant");
    if (k > 0 && lda < k) return fail(MVG_E_INVALID, "mvg_gemv_t: lda < k");
    return MVG_OK;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_gemv_t_variant_count(void) { return kNumTVariants; }

int mvg_gemv_t_auto_variant(int64_t lda, int64_t m, int64_t k) { return pick_t_variant(lda, m, k); }

const char* mvg_gemv_t_variant_name(int v) {
    if (v < 0 || v >= kNumTVariants) return "invalid";
    return kTVariants[v].name;
}

int mvg_gemv_t_plan(int64_t lda, int64_t m, int64_t k, int variant, int64_t* band_rows, int64_t* bands,
                    int64_t* strip_cols) {
    if (int rc = check_t_shape(lda, m, k, variant); rc != MVG_OK) return rc;
    if (!band_rows || !bands || !strip_cols) return fail(MVG_E_INVALID, "mvg_gemv_t_plan: null");
    const TVariant& var = kTVariants[variant == 0 ? pick_t_variant(lda, m, k) : variant];
    TPlan p;
    if (int rc = plan_t(var, m, k, &p); rc != MVG_OK) return rc;
    *band_rows = p.band_rows;
    *bands = p.bands;
    *strip_cols = var.strip_cols;
    return MVG_OK;
}

int mvg_gemv_t_variant(const double* A, int64_t lda, const double* z, double* y, int64_t m, int64_t k, int variant,
                       void* stream) {
    if (int rc = check_t_shape(lda, m, k, variant); rc != MVG_OK) return rc;
    if (k == 0) return MVG_OK;
    if (!y) return fail(MVG_E_INVALID, "mvg_gemv_t: null y");
    if (m > 0 && (!A || !z)) return fail(MVG_E_INVALID, "mvg_gemv_t: null A or z");
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {  // the empty sum
        if (int rc = take_pending_error("mvg_gemv_t"); rc != MVG_OK) return rc;
        hipLaunchKernelGGL(gemvt_zero, dim3((unsigned)((k + 255) / 256 < 4096 ? (k + 255) / 256 : 4096)), dim3(256), 0,
                           s, y, k);
        MVG_HIP(hipGetLastError());
        return MVG_OK;
    }
    return launch_t(variant == 0 ? pick_t_variant(lda, m, k) : variant, A, lda, z, y, m, k, s);
}

int mvg_gemv_t(const double* A, int64_t lda, const double* z, double* y, int64_t m, int64_t k, void* stream) {
    return mvg_gemv_t_variant(A, lda, z, y, m, k, 0, stream);
}

}  // extern "C"
