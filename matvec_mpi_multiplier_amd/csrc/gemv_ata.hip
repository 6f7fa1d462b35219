// fp64 fused normal-equations product for gfx950 (MI355X): t = A x and w = A^T t in one pass over
// the row-major A that gemv.hip and gemv_t.hip each stream once (no counterpart in the reference).
//
//   t[i] = sum_j A[i*lda + j] * x[j]      i < m
//   w[j] = sum_i A[i*lda + j] * t[i]      j < k, with the t[i] that was stored
//
// The row that has just produced t[i] is still in the registers that loaded it, so w += t[i] * row
// costs no second read. t[i] needs the whole row first, so a workgroup owns whole rows: the split is
// over rows alone. A workgroup takes a band of band_rows rows, keeps the k column sums of its band
// in registers, and stores them into w (one band) or into partial[band][0..k) in the
// per-(device, stream) workspace; gemv_t.hip's band reduce (launch_band_reduce) adds the bands.
//
// Two geometries:
//   ata_wrow   a wave per row, k <= 64*CPL. Wave w takes rows w, w + NW, ... of the band; a lane
//              owns columns lane, lane + 64, ... (8-B non-temporal loads, a lane per 64-column
//              stride: the layout that won the transposed sweep), holds its CPL entries of x and
//              CPL column sums, and keeps UNR rows of loads in flight. Per row: an FMA chain over
//              the lane's columns, the fixed-order DPP sum of the tree kernels (wave_sum.h), lane 0
//              stores t[i], then acc[j] = fma(v[j], t_i, acc[j]). No barrier in the row loop; the
//              NW per-wave sums meet in LDS once, at the band's end, in wave order.
//   ata_wgrow  a workgroup per row, k <= 64*NW*CPL. Wave w owns columns [w*64*CPL, +64*CPL) of
//              every row. The per-wave partial dots of RB rows go to LDS, meet at one barrier (the
//              LDS slots alternate, so one barrier per group is enough), and every wave adds the NW
//              partials in wave order: all waves hold the same t_i bits. A wave's column sums are
//              its own: they go straight out, no LDS merge.
// Columns beyond k contribute +0.0 and are never loaded or stored, rows beyond m in the last band
// are skipped, row offsets are 64-bit. No atomics anywhere: every sum has one fixed order for a
// given (variant, m, k), so t and w are the same bits from run to run whatever the workspace held.
// A NaN in A[i, j] reaches t[i] alone, and through t[i] every w[j] (0 * NaN included), as in the
// composed pair.
#include "ata_row.h"
#include "wave_sum.h"

namespace mvg {

// Rows r, r + NW, ... (NR of them) of one wave.
template <int NW, int CPL, int NR, bool EDGE>
__device__ __forceinline__ void wrow_step(const double* __restrict__ a, int64_t lda, double* __restrict__ t,
                                          int64_t r, int lane, int k, const double (&x)[CPL], double (&acc)[CPL]) {
    double v[NR][CPL];
    double ti[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) ata_load_row<CPL, EDGE>(a + (r + (int64_t)u * NW) * lda, 0, lane, k, v[u]);
#pragma unroll
    for (int u = 0; u < NR; ++u) ti[u] = group_sum_dpp<64>(ata_dot<CPL>(v[u], x));
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        if (lane == 0) t[r + (int64_t)u * NW] = ti[u];
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] = __builtin_fma(v[u][j], ti[u], acc[j]);
    }
}

// out: w when there is one band (out_ld unused), else the workspace partial[band * out_ld + j].
// EDGE: K < 64 * CPL.
template <int NW, int CPL, int UNR, bool EDGE>
__global__ __launch_bounds__(NW * 64) void ata_wrow(const double* __restrict__ A, int64_t lda,
                                                     const double* __restrict__ x, double* __restrict__ t,
                                                     double* __restrict__ out, int64_t M, int K, int64_t band_rows,
                                                     int64_t out_ld) {
    constexpr int SC = 64 * CPL;
    __shared__ double part[NW][SC];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: rows stay scalar
    const int64_t band = blockIdx.x;
    const int64_t r0 = band * band_rows;
    const int64_t r1 = r0 + band_rows < M ? r0 + band_rows : M;

    double xr[CPL], acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = j * 64 + lane;
        xr[j] = c < K ? x[c] : 0.0;
        acc[j] = 0.0;
    }
    // wave w's rows r0 + w, r0 + w + NW, ... < r1, in that order, UNR at a time
    int64_t r = r0 + w;
    for (; r + (int64_t)(UNR - 1) * NW < r1; r += (int64_t)UNR * NW)
        wrow_step<NW, CPL, UNR, EDGE>(A, lda, t, r, lane, K, xr, acc);
    for (; r < r1; r += NW) wrow_step<NW, CPL, 1, EDGE>(A, lda, t, r, lane, K, xr, acc);

#pragma unroll
    for (int j = 0; j < CPL; ++j) part[w][j * 64 + lane] = acc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < SC; c += NW * 64) {
        double s = part[0][c];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) s += part[ww][c];
        if (c < K) out[band * out_ld + c] = s;
    }
}

// NR rows r .. r + NR - 1 of the band by the whole workgroup; slot: which half of dots this group
// uses (a wave can be at most one group ahead of the slowest one, which still reads the other half).
template <int NW, int CPL, int NR, int RB, bool EDGE>
__device__ __forceinline__ void wgrow_step(const double* __restrict__ a, int64_t lda, double* __restrict__ t,
                                           int64_t r, int w, int lane, int k, const double (&x)[CPL],
                                           double (&acc)[CPL], double (&dots)[2][RB][NW], int slot) {
    double v[NR][CPL];
#pragma unroll
    for (int u = 0; u < NR; ++u) ata_load_row<CPL, EDGE>(a + (r + u) * lda, w * 64 * CPL, lane, k, v[u]);
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const double d = group_sum_dpp<64>(ata_dot<CPL>(v[u], x));
        if (lane == 0) dots[slot][u][w] = d;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        // lane ww fetches wave ww's partial; the sum runs in wave order over scalar reads of them,
        // so the NW partials cost two registers, not 2 * NW, beside the row still held in v
        const double mine = dots[slot][u][lane < NW ? lane : 0];
        double ti = readlane_d(mine, 0);
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) ti += readlane_d(mine, ww);
        if (threadIdx.x == 0) t[r + u] = ti;
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] = __builtin_fma(v[u][j], ti, acc[j]);
    }
}

// EDGE: K < 64 * NW * CPL (a wave whose columns all lie beyond K adds +0.0 and stores nothing).
template <int NW, int CPL, int RB, bool EDGE>
__global__ __launch_bounds__(NW * 64) void ata_wgrow(const double* __restrict__ A, int64_t lda,
                                                      const double* __restrict__ x, double* __restrict__ t,
                                                      double* __restrict__ out, int64_t M, int K, int64_t band_rows,
                                                      int64_t out_ld) {
    __shared__ double dots[2][RB][NW];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t band = blockIdx.x;
    const int64_t r0 = band * band_rows;
    const int64_t r1 = r0 + band_rows < M ? r0 + band_rows : M;
    const int c0 = w * 64 * CPL;  // the wave's first column

    double xr[CPL], acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = c0 + j * 64 + lane;
        xr[j] = c < K ? x[c] : 0.0;
        acc[j] = 0.0;
    }
    int slot = 0;
    int64_t r = r0;  // the trip counts are the same for every wave: each step is one barrier
    for (; r + RB <= r1; r += RB, slot ^= 1)
        wgrow_step<NW, CPL, RB, RB, EDGE>(A, lda, t, r, w, lane, K, xr, acc, dots, slot);
    for (; r < r1; ++r, slot ^= 1) wgrow_step<NW, CPL, 1, RB, EDGE>(A, lda, t, r, w, lane, K, xr, acc, dots, slot);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = c0 + j * 64 + lane;
        if (c < K) out[band * out_ld + c] = acc[j];
    }
}

// ------------------------------------------------------------------ variant table
typedef void (*ata_fn)(const double*, int64_t, const double*, double*, double*, int64_t, int, int64_t, int64_t);

struct AVariant {
    const char* name;
    ata_fn fn;       // nullptr: auto, two_pass; for k == max_k
    ata_fn fn_edge;  // for k < max_k
    int threads;     // workgroup size (NW * 64)
    int64_t max_k;   // widest row the fused form holds in registers
    int64_t fill;    // workgroups that fill the chip: 256 CUs x the workgroups of this size a CU holds
};

#define MVG_WROW(NW, CPL, UNR) ata_wrow<NW, CPL, UNR, false>, ata_wrow<NW, CPL, UNR, true>, NW * 64, 64 * CPL, 512
#define MVG_WGROW(NW, CPL, RB) ata_wgrow<NW, CPL, RB, false>, ata_wgrow<NW, CPL, RB, true>, NW * 64, 64 * NW * CPL, NW == 16 ? 256 : 512
// VGPRs (the k == max_k kernel / the one cut by k), waves per SIMD and LDS per kernel
// (-Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2) beside each entry; none has scratch.
static constexpr AVariant kAVariants[] = {
    {"auto", nullptr, nullptr, 0, 0, 0},
    {"two_pass", nullptr, nullptr, 0, INT64_MAX, 0},  // mvg_gemv into t, then mvg_gemv_t from t
    {"wrow_w8_c4_u8", MVG_WROW(8, 4, 8)},             // 106 / 108 VGPRs, 4 waves, 16 KiB
    {"wrow_w8_c8_u4", MVG_WROW(8, 8, 4)},             // 114 / 120, 4, 32 KiB
    {"wrow_w4_c16_u2", MVG_WROW(4, 16, 2)},           // 142 / 158, 3, 32 KiB
    {"wgrow_w8_c8_r2", MVG_WGROW(8, 8, 2)},           // 78 / 86, 6 / 5, 256 B
    {"wgrow_w8_c16_r1", MVG_WGROW(8, 16, 1)},         // 126 / 126, 4, 128 B
    {"wgrow_w16_c8_r2", MVG_WGROW(16, 8, 2)},         // 78 / 86, 6 / 5, 512 B
    {"wgrow_w16_c16_r1", MVG_WGROW(16, 16, 1)},       // 126 / 126, 4 (one 1024-thread workgroup per CU), 256 B
};
#undef MVG_WROW
#undef MVG_WGROW
constexpr int kNumAVariants = (int)(sizeof(kAVariants) / sizeof(kAVariants[0]));
constexpr int kATwoPass = variant_id(kAVariants, "two_pass");
static_assert(kATwoPass == 1, "two_pass is variant 1 (include/matvec_gpu.h)");

constexpr int kAWide = variant_id(kAVariants, "wgrow_w16_c16_r1");
constexpr int kAMid = variant_id(kAVariants, "wgrow_w16_c8_r2");
constexpr int kANarrow = variant_id(kAVariants, "wrow_w8_c8_u4");
constexpr int kAThin = variant_id(kAVariants, "wrow_w8_c4_u8");
static_assert(kAWide > 0 && kAMid > 0 && kANarrow > 0 && kAThin > 0, "dispatch names a missing variant");

// From the two sweeps kept under profiles/r08/gemv_ata/ (MEASUREMENTS §17; two processes, the
// second with the first six shapes only): a fused form where they show it more than 2 % ahead of two_pass,
// which is a k in the upper half of a variant's bracket (from 64 columns for the narrowest) and at
// least the rows of the swept shape. Ratio to the pair issued by hand, at max_k and at a cut k:
//   8192 < k <= 16384, m >= 16384    wgrow_w16_c16_r1  0.53 (16384^2), 0.62 (16384 x 12288)
//   4096 < k <= 8192,  m >= 65536    wgrow_w16_c8_r2   0.52 (65536 x 8192), 0.63 (65536 x 6144)
//   256 < k <= 512,    m >= 524288   wrow_w8_c8_u4     0.54 (524288 x 512), 0.50 (524288 x 384)
//   64 <= k <= 256,    m >= 4194304  wrow_w8_c4_u8     0.61 (4194304 x 64), 0.43 (4194304 x 192)
// Everything else is two_pass: fused slower by 55 % at 2048 x 16384 (64 bands on 256 CUs), k beyond
// 16384 has no fused form, and every other class (512 < k <= 4096, fewer rows than swept) is not
// tuned.
static int pick_ata_variant(int64_t /*lda*/, int64_t m, int64_t k) {
    if (k > 8192 && k <= 16384 && m >= 16384) return kAWide;
    if (k > 4096 && k <= 8192 && m >= 65536) return kAMid;
    if (k > 256 && k <= 512 && m >= 524288) return kANarrow;
    if (k >= 64 && k <= 256 && m >= 4194304) return kAThin;
    return kATwoPass;
}

// The band cut is ata_row.h's plan_ata, per variant.
static APlan plan_ata(const AVariant& var, int64_t m) { return plan_ata(var.threads, var.fill, m); }

// Argument checks shared by the launch and the plan; *v: the variant that runs (auto resolved).
static int check_ata_shape(int64_t lda, int64_t m, int64_t k, int variant, int* v) {
    if (m < 0 || k < 0) return fail(MVG_E_INVALID, "mvg_gemv_ata: negative size");
    if (variant < 0 || variant >= kNumAVariants) return fail(MVG_E_INVALID, "mvg_gemv_ata: bad variant");
    if (k > 0 && lda < k) return fail(MVG_E_INVALID, "mvg_gemv_ata: lda < k");
    *v = variant == 0 ? pick_ata_variant(lda, m, k) : variant;
    if (k > kAVariants[*v].max_k)
        return fail(MVG_E_INVALID, std::string("mvg_gemv_ata: k beyond the max_k of ") + kAVariants[*v].name);
    if (*v == kATwoPass) {  // the pair's own grid limit (mvg_gemv_t: column strips of one launch)
        int64_t b, n, sc;
        if (mvg_gemv_t_plan(lda, m, k, 0, &b, &n, &sc) != MVG_OK)
            return fail(MVG_E_INVALID, "mvg_gemv_ata: too many column strips for one grid (two_pass)");
    }
    return MVG_OK;
}

static int launch_ata(const AVariant& var, const double* A, int64_t lda, const double* x, double* t, double* w,
                      int64_t m, int64_t k, hipStream_t s) {
    const APlan p = plan_ata(var, m);
    if (int rc = take_pending_error("mvg_gemv_ata"); rc != MVG_OK) return rc;  // before our first HIP call
    double* out = w;
    if (p.bands > 1) {
        int rc = workspace(s, (size_t)(p.bands * k), &out);
        if (rc != MVG_OK) return rc;
    }
    hipLaunchKernelGGL(k == var.max_k ? var.fn : var.fn_edge, dim3((unsigned)p.bands), dim3(var.threads), 0, s, A, lda, x,
                       t, out, m, (int)k, p.band_rows, k);
    MVG_HIP(hipGetLastError());
    if (p.bands > 1) return launch_band_reduce(out, p.bands, w, k, s);
    return MVG_OK;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_gemv_ata_variant_count(void) { return kNumAVariants; }

int mvg_gemv_ata_auto_variant(int64_t lda, int64_t m, int64_t k) { return pick_ata_variant(lda, m, k); }

const char* mvg_gemv_ata_variant_name(int v) {
    if (v < 0 || v >= kNumAVariants) return "invalid";
    return kAVariants[v].name;
}

int mvg_gemv_ata_plan(int64_t lda, int64_t m, int64_t k, int variant, int64_t* band_rows, int64_t* bands,
                      int64_t* max_k) {
    int v = 0;
    if (int rc = check_ata_shape(lda, m, k, variant, &v); rc != MVG_OK) return rc;
    if (!band_rows || !bands || !max_k) return fail(MVG_E_INVALID, "mvg_gemv_ata_plan: null");
    const AVariant& var = kAVariants[v];
    const APlan p = var.fn ? plan_ata(var, m) : APlan{0, 0};
    *band_rows = p.band_rows;
    *bands = p.bands;
    *max_k = var.max_k;
    return MVG_OK;
}

int mvg_gemv_ata_variant(const double* A, int64_t lda, const double* x, double* t, double* w, int64_t m, int64_t k,
                         int variant, void* stream) {
    int v = 0;
    if (int rc = check_ata_shape(lda, m, k, variant, &v); rc != MVG_OK) return rc;
    if (m > 0 && !t) return fail(MVG_E_INVALID, "mvg_gemv_ata: null t");
    if (k > 0 && !w) return fail(MVG_E_INVALID, "mvg_gemv_ata: null w");
    if (m > 0 && k > 0 && (!A || !x)) return fail(MVG_E_INVALID, "mvg_gemv_ata: null A or x");
    if (v == kATwoPass || m == 0 || k == 0) {
        // the composed pair, which is also the empty sums: m == 0 zeroes w, k == 0 zeroes t; each
        // entry point takes a pending error before its own first HIP call
        if (int rc = mvg_gemv(A, lda, x, t, m, k, stream); rc != MVG_OK) return rc;
        return mvg_gemv_t(A, lda, t, w, m, k, stream);
    }
    return launch_ata(kAVariants[v], A, lda, x, t, w, m, k, (hipStream_t)stream);
}

int mvg_gemv_ata(const double* A, int64_t lda, const double* x, double* t, double* w, int64_t m, int64_t k,
                 void* stream) {
    return mvg_gemv_ata_variant(A, lda, x, t, w, m, k, 0, stream);
}

}  // extern "C"
