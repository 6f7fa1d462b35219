// fp64 fused normal-equations product for a block of vectors on gfx950 (MI355X): T = A X and
// W = A^T T in one pass over the row-major A per group of vectors (what subspace iteration, block
// Lanczos and randomized range finders form in every step; no counterpart in the reference).
//
//   T[i + v*ldt] = sum_j A[i*lda + j] * X[j + v*ldx]      i < m, v < nv
//   W[j + v*ldw] = sum_i A[i*lda + j] * T[i + v*ldt]      j < k, with the T[i, v] that was stored
//
// The kernels are gemv_ata.hip's two geometries with NV column sets, siblings of them and not
// generalisations: a workgroup owns a band of whole rows; a lane holds NV * CPL entries
// of X and NV * CPL column sums, and the registers of a loaded row serve all NV chains.
//   ata_wrowm   a wave per row, k <= 64*CPL. Per row: NV FMA chains over the lane's columns, NV
//               fixed-order DPP sums (wave_sum.h), lane 0 stores the NV values of T[i, .], then
//               acc[v][j] = fma(row[j], t_v, acc[v][j]). No barrier in the row loop; the NW per-wave
//               sums meet in LDS at the band's end, a few vectors at a time, in wave order.
//   ata_wgrowm  a workgroup per row, k <= 64*NW*CPL. The per-wave partial dots of RB rows and NV
//               vectors go to LDS (dots[2][RB][NV][NW], the halves alternate), meet at one barrier
//               per RB rows, and every wave adds the NW partials of a (row, vector) in wave order.
// A chain's operations are those of the one-vector kernel of the same geometry, each on its own
// vector: a column's bits depend on A, x_v, the variant, m and k alone, never on the other vectors
// or on the column's place in its group. A group shorter than NV runs the same kernel: its spare
// chains hold the group's last vector again and store nothing, so no chain holds anything the
// caller did not pass (0 * NaN is NaN). The workgroup stores its column sums into W (one band) or
// into partial[v][band][j] in the per-(device, stream) workspace, and gemv_t_multi.hip's band reduce
// (launch_band_reduce_multi) adds the bands of all vectors of the group in one launch. Columns beyond k
// contribute +0.0 and are never loaded or stored, rows beyond m are skipped, row and vector offsets
// are 64-bit. No atomics: every sum has one fixed order for a given (variant, m, k).
#include "ata_row.h"
#include "wave_sum.h"

namespace mvg {

// Rows r, r + NW, ... (NR of them) of one wave, into the NV chains; vectors from g on are not stored.
template <int NW, int CPL, int NR, int NV, bool EDGE>
__device__ __forceinline__ void wrowm_step(const double* __restrict__ a, int64_t lda, double* __restrict__ T, int64_t ldt,
                                           int g, int64_t r, int lane, int k, const double (&x)[NV][CPL],
                                           double (&acc)[NV][CPL]) {
    double v[NR][CPL];
#pragma unroll
    for (int u = 0; u < NR; ++u) ata_load_row<CPL, EDGE>(a + (r + (int64_t)u * NW) * lda, 0, lane, k, v[u]);
    // row by row: the NV sums of a row are independent (their DPP steps interleave), and only NV
    // wave-uniform values of T are live at a time
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        double ti[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) ti[c] = group_sum_dpp<64>(ata_dot<CPL>(v[u], x[c]));
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            if (lane == 0 && c < g) T[(int64_t)c * ldt + r + (int64_t)u * NW] = ti[c];
#pragma unroll
            for (int j = 0; j < CPL; ++j) acc[c][j] = __builtin_fma(v[u][j], ti[c], acc[c][j]);
        }
    }
}

// out[v * out_vs + band * out_bs + j]: W itself when there is one band (out_vs = ldw, out_bs = 0),
// else the workspace partial[v][band][j] (out_vs = bands * K, out_bs = K). g <= NV: the vectors of
// this group. EDGE: K < 64 * CPL.
template <int NW, int CPL, int UNR, int NV, bool EDGE>
__global__ __launch_bounds__(NW * 64) void ata_wrowm(const double* __restrict__ A, int64_t lda,
                                                      const double* __restrict__ X, int64_t ldx, double* __restrict__ T,
                                                      int64_t ldt, double* __restrict__ out, int64_t out_vs, int64_t out_bs,
                                                      int64_t M, int K, int64_t band_rows, int g) {
    constexpr int SC = 64 * CPL;
    constexpr int VFIT = 32768 / (NW * SC * 8);  // vectors per LDS round: 32 KiB of LDS
    constexpr int VC = VFIT < 1 ? 1 : (VFIT < NV ? VFIT : NV);
    static_assert(NV % VC == 0, "the LDS rounds are whole");
    __shared__ double part[NW][VC][SC];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: rows stay scalar
    const int64_t band = blockIdx.x;
    const int64_t r0 = band * band_rows;
    const int64_t r1 = r0 + band_rows < M ? r0 + band_rows : M;

    double xr[NV][CPL], acc[NV][CPL];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const double* __restrict__ x = X + (int64_t)(c < g ? c : g - 1) * ldx;  // a spare chain: the last vector again
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int col = j * 64 + lane;
            xr[c][j] = col < K ? x[col] : 0.0;
            acc[c][j] = 0.0;
        }
    }
    // wave w's rows r0 + w, r0 + w + NW, ... < r1, in that order, UNR at a time
    int64_t r = r0 + w;
    for (; r + (int64_t)(UNR - 1) * NW < r1; r += (int64_t)UNR * NW)
        wrowm_step<NW, CPL, UNR, NV, EDGE>(A, lda, T, ldt, g, r, lane, K, xr, acc);
    for (; r < r1; r += NW) wrowm_step<NW, CPL, 1, NV, EDGE>(A, lda, T, ldt, g, r, lane, K, xr, acc);

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
            if (vb + c < g && col < K) out[(int64_t)(vb + c) * out_vs + band * out_bs + col] = s;
        }
    }
}

// NR rows r .. r + NR - 1 of the band by the whole workgroup; slot: which half of dots this group
// uses (a wave can be at most one group ahead of the slowest one, which still reads the other half).
template <int NW, int CPL, int NR, int RB, int NV, bool EDGE>
__device__ __forceinline__ void wgrowm_step(const double* __restrict__ a, int64_t lda, double* __restrict__ T, int64_t ldt,
                                            int g, int64_t r, int w, int lane, int k, const double (&x)[NV][CPL],
                                            double (&acc)[NV][CPL], double (&dots)[2][RB][NV][NW], int slot) {
    double v[NR][CPL];
#pragma unroll
    for (int u = 0; u < NR; ++u) ata_load_row<CPL, EDGE>(a + (r + u) * lda, w * 64 * CPL, lane, k, v[u]);
#pragma unroll
    for (int u = 0; u < NR; ++u)
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const double d = group_sum_dpp<64>(ata_dot<CPL>(v[u], x[c]));
            if (lane == 0) dots[slot][u][c][w] = d;
        }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NR; ++u)
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            // lane ww fetches wave ww's partial; the sum runs in wave order over scalar reads of them
            const double mine = dots[slot][u][c][lane < NW ? lane : 0];
            double ti = readlane_d(mine, 0);
#pragma unroll
            for (int ww = 1; ww < NW; ++ww) ti += readlane_d(mine, ww);
            if (threadIdx.x == 0 && c < g) T[(int64_t)c * ldt + r + u] = ti;
#pragma unroll
            for (int j = 0; j < CPL; ++j) acc[c][j] = __builtin_fma(v[u][j], ti, acc[c][j]);
        }
}

// EDGE: K < 64 * NW * CPL (a wave whose columns all lie beyond K adds +0.0 and stores nothing).
template <int NW, int CPL, int RB, int NV, bool EDGE>
__global__ __launch_bounds__(NW * 64) void ata_wgrowm(const double* __restrict__ A, int64_t lda,
                                                       const double* __restrict__ X, int64_t ldx, double* __restrict__ T,
                                                       int64_t ldt, double* __restrict__ out, int64_t out_vs, int64_t out_bs,
                                                       int64_t M, int K, int64_t band_rows, int g) {
    __shared__ double dots[2][RB][NV][NW];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t band = blockIdx.x;
    const int64_t r0 = band * band_rows;
    const int64_t r1 = r0 + band_rows < M ? r0 + band_rows : M;
    const int c0 = w * 64 * CPL;  // the wave's first column

    double xr[NV][CPL], acc[NV][CPL];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const double* __restrict__ x = X + (int64_t)(c < g ? c : g - 1) * ldx;  // a spare chain: the last vector again
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int col = c0 + j * 64 + lane;
            xr[c][j] = col < K ? x[col] : 0.0;
            acc[c][j] = 0.0;
        }
    }
    int slot = 0;
    int64_t r = r0;  // the trip counts are the same for every wave: each step is one barrier
    for (; r + RB <= r1; r += RB, slot ^= 1)
        wgrowm_step<NW, CPL, RB, RB, NV, EDGE>(A, lda, T, ldt, g, r, w, lane, K, xr, acc, dots, slot);
    for (; r < r1; ++r, slot ^= 1) wgrowm_step<NW, CPL, 1, RB, NV, EDGE>(A, lda, T, ldt, g, r, w, lane, K, xr, acc, dots, slot);
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int col = c0 + j * 64 + lane;
            if (c < g && col < K) out[(int64_t)c * out_vs + band * out_bs + col] = acc[c][j];
        }
}

// ------------------------------------------------------------------ variant table
typedef void (*atam_fn)(const double*, int64_t, const double*, int64_t, double*, int64_t, double*, int64_t, int64_t, int64_t,
                        int, int64_t, int);

struct AMVariant {
    const char* name;
    atam_fn fn;       // nullptr: auto, two_pass; for k == max_k
    atam_fn fn_edge;  // for k < max_k
    int threads;      // workgroup size (NW * 64)
    int64_t max_k;    // widest row the fused form holds in registers
    int64_t fill;     // workgroups that fill the chip
    int nv;           // chains: vectors per pass over A
};

#define MVG_WROWM(NW, CPL, UNR, NV) \
    ata_wrowm<NW, CPL, UNR, NV, false>, ata_wrowm<NW, CPL, UNR, NV, true>, NW * 64, 64 * CPL, 512, NV
#define MVG_WGROWM(NW, CPL, RB, NV) \
    ata_wgrowm<NW, CPL, RB, NV, false>, ata_wgrowm<NW, CPL, RB, NV, true>, NW * 64, 64 * NW * CPL, NW == 16 ? 256 : 512, NV
// A lane holds 2 * CPL * (2 * NV + rows in flight) VGPRs of operands, and a 1024-thread workgroup
// has 128 per lane: that bounds the table (k > 8192 has no fused block form). VGPRs (the k == max_k
// kernel / the one cut by k), waves per SIMD and LDS per kernel (-Rpass-analysis=kernel-resource-usage,
// gfx950, ROCm 7.2) beside each entry; none has scratch.
static constexpr AMVariant kAMVariants[] = {
    {"auto", nullptr, nullptr, 0, 0, 0, 0},
    {"two_pass", nullptr, nullptr, 0, INT64_MAX, 0, 0},  // mvg_gemv_multi into T, then mvg_gemv_t_multi from T
    {"wrowm_w8_c4_u4_v2", MVG_WROWM(8, 4, 4, 2)},         // 90 / 92 VGPRs, 5 waves, 32 KiB
    {"wrowm_w8_c4_u4_v4", MVG_WROWM(8, 4, 4, 4)},         // 136 / 138, 3, 32 KiB
    {"wrowm_w8_c8_u2_v2", MVG_WROWM(8, 8, 2, 2)},         // 112 / 120, 4, 32 KiB
    {"wrowm_w8_c8_u2_v4", MVG_WROWM(8, 8, 2, 4)},         // 184 / 192, 2 (one workgroup per CU), 32 KiB
    {"wgrowm_w16_c4_r2_v2", MVG_WGROWM(16, 4, 2, 2)},     // 68 / 70, 7 (one 1024-thread workgroup per CU), 1 KiB
    {"wgrowm_w16_c4_r2_v4", MVG_WGROWM(16, 4, 2, 4)},     // 106 / 110, 4, 2 KiB
    {"wgrowm_w16_c8_r1_v2", MVG_WGROWM(16, 8, 1, 2)},     // 96 / 94, 5, 512 B
};
#undef MVG_WROWM
#undef MVG_WGROWM
constexpr int kNumAMVariants = (int)(sizeof(kAMVariants) / sizeof(kAMVariants[0]));
constexpr int kAMTwoPass = variant_id(kAMVariants, "two_pass");
static_assert(kAMTwoPass == 1, "two_pass is variant 1 (include/matvec_gpu.h)");

// The form for the group that opens a run of `rem` vectors: one with at most rem chains, or
// two_pass. The house rule: a fused form enters here only for a class of shapes where two kept
// sweep runs (tools/gemv_ata_multi_sweep.py) both show it more than 2 % ahead of two_pass. No sweep
// has been run yet, so nothing is tuned: two_pass everywhere.
static int pick_atam_variant(int64_t /*lda*/, int64_t /*ldx*/, int64_t /*m*/, int64_t /*k*/, int /*rem*/) {
    return kAMTwoPass;
}

// The group that opens a run of `rem` vectors, and what runs it. *v is a fused variant with
// *g = min(rem, NV) vectors (auto only names one with NV <= rem, so its groups are full);
// kAMTwoPass with *g = rem (the pair takes every vector that is left at once); or kAMSingle with
// *g = 1: one vector through mvg_gemv_ata, which is a fused variant's single leftover vector and
// auto's last vector.
constexpr int kAMSingle = -1;
static void next_am_group(int variant, int64_t lda, int64_t ldx, int64_t m, int64_t k, int rem, int* v, int* g) {
    *v = variant == 0 ? pick_atam_variant(lda, ldx, m, k, rem) : variant;
    *g = rem;
    if (rem < 1) return;
    if (rem == 1 && variant != kAMTwoPass) {
        *v = kAMSingle;
        return;
    }
    if (*v != kAMTwoPass) *g = rem < kAMVariants[*v].nv ? rem : kAMVariants[*v].nv;
}

// Argument checks shared by the launch and the plan (ldx, ldt, ldw: the launch passes its own, the
// plan the smallest that are allowed).
static int check_atam_shape(int64_t lda, int64_t ldx, int64_t ldt, int64_t ldw, int64_t m, int64_t k, int nv, int variant) {
    if (m < 0 || k < 0 || nv < 0) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: negative size or nv");
    if (variant < 0 || variant >= kNumAMVariants) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: bad variant");
    if (k > 0 && lda < k) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: lda < k");
    if (nv > 0 && ldx < k) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: ldx < k");
    if (nv > 0 && ldt < m) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: ldt < m");
    if (nv > 0 && ldw < k) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: ldw < k");
    if (k > kAMVariants[variant].max_k && variant != 0)
        return fail(MVG_E_INVALID, std::string("mvg_gemv_ata_multi: k beyond the max_k of ") + kAMVariants[variant].name);
    return MVG_OK;
}

// The grid limits of everything a call launches, group by group. A fused group's grid always fits
// (plan_ata grows the bands); the pair and the single vector have the column-strip limits of
// mvg_gemv_t_multi and mvg_gemv_ata.
static int check_atam_grids(int variant, int64_t lda, int64_t ldx, int64_t m, int64_t k, int nv) {
    int64_t b, n, x;
    int grp;
    for (int rem = nv; rem > 0;) {
        int v, g;
        next_am_group(variant, lda, ldx, m, k, rem, &v, &g);
        if (v == kAMTwoPass && mvg_gemv_t_multi_plan(lda, m, k, g, 0, &b, &n, &x, &grp) != MVG_OK)
            return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: too many column strips for one grid (two_pass)");
        if (v == kAMSingle && mvg_gemv_ata_plan(lda, m, k, 0, &b, &n, &x) != MVG_OK)
            return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: too many column strips for one grid (mvg_gemv_ata)");
        rem -= g;
    }
    return MVG_OK;
}

// one group of g <= var.nv vectors (m, k > 0)
static int launch_atam(const AMVariant& var, const double* A, int64_t lda, const double* X, int64_t ldx, double* T,
                       int64_t ldt, double* W, int64_t ldw, int64_t m, int64_t k, int g, hipStream_t s) {
    const APlan p = plan_ata(var.threads, var.fill, m);
    double* out = W;
    int64_t out_vs = ldw, out_bs = 0;
    if (p.bands > 1) {
        int rc = workspace(s, (size_t)(p.bands * k * g), &out);
        if (rc != MVG_OK) return rc;
        out_vs = p.bands * k;
        out_bs = k;
    }
    hipLaunchKernelGGL(k == var.max_k ? var.fn : var.fn_edge, dim3((unsigned)p.bands), dim3(var.threads), 0, s, A, lda, X,
                       ldx, T, ldt, out, out_vs, out_bs, m, (int)k, p.band_rows, g);
    MVG_HIP(hipGetLastError());
    if (p.bands > 1) return launch_band_reduce_multi(out, out_vs, p.bands, W, ldw, k, g, s);
    return MVG_OK;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_gemv_ata_multi_variant_count(void) { return kNumAMVariants; }

int mvg_gemv_ata_multi_auto_variant(int64_t lda, int64_t ldx, int64_t m, int64_t k, int nv) {
    return pick_atam_variant(lda, ldx, m, k, nv);
}

const char* mvg_gemv_ata_multi_variant_name(int v) {
    if (v < 0 || v >= kNumAMVariants) return "invalid";
    return kAMVariants[v].name;
}

int mvg_gemv_ata_multi_plan(int64_t lda, int64_t m, int64_t k, int nv, int variant, int64_t* band_rows, int64_t* bands,
                            int64_t* max_k, int* group) {
    if (int rc = check_atam_shape(lda, k, m, k, m, k, nv, variant); rc != MVG_OK) return rc;
    if (!band_rows || !bands || !max_k || !group) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi_plan: null");
    if (int rc = check_atam_grids(variant, lda, k, m, k, nv); rc != MVG_OK) return rc;
    int v;
    next_am_group(variant, lda, k, m, k, nv, &v, group);
    if (v == kAMSingle) return mvg_gemv_ata_plan(lda, m, k, 0, band_rows, bands, max_k);  // mvg_gemv_ata's own cut
    const AMVariant& var = kAMVariants[v];
    const APlan p = var.fn ? plan_ata(var.threads, var.fill, m) : APlan{0, 0};
    *band_rows = p.band_rows;
    *bands = p.bands;
    *max_k = var.max_k;
    return MVG_OK;
}

int mvg_gemv_ata_multi_variant(const double* A, int64_t lda, const double* X, int64_t ldx, double* T, int64_t ldt, double* W,
                               int64_t ldw, int64_t m, int64_t k, int nv, int variant, void* stream) {
    if (int rc = check_atam_shape(lda, ldx, ldt, ldw, m, k, nv, variant); rc != MVG_OK) return rc;
    if (nv == 0 || (m == 0 && k == 0)) return MVG_OK;
    if (m > 0 && !T) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: null T");
    if (k > 0 && !W) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: null W");
    if (m > 0 && k > 0 && (!A || !X)) return fail(MVG_E_INVALID, "mvg_gemv_ata_multi: null A or X");
    if (m == 0 || k == 0) variant = kAMTwoPass;  // the empty sums: the pair writes the zeros
    if (int rc = check_atam_grids(variant, lda, ldx, m, k, nv); rc != MVG_OK) return rc;
    bool taken = false;
    for (int done = 0; done < nv;) {
        int v, g;
        next_am_group(variant, lda, ldx, m, k, nv - done, &v, &g);
        const double* Xg = X ? X + (int64_t)done * ldx : X;
        double* Tg = T ? T + (int64_t)done * ldt : T;
        double* Wg = W ? W + (int64_t)done * ldw : W;
        if (v == kAMTwoPass) {  // each entry point takes a pending error before its own first HIP call
            if (int rc = mvg_gemv_multi(A, lda, Xg, ldx, Tg, ldt, m, k, g, stream); rc != MVG_OK) return rc;
            if (int rc = mvg_gemv_t_multi(A, lda, Tg, ldt, Wg, ldw, m, k, g, stream); rc != MVG_OK) return rc;
        } else if (v == kAMSingle) {
            if (int rc = mvg_gemv_ata(A, lda, Xg, Tg, Wg, m, k, stream); rc != MVG_OK) return rc;
        } else {
            if (!taken)  // before our first HIP call
                if (int rc = take_pending_error("mvg_gemv_ata_multi"); rc != MVG_OK) return rc;
            taken = true;
            if (int rc = launch_atam(kAMVariants[v], A, lda, Xg, ldx, Tg, ldt, Wg, ldw, m, k, g, (hipStream_t)stream);
                rc != MVG_OK)
                return rc;
        }
        done += g;
    }
    return MVG_OK;
}

int mvg_gemv_ata_multi(const double* A, int64_t lda, const double* X, int64_t ldx, double* T, int64_t ldt, double* W,
                       int64_t ldw, int64_t m, int64_t k, int nv, void* stream) {
    return mvg_gemv_ata_multi_variant(A, lda, X, ldx, T, ldt, W, ldw, m, k, nv, 0, stream);
}

}  // extern "C"
