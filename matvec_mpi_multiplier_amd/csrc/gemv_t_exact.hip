// Bit-exact fp64 transposed GEMV for gfx950 (MI355X): y = A^T z on the row-major A, with the bits of
// the reference's sequential rounded sum (multiply_std_rowwise, src/matr_utils.c:86-96, on a
// contiguous transposed copy of A):
//
//   y[j]: sum = +0.0; for i = 0 .. m-1: sum = round(sum + round(A[i*lda + j] * z[i]))
//
// a rounded multiply, then a rounded add (no FMA), rows strictly in order. Columns are summed down
// the rows, so the lane that owns a column carries the reference's chain itself: no lane-to-lane
// hop (gemv_exact.hip) and no combine across bands (gemv_t.hip) — a chain cannot be cut into bands,
// so a workgroup owns a strip of SC columns over all m rows and the grid is ceil(k / SC) workgroups.
// Every form below runs the same chain per column, so y is the same bits for every variant, shape,
// lda, alignment and run.
//
// Direct form (gemvt_seq, tseq_c<SC>_u<U>): a lane per column, U rows of 8-B non-temporal loads in
// flight in registers (slot i % U holds row i and is refilled U rows ahead as soon as it has been
// summed), any lda and any 8-B alignment. z is wave-uniform: a wave reads 64 consecutive entries of
// z with one coalesced load (lane l holds z[r0 + l], the next 64 are fetched a block ahead) and row
// r0 + i's value comes out of lane i as a scalar, so no latency of z sits on the chain. In a strip
// cut by k the lanes that own no column read the strip's first column again and store nothing;
// rows past m - 1 are never read.
//
// Staged form (gemvt_seqx, tseqx_w<NW>_c<SC>_t<T>_b<NB>): NW waves fetch tiles of T rows x SC
// columns, and the tile's T entries of z, into a ring of NB LDS buffers with
// `global_load_lds_dwordx4` (LDS-DMA: no registers held while in flight, lds_dma.h), NB - 1 tiles
// in flight behind the one being summed; the first SC lanes of the workgroup are the chain lanes
// and read their column of the tile, row by row, while the next tiles arrive. One s_barrier per
// tile: a wave waits for its own loads of tile t (a counted s_waitcnt), the barrier makes every
// wave's part visible and says that tile t - 1 has been summed, whose buffer tile t + NB - 1 then
// takes. It needs what the DMA needs: A and z 16-B aligned, an even lda, and T rows of lda within
// the 32-bit per-lane byte offset (lda < 2^29 / T). Whole tiles and whole strips only: the last
// m % T rows go through the direct form's loop, and the host sends the k % SC columns of a strip
// cut by k to the direct form (variant 1) in a launch of its own on the same stream, so nothing is
// read outside A[i, 0..k) and z[0..m) and nothing is stored outside y[0..k).
//
// Multi form (gemvt_seq_multi, tseqm_c<SC>_u<U>_v<NV>): the direct form with NV independent chains
// per column over one read of A (row i's NV values of Z come out of NV blocks of Z the same way);
// each chain is the single-vector chain, so column v has the bits of gemvt_seq on z_v.
#include <atomic>

#include "common.h"
#include "lds_dma.h"

// hipcc contracts a*b + c into an FMA by default (-ffp-contract=fast); the reference rounds the
// product first. Off for this whole file (the Makefile also passes -ffp-contract=off for it).
#pragma clang fp contract(off)

namespace mvg {

// The reference's step: a rounded product, then a rounded add (plain operators under the pragma
// above; __dmul_rn/__dadd_rn were fused after inlining, MEASUREMENTS §3).
__device__ __forceinline__ double tx_step(double sum, double a, double z) {
    const double p = a * z;
    return sum + p;
}

// lane l's value of v as a wave-uniform scalar (l uniform)
__device__ __forceinline__ double lane_value(double v, int l) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Rows [rb, M) (rb < M) of NV chains, one column per lane: p = A + the lane's column (a lane that
// owns no column is given the strip's first one: it reads inside A[i, 0..k) and stores nothing),
// zs[n] = vector n. U slots of A in flight; z in blocks of 64 rows.
//   prime : slots 0 .. U-1 take rows rb .. rb+U-1 (row M-1 again past the end);
//   main  : whole blocks of 64 rows while every refill lies inside A, one basic block each: row i
//           is summed out of slot i % U, which is then refilled with row i + U (pn walks down the
//           rows); the next block of z is fetched a block ahead; the scheduling barriers keep the
//           loads in slot order, so the compiler's vmcnt waits retire exactly the slot about to be
//           summed. A wave issues one instruction at a time, so the step is kept to the two lane
//           reads, the product, the add, the pointer and the load;
//   rest  : the final M - r0 < 64 + U rows, the same steps behind wave-uniform tests; no refill
//           past row M-1.
template <int U, int NV>
__device__ __forceinline__ void chain_rows(const double* __restrict__ p, int64_t lda, const double* (&zs)[NV],
                                           int64_t rb, int64_t M, int lane, double (&sum)[NV]) {
    static_assert(64 % U == 0, "a block of 64 rows is whole rounds of the U slots");
    double v[U];
    double zc[NV], zn[NV];
    const int64_t last = M - 1;
    auto zblock = [&](int64_t r0, double (&d)[NV]) {  // lane l: z[r0 + l], the last entry again past the end
        const int64_t r = r0 + lane < last ? r0 + lane : last;
#pragma unroll
        for (int n = 0; n < NV; ++n) d[n] = zs[n][r];
    };
    zblock(rb, zc);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t r = rb + u < last ? rb + u : last;
        v[u] = __builtin_nontemporal_load(p + r * lda);
        __builtin_amdgcn_sched_barrier(0);  // same load order as the loop's refills
    }
    const double* pn = p + (rb + U) * lda;  // the next refill's row (dereferenced only while it is < M)
    int64_t r0 = rb;
    for (; r0 + 64 + U <= M; r0 += 64) {
        zblock(r0 + 64, zn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 64; ++i) {
#pragma unroll
            for (int n = 0; n < NV; ++n) sum[n] = tx_step(sum[n], v[i % U], lane_value(zc[n], i));
            __builtin_amdgcn_sched_barrier(0);
            v[i % U] = __builtin_nontemporal_load(pn);
            pn += lda;
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int n = 0; n < NV; ++n) zc[n] = zn[n];
    }
    for (; r0 < M; r0 += 64) {
        if (r0 > rb) zblock(r0, zc);
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            if (r0 + i < M) {
#pragma unroll
                for (int n = 0; n < NV; ++n) sum[n] = tx_step(sum[n], v[i % U], lane_value(zc[n], i));
                if (r0 + i + U < M) v[i % U] = __builtin_nontemporal_load(pn);
                pn += lda;
            }
        }
    }
}

// ------------------------------------------------------------------ direct form
template <int SC, int U>
__global__ __launch_bounds__(SC < 64 ? 64 : SC) void gemvt_seq(const double* __restrict__ A, int64_t lda,
                                                                const double* __restrict__ z,
                                                                double* __restrict__ y, int64_t M, int64_t K) {
    static_assert(SC == 16 || SC == 32 || SC % 64 == 0, "strip width");
    const int lane = threadIdx.x & 63;
    const int64_t c0 = (int64_t)blockIdx.x * SC;
    const int64_t cols = K - c0 < SC ? K - c0 : SC;
    const bool on = (int)threadIdx.x < cols;
    const double* p = A + c0 + (on ? threadIdx.x : 0);
    const double* zs[1] = {z};
    double sum[1] = {0.0};
    chain_rows<U, 1>(p, lda, zs, 0, M, lane, sum);
    if (on) y[c0 + threadIdx.x] = sum[0];
}

// NV chains per column. Vector n of the group is Z + n*ldz -> Y + n*ldy; with g < NV the chains
// from g on read vector g - 1 again and store nothing.
template <int SC, int U, int NV>
__global__ __launch_bounds__(SC < 64 ? 64 : SC) void gemvt_seq_multi(const double* __restrict__ A, int64_t lda,
                                                                      const double* __restrict__ Z, int64_t ldz,
                                                                      double* __restrict__ Y, int64_t ldy, int64_t M,
                                                                      int64_t K, int g) {
    static_assert(SC == 16 || SC == 32 || SC % 64 == 0, "strip width");
    static_assert(NV >= 2, "one vector: gemvt_seq");
    const int lane = threadIdx.x & 63;
    const int64_t c0 = (int64_t)blockIdx.x * SC;
    const int64_t cols = K - c0 < SC ? K - c0 : SC;
    const bool on = (int)threadIdx.x < cols;
    const double* p = A + c0 + (on ? threadIdx.x : 0);
    const double* zs[NV];
    double sum[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) {
        zs[n] = Z + (int64_t)(n < g ? n : g - 1) * ldz;
        sum[n] = 0.0;
    }
    chain_rows<U, NV>(p, lda, zs, 0, M, lane, sum);
    if (on) {
#pragma unroll
        for (int n = 0; n < NV; ++n)
            if (n < g) Y[(int64_t)n * ldy + c0 + threadIdx.x] = sum[n];
    }
}

// ------------------------------------------------------------------ staged form
constexpr int kTailSlots = 16;  // rows in flight in the staged form's direct loop (its last m % T rows)

template <int NW, int SC, int T, int NB>
__global__ __launch_bounds__(NW * 64) void gemvt_seqx(const double* __restrict__ A, int64_t lda,
                                                       const double* __restrict__ z, double* __restrict__ y,
                                                       int64_t M, int64_t /*K: whole strips only*/) {
    constexpr int kRowBytes = SC * 8;            // LDS row stride: the tile's rows lie back to back
    constexpr int kTileBytes = T * kRowBytes;
    constexpr int kTileInst = kTileBytes / 1024;  // LDS-DMA instructions per tile (1 KiB each)
    constexpr int kI = kTileInst / NW;            // of which each wave issues this many
    constexpr int kBufBytes = kTileBytes + 1024;  // tile + its z segment (lanes past T/2 repeat chunk T/2 - 1)
    static_assert(SC >= 16 && SC % 2 == 0 && SC <= NW * 64, "a chain lane per column, 16-B chunks");
    static_assert(kTileBytes % 1024 == 0 && kTileInst % NW == 0 && kI >= 1, "a tile is whole instructions per wave");
    static_assert(1024 % kRowBytes == 0 || kRowBytes % 1024 == 0, "an instruction covers whole rows or part of one");
    static_assert(T % 2 == 0 && T <= 128, "the z segment is whole 16-B chunks of one instruction");
    static_assert(NB >= 2 && (kI + 1) * (NB - 1) <= 63, "loads in flight must fit the vmcnt counter");
    __shared__ __attribute__((aligned(16))) unsigned char lds[NB * kBufBytes];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t c0 = (int64_t)blockIdx.x * SC;  // a whole strip: the host sends a strip cut by k to gemvt_seq
    const bool on = tid < SC;
    double sum[1] = {0.0};
    const int64_t ntiles = M / T;

    {
        // load side: this wave's instruction j is the tile's instruction w*kI + j; lane l of it
        // moves bytes [q, q + 16) of the tile image, q = inst*1024 + 16*l: row q / kRowBytes, byte
        // q % kRowBytes of the row. Addresses are a wave-uniform base (the tile's first row at the
        // strip's first column) plus a 32-bit per-lane byte offset (the host guarantees that T
        // rows of lda fit 32 bits).
        uint32_t off[kI];
#pragma unroll
        for (int j = 0; j < kI; ++j) {
            const uint32_t q = (uint32_t)((w * kI + j) * 1024 + 16 * lane);
            off[j] = (uint32_t)((int64_t)(q / kRowBytes) * lda * (int64_t)sizeof(double) + q % kRowBytes);
        }
        const uint32_t zoff = (uint32_t)(16 * (lane < T / 2 ? lane : T / 2 - 1));
        const unsigned char* const a0 = reinterpret_cast<const unsigned char*>(A + c0);
        const unsigned char* const z0 = reinterpret_cast<const unsigned char*>(z);
        auto issue = [&](int64_t t, int b) {
            const unsigned char* base = a0 + t * T * lda * (int64_t)sizeof(double);
#pragma unroll
            for (int j = 0; j < kI; ++j)
                __builtin_amdgcn_global_load_lds((gbl_void_t)(base + off[j]),
                                                 (lds_void_t)(lds + b * kBufBytes + (w * kI + j) * 1024), 16, 0,
                                                 2 /* nt */);
            if (w == 0)
                __builtin_amdgcn_global_load_lds((gbl_void_t)(z0 + t * T * (int64_t)sizeof(double) + zoff),
                                                 (lds_void_t)(lds + b * kBufBytes + kTileBytes), 16, 0, 0);
        };
        // compute side: chain lane c reads its column of the tile and the z segment (a broadcast)
        auto consume = [&](int b) {
            const unsigned char* tile = lds + b * kBufBytes;
            const unsigned char* zt = tile + kTileBytes;
            double a[T], zz[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                a[i] = *reinterpret_cast<const double*>(tile + i * kRowBytes + tid * 8);
                zz[i] = *reinterpret_cast<const double*>(zt + i * 8);
            }
#pragma unroll
            for (int i = 0; i < T; ++i) sum[0] = tx_step(sum[0], a[i], zz[i]);
        };

        for (int q = 0; q < NB - 1; ++q)
            if (q < ntiles) issue(q, q);
        for (int64_t t = 0; t < ntiles; ++t) {
            // this wave's loads of tile t are done once only those of the NB - 2 tiles issued
            // after it are outstanding (fewer tiles than that near the end: wait for all)
            if (t + NB - 2 < ntiles) {
                if (w == 0)
                    wait_vmcnt<(NB - 2) * (kI + 1)>();
                else
                    wait_vmcnt<(NB - 2) * kI>();
            } else {
                wait_vmcnt<0>();
            }
            // the chain lanes' reads of tile t - 1 have returned (their values fed the adds)
            wait_lgkmcnt0();
            __builtin_amdgcn_s_barrier();  // tile t is whole in LDS; tile t - 1 has been summed
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            const int64_t tn = t + NB - 1;
            if (tn < ntiles) issue(tn, (int)(tn % NB));
            if (on) consume((int)(t % NB));
        }
    }
    // what the ring did not take: the last M % T rows
    if (ntiles * T < M && w * 64 < SC) {
        const double* zs[1] = {z};
        chain_rows<kTailSlots, 1>(A + c0 + (on ? tid : 0), lda, zs, ntiles * T, M, lane, sum);
    }
    if (on) y[c0 + tid] = sum[0];
}

__global__ void gemvtx_zero(double* y, int64_t k) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = 0.0;
}

// ------------------------------------------------------------------ variant table
typedef void (*tx_fn)(const double*, int64_t, const double*, double*, int64_t, int64_t);

struct TxVariant {
    const char* name;
    tx_fn fn;
    int threads;     // workgroup size
    int strip_cols;  // columns one workgroup covers (SC)
    int tile_rows;   // staged forms: T (lda < 2^29 / T, 16-B aligned A and z, even lda); 0: any operands
};

#define TSEQ(SC, U) {"tseq_c" #SC "_u" #U, gemvt_seq<SC, U>, SC < 64 ? 64 : SC, SC, 0}
#define TSEQX(NW, SC, T, NB) {"tseqx_w" #NW "_c" #SC "_t" #T "_b" #NB, gemvt_seqx<NW, SC, T, NB>, NW * 64, SC, T}
// VGPRs / LDS per kernel (-Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2) beside each
// entry; none with scratch. The direct (and multi) forms with 16- and 32-column strips launch
// 64-lane workgroups in which 48 or 32 lanes own no column (they read the strip's first column
// again and store nothing): sweep candidates for a narrow k, none of them picked.
static constexpr TxVariant kTxVariants[] = {
    {"auto", nullptr, 0, 0, 0},
    TSEQ(64, 16),  // 76 VGPRs; the direct form that defines the result
    TSEQ(64, 32),  // 78
    TSEQ(64, 64),  // 142
    TSEQ(32, 32),  // 78
    TSEQ(16, 32),  // 78
    TSEQ(16, 64),  // 142
    TSEQ(128, 32),  // 80
    TSEQX(4, 64, 32, 3),   // 154 VGPRs, 51 KiB of LDS (NB x (T x SC x 8 + 1024) bytes)
    TSEQX(4, 64, 32, 2),   // 133, 34 KiB
    TSEQX(4, 32, 32, 3),   // 104, 27 KiB
    TSEQX(4, 16, 64, 3),   // 114, 27 KiB
    TSEQX(2, 16, 32, 4),   // 132, 20 KiB
    TSEQX(4, 128, 16, 3),  // 90, 51 KiB
};
#undef TSEQ
#undef TSEQX
constexpr int kNumTxVariants = (int)(sizeof(kTxVariants) / sizeof(kTxVariants[0]));
constexpr int kTxDirect = variant_id(kTxVariants, "tseq_c64_u16");
static_assert(kTxDirect == 1 && kTxVariants[kTxDirect].tile_rows == 0,
              "variant 1 is the direct form that takes any operands (include/matvec_gpu.h)");

// a staged form's operand rules, from the arguments alone
static bool tx_operands_ok(const TxVariant& var, int64_t lda, bool aligned16) {
    if (var.tile_rows == 0) return true;
    return aligned16 && lda % 2 == 0 && lda < (1ll << 29) / var.tile_rows;
}

constexpr int kTxWide = variant_id(kTxVariants, "tseqx_w4_c128_t16_b3");
constexpr int kTxMid = variant_id(kTxVariants, "tseqx_w4_c64_t32_b3");
constexpr int kTxNarrow = variant_id(kTxVariants, "tseqx_w4_c16_t64_b3");
static_assert(kTxWide > 0 && kTxMid > 0 && kTxNarrow > 0, "dispatch names a missing variant");

constexpr int64_t kTxSweptRows = 16384;      // the shortest swept shape
constexpr int64_t kTxSweptCols = 64;         // the narrowest
constexpr int64_t kTxSweptMaxCols = 32768;   // the widest
constexpr int64_t kTxSweptSize = 1ll << 28;  // the smallest: 16384^2, 524288 x 512, 4194304 x 64
constexpr int64_t kTxSweptMaxSize = 1ll << 31;  // the largest: 65536 x 32768
// Test hook (mvg_debug_set_gemv_t_exact_swept, include/matvec_gpu.h): a row count and a size standing
// in for the swept range's lower bounds, so that a small problem takes the picks below.
static std::atomic<int64_t> g_swept_rows{kTxSweptRows}, g_swept_size{kTxSweptSize};
static bool tx_swept(int64_t m, int64_t k) {
    const int64_t size = g_swept_size.load(std::memory_order_relaxed);
    return m >= g_swept_rows.load(std::memory_order_relaxed) && k >= kTxSweptCols && k <= kTxSweptMaxCols &&
           m >= (size + k - 1) / k && m <= kTxSweptMaxSize / k;
}

// From the two sweep runs kept under profiles/r09/gemv_t_exact/ (MEASUREMENTS §19; 16384^2 at lda
// 16384 and 16400, 65536 x 8192, 65536 x 32768, 524288 x 512, 4194304 x 64), the house rule: a
// staged form only for a class in which both runs show it more than 2 % ahead of variant 1. Inside
// the swept range (m >= 16384, 64 <= k <= 32768, 2^28 <= m * k <= 2^31), by the width the shapes
// were swept at (first / second run, the share of variant 1's time):
//   k = 32768        128-column strips, 16-row tiles (65536 x 32768: 0.90 / 0.90; the 64-column
//                    ring is level with variant 1 there, 1.00 / 0.99)
//   8192 < k < 32768  64-column strips, 32-row tiles, three buffers (16384^2: 0.55 / 0.55, at lda
//                    16400 0.52 / 0.52)
//   k <= 8192        16-column strips, 64-row tiles (65536 x 8192: 0.50 / 0.49; 524288 x 512:
//                    0.51 / 0.51; 4194304 x 64: 0.53 / 0.52): narrow strips give a narrow k more
//                    workgroups
// The classes between the swept widths (64 < k < 512, 512 < k < 8192, 8192 < k < 16384,
// 16384 < k < 32768) are extrapolated from their nearest swept neighbour; every candidate is at or
// ahead of variant 1 at both ends of each. Everything else (fewer rows, a wider or narrower k, a
// smaller or larger A) is not tuned: variant 1. A call whose operands break the staged form's
// rules (an odd lda, 8 bytes off a 16-B boundary, lda >= 2^29 / T) takes variant 1 as well: the
// same bits.
static int pick_tx_variant(int64_t m, int64_t k) {
    if (!tx_swept(m, k)) return kTxDirect;
    return k >= 32768 ? kTxWide : k > 8192 ? kTxMid : kTxNarrow;
}

// what auto runs for these operands: the pick, or variant 1 where the operands break its rules
static int resolve_tx_variant(int64_t lda, int64_t m, int64_t k, bool aligned16) {
    const int v = pick_tx_variant(m, k);
    return tx_operands_ok(kTxVariants[v], lda, aligned16) ? v : kTxDirect;
}

static int check_tx_shape(int64_t lda, int64_t m, int64_t k, int variant) {
    if (m < 0 || k < 0) return fail(MVG_E_INVALID, "mvg_gemv_t_exact: negative size");
    if (variant < 0 || variant >= kNumTxVariants) return fail(MVG_E_INVALID, "mvg_gemv_t_exact: bad variant");
    if (k > 0 && lda < k) return fail(MVG_E_INVALID, "mvg_gemv_t_exact: lda < k");
    return MVG_OK;
}

// one grid of ceil(k / SC) workgroups: gridDim.x * blockDim.x < 2^32
static int check_tx_grid(int threads, int strip_cols, int64_t k, const char* who) {
    if ((k + strip_cols - 1) / strip_cols > (1ll << 31) / threads)
        return fail(MVG_E_INVALID, std::string(who) + ": too many column strips for one grid");
    return MVG_OK;
}

// ------------------------------------------------------------------ multi-vector variant table
typedef void (*txm_fn)(const double*, int64_t, const double*, int64_t, double*, int64_t, int64_t, int64_t, int);
struct TxMultiVariant {
    const char* name;
    txm_fn fn;  // nullptr: auto, separate
    int threads;
    int strip_cols;
    int nv;  // chains per column
};
#define TSEQM(SC, U, NV) {"tseqm_c" #SC "_u" #U "_v" #NV, gemvt_seq_multi<SC, U, NV>, SC < 64 ? 64 : SC, SC, NV}
static constexpr TxMultiVariant kTxMultiVariants[] = {
    {"auto", nullptr, 0, 0, 0},
    {"separate", nullptr, 0, 0, 1},  // one mvg_gemv_t_exact per vector
    TSEQM(64, 16, 2),  // 80 VGPRs, no scratch, no LDS
    TSEQM(64, 16, 4),  // 72
    TSEQM(64, 32, 2),  // 88
    TSEQM(16, 32, 2),  // 88
    TSEQM(16, 32, 4),  // 102
};
#undef TSEQM
constexpr int kNumTxMultiVariants = (int)(sizeof(kTxMultiVariants) / sizeof(kTxMultiVariants[0]));
constexpr int kTxmSeparate = variant_id(kTxMultiVariants, "separate");
static_assert(kTxmSeparate == 1, "separate is variant 1 (include/matvec_gpu.h)");

constexpr int kTxm2 = variant_id(kTxMultiVariants, "tseqm_c64_u32_v2");
constexpr int kTxm4 = variant_id(kTxMultiVariants, "tseqm_c64_u16_v4");
static_assert(kTxm2 > 0 && kTxm4 > 0, "multi dispatch names a missing variant");

// The variant for the group that opens a run of `rem` vectors (the same two runs, nv = 2 and 4):
// inside the swept range four chains per column take 0.29-0.38 of four separate passes of
// variant 1 and two chains 0.40-0.46 of two, in every shape of both runs; against separate passes
// of the staged picks above (the second run's `separate`) they take 0.32-0.73 and 0.51-0.89, more
// than 2 % ahead everywhere; a run of 3 goes out as 2 + 1. Outside the swept range: separate, not
// tuned.
static int pick_txm_variant(int64_t m, int64_t k, int rem) {
    if (rem < 2 || !tx_swept(m, k)) return kTxmSeparate;
    return rem >= 4 ? kTxm4 : kTxm2;
}

// The group that opens a run of `rem` vectors: auto asks the dispatch group by group; an explicit
// fused variant takes min(rem, NV) vectors while at least two are left. *v == separate comes with
// *g == 1: one vector through mvg_gemv_t_exact.
static void next_tx_group(int variant, int64_t m, int64_t k, int rem, int* v, int* g) {
    *v = variant == 0 ? pick_txm_variant(m, k, rem) : variant;
    const TxMultiVariant& var = kTxMultiVariants[*v];
    if (!var.fn || rem < 2) {
        *v = kTxmSeparate;
        *g = rem < 1 ? rem : 1;
        return;
    }
    *g = rem < var.nv ? rem : var.nv;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_gemv_t_exact_variant_count(void) { return kNumTxVariants; }

int mvg_gemv_t_exact_auto_variant(int64_t lda, int64_t m, int64_t k) {
    return resolve_tx_variant(lda, m, k, true);
}

int mvg_gemv_t_exact_resolve_variant(const double* A, int64_t lda, const double* z, int64_t m, int64_t k) {
    return resolve_tx_variant(lda, m, k, (uintptr_t)A % 16 == 0 && (uintptr_t)z % 16 == 0);
}

int mvg_debug_set_gemv_t_exact_swept(int64_t min_rows, int64_t min_size) {
    if (min_rows < 0 || min_size < 0) return fail(MVG_E_INVALID, "mvg_debug_set_gemv_t_exact_swept: negative bound");
    g_swept_rows.store(min_rows > 0 ? min_rows : kTxSweptRows, std::memory_order_relaxed);
    g_swept_size.store(min_size > 0 ? min_size : kTxSweptSize, std::memory_order_relaxed);
    return MVG_OK;
}

const char* mvg_gemv_t_exact_variant_name(int v) {
    if (v < 0 || v >= kNumTxVariants) return "invalid";
    return kTxVariants[v].name;
}

int mvg_gemv_t_exact_variant(const double* A, int64_t lda, const double* z, double* y, int64_t m, int64_t k,
                             int variant, void* stream) {
    if (int rc = check_tx_shape(lda, m, k, variant); rc != MVG_OK) return rc;
    if (k == 0) return MVG_OK;
    if (!y) return fail(MVG_E_INVALID, "mvg_gemv_t_exact: null y");
    if (m > 0 && (!A || !z)) return fail(MVG_E_INVALID, "mvg_gemv_t_exact: null A or z");
    const bool aligned16 = (uintptr_t)A % 16 == 0 && (uintptr_t)z % 16 == 0;
    int v = variant;
    if (v == 0) {  // a staged pick whose operand rules this call breaks: the direct form, same bits
        v = resolve_tx_variant(lda, m, k, aligned16);
    } else if (m > 0 && !tx_operands_ok(kTxVariants[v], lda, aligned16)) {
        return fail(MVG_E_INVALID, "mvg_gemv_t_exact: staged variant needs 16-B aligned A and z and an even lda < 2^29 / T");
    }
    const TxVariant& var = kTxVariants[v];
    if (int rc = check_tx_grid(var.threads, var.strip_cols, k, "mvg_gemv_t_exact"); rc != MVG_OK) return rc;
    if (int rc = take_pending_error("mvg_gemv_t_exact"); rc != MVG_OK) return rc;  // before our first HIP call
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {  // the empty sum: +0.0
        hipLaunchKernelGGL(gemvtx_zero, dim3((unsigned)((k + 255) / 256 < 4096 ? (k + 255) / 256 : 4096)), dim3(256), 0,
                           s, y, k);
        MVG_HIP(hipGetLastError());
        return MVG_OK;
    }
    if (var.tile_rows == 0) {
        hipLaunchKernelGGL(var.fn, dim3((unsigned)((k + var.strip_cols - 1) / var.strip_cols)), dim3(var.threads), 0, s,
                           A, lda, z, y, m, k);
        MVG_HIP(hipGetLastError());
        return MVG_OK;
    }
    // staged: the whole strips, then the k % SC columns of the cut strip through the direct form
    const int64_t kw = k / var.strip_cols * var.strip_cols;
    if (kw > 0) {
        hipLaunchKernelGGL(var.fn, dim3((unsigned)(kw / var.strip_cols)), dim3(var.threads), 0, s, A, lda, z, y, m, kw);
        MVG_HIP(hipGetLastError());
    }
    if (kw < k) {
        const TxVariant& dir = kTxVariants[kTxDirect];
        hipLaunchKernelGGL(dir.fn, dim3((unsigned)((k - kw + dir.strip_cols - 1) / dir.strip_cols)), dim3(dir.threads), 0,
                           s, A + kw, lda, z, y + kw, m, k - kw);
        MVG_HIP(hipGetLastError());
    }
    return MVG_OK;
}

int mvg_gemv_t_exact(const double* A, int64_t lda, const double* z, double* y, int64_t m, int64_t k, void* stream) {
    return mvg_gemv_t_exact_variant(A, lda, z, y, m, k, 0, stream);
}

// ---- a block of vectors (gemvt_seq_multi)
int mvg_gemv_t_exact_multi_variant_count(void) { return kNumTxMultiVariants; }

int mvg_gemv_t_exact_multi_auto_variant(int64_t lda, int64_t ldz, int64_t m, int64_t k, int nv) {
    (void)lda, (void)ldz;  // the fused forms take any operands
    return pick_txm_variant(m, k, nv);
}

const char* mvg_gemv_t_exact_multi_variant_name(int v) {
    if (v < 0 || v >= kNumTxMultiVariants) return "invalid";
    return kTxMultiVariants[v].name;
}

int mvg_gemv_t_exact_multi_variant(const double* A, int64_t lda, const double* Z, int64_t ldz, double* Y, int64_t ldy,
                                   int64_t m, int64_t k, int nv, int variant, void* stream) {
    if (m < 0 || k < 0 || nv < 0) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: negative size or nv");
    if (variant < 0 || variant >= kNumTxMultiVariants) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: bad variant");
    if (k > 0 && lda < k) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: lda < k");
    if (k > 0 && nv > 0 && ldz < m) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: ldz < m");
    if (nv > 0 && ldy < k) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: ldy < k");
    if (k == 0 || nv == 0) return MVG_OK;
    if (!Y) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: null Y");
    if (m > 0 && (!A || !Z)) return fail(MVG_E_INVALID, "mvg_gemv_t_exact_multi: null A or Z");
    if (m == 0) variant = kTxmSeparate;  // the empty sum: mvg_gemv_t_exact writes the zeros
    // the grid limits of everything the call launches, group by group, before any of it
    for (int rem = nv; rem > 0;) {
        int v, g;
        next_tx_group(variant, m, k, rem, &v, &g);
        const TxMultiVariant& var = kTxMultiVariants[v];
        const int threads = var.fn ? var.threads : kTxVariants[kTxDirect].threads;
        const int sc = var.fn ? var.strip_cols : kTxVariants[kTxDirect].strip_cols;
        if (int rc = check_tx_grid(threads, sc, k, "mvg_gemv_t_exact_multi"); rc != MVG_OK) return rc;
        rem -= g;
    }
    bool taken = false;
    for (int done = 0; done < nv;) {
        int v, g;
        next_tx_group(variant, m, k, nv - done, &v, &g);
        const double* Zg = Z ? Z + (int64_t)done * ldz : Z;
        double* Yg = Y + (int64_t)done * ldy;
        if (v == kTxmSeparate) {  // mvg_gemv_t_exact takes a pending error before its own first HIP call
            if (int rc = mvg_gemv_t_exact(A, lda, Zg, Yg, m, k, stream); rc != MVG_OK) return rc;
        } else {
            if (!taken)  // before our first HIP call
                if (int rc = take_pending_error("mvg_gemv_t_exact_multi"); rc != MVG_OK) return rc;
            taken = true;
            const TxMultiVariant& var = kTxMultiVariants[v];
            hipLaunchKernelGGL(var.fn, dim3((unsigned)((k + var.strip_cols - 1) / var.strip_cols)), dim3(var.threads), 0,
                               (hipStream_t)stream, A, lda, Zg, ldz, Yg, ldy, m, k, g);
            MVG_HIP(hipGetLastError());
        }
        done += g;
    }
    return MVG_OK;
}

int mvg_gemv_t_exact_multi(const double* A, int64_t lda, const double* Z, int64_t ldz, double* Y, int64_t ldy,
                           int64_t m, int64_t k, int nv, void* stream) {
    return mvg_gemv_t_exact_multi_variant(A, lda, Z, ldz, Y, ldy, m, k, nv, 0, stream);
}

}  // extern "C"
