// Internal helpers shared by the libmatvec_gpu translation units (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <thread>
#include <vector>

#include "../../include/matvec_gpu.h"

namespace mvg {

// Last error text for mvg_last_error(); thread-local like errno.
void set_error(const std::string& msg);
const std::string& get_error();

int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

// An error that an earlier HIP call on this thread left pending belongs to that call. Every
// public launch entry point (tree, multi-vector, exact, panels, relayout, fill, stream read)
// takes it after its argument checks (pure host logic) and before its first HIP call, and
// reports it as such — the call fails, nothing is launched — so the hipGetLastError after its
// own launch only ever sees that launch's error.
int take_pending_error(const char* where);

#define MVG_HIP(call)                                                     \
    do {                                                                  \
        hipError_t _e = (call);                                           \
        if (_e != hipSuccess) return ::mvg::hip_fail(_e, #call);          \
    } while (0)

// ----- variant tables (gemv.hip, gemv_exact.hip)
// Variants are addressed by name, resolved at compile time: inserting or removing a table
// entry cannot send a shape to the wrong kernel (a missing name fails the build).
constexpr bool name_eq(const char* a, const char* b) {
    while (*a && *a == *b) ++a, ++b;
    return *a == *b;
}
template <typename T, size_t N>
constexpr int variant_id(const T (&table)[N], const char* name) {
    for (size_t i = 0; i < N; ++i)
        if (name_eq(table[i].name, name)) return (int)i;
    return -1;
}

// Short rows (K <= 768) go out in launches of at most 1 GiB of A, for the tree form's one-row
// waves and the exact forms alike (the measurements stand at the two launch loops): 1 GiB of the
// bytes read, k per row — a view's wider lda does not shrink the pieces — and never under 65536
// rows, so a launch still fills the chip; whole workgroups of rows_per_block rows.
constexpr int64_t kOneRowLaunchBytes = 1ll << 30;
constexpr int64_t kMinPieceRows = 65536;
inline int64_t short_row_piece_rows(int64_t k, int rows_per_block) {
    int64_t cap = kOneRowLaunchBytes / (k * (int64_t)sizeof(double));
    if (cap < kMinPieceRows) cap = kMinPieceRows;
    return cap / rows_per_block * rows_per_block;
}

// Rows [0, m) as consecutive ranges of at most max_rows rows, in order (each range is an
// independent GEMV; max_rows: the caller's grid limit, and its short-row cap where it has one).
// piece(r0, rows) launches one range and returns its status — the hipGetLastError after its
// launch — and the first failure ends the walk and is returned.
template <class F>
int for_row_pieces(int64_t m, int64_t max_rows, F&& piece) {
    for (int64_t r0 = 0; r0 < m; r0 += max_rows) {
        const int rc = piece(r0, m - r0 < max_rows ? m - r0 : max_rows);
        if (rc != MVG_OK) return rc;
    }
    return MVG_OK;
}

// ----- the kernels' workspace (gemv.hip): n doubles of device memory that belong to `s` on the
// current device, one buffer per (device, stream) grown on demand; the split-K partials of
// mvg_gemv and the band partials of mvg_gemv_t (gemv_t.hip) and mvg_gemv_ata (gemv_ata.hip) live
// there, each call's use ending with its own last kernel on `s` (stream contract).
int workspace(hipStream_t s, size_t n, double** out);

// ----- the band reduce of the transposed product (gemv_t.hip, gemvt_reduce): y[j] = the sum over
// b < bands of partial[b*k + j], j < k, in one fixed order for a given band count; mvg_gemv_t and
// the fused mvg_gemv_ata (gemv_ata.hip) both end with it when they cut m into more than one band
int launch_band_reduce(const double* partial, int64_t bands, double* y, int64_t k, hipStream_t s);
// the same for a group of g vectors in one launch (gemv_t_multi.hip, gemvtm_reduce): Y[j + v*ldy] =
// the sum over b < bands of partial[v*vs + b*k + j], in launch_band_reduce's order per vector;
// mvg_gemv_t_multi and the fused mvg_gemv_ata_multi (gemv_ata_multi.hip) both end with it
int launch_band_reduce_multi(const double* partial, int64_t vs, int64_t bands, double* Y, int64_t ldy, int64_t k, int g,
                             hipStream_t s);

// ----- exact exchange (gemv_exact.hip): the reference's own combine orders on the root
// MPI_Reduce(SUM) as the reference's MPICH runs it (colwise.c:124): binomial tree or, for long
// buffers, reduce-scatter + gather, by MPICH 3.3.2's own rule (gemv_exact.hip); overwrites parts
int launch_combine_mpich_reduce(double* parts, int P, int64_t n, double* y, hipStream_t s);
// gather_local_results (blockwise.c:150-207): y = ((0 + p[gi*gc]) + p[gi*gc+1]) + ... per grid row
int launch_combine_grid_rows(const double* parts, int gr, int gc, int64_t lr, double* y, hipStream_t s);

// ----- synthetic generator (spec in include/matvec_gpu.h) ---------------------------
constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ULL;

__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t splitmix64(uint64_t x) { return mix64(x + kGamma); }

__host__ __device__ inline uint64_t mulhi_10000(uint64_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(z, 10000ULL);
#else
    return (uint64_t)(((unsigned __int128)z * 10000u) >> 64);
#endif
}

// s0 = splitmix64(seed); value = floor(splitmix64(s0 + idx*gamma) * 1e4 / 2^64) / 1e4
__host__ __device__ inline double synth_value(uint64_t s0, uint64_t idx) {
    const uint64_t z = splitmix64(s0 + idx * kGamma);
    return (double)mulhi_10000(z) / 10000.0;
}

// Host threads the library's CPU work (loader, host generator, first touch) uses: $MVG_THREADS
// if set, else the CPUs this process may actually run on — its affinity mask, capped by its
// cgroup's CPU quota (a job given 16 CPUs of a 256-CPU host sees 256 in hardware_concurrency) —
// at most 64 (host.cpp).
int host_thread_count();

// Static split of [0, n) over host_thread_count() threads. `serial` forces one thread.
template <class F>
void parallel_for(int64_t n, F&& body, bool serial = false) {
    int nt = host_thread_count();
    if (nt > n) nt = (int)(n > 0 ? n : 1);
    if (serial || nt == 1) {
        body((int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) {
        const int64_t b = n * t / nt, e = n * (t + 1) / nt;
        th.emplace_back([&body, b, e] { body(b, e); });
    }
    for (auto& t : th) t.join();
}

}  // namespace mvg
