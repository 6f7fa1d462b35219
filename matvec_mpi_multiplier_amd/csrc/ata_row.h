// What the fused A^T A kernels for one vector (gemv_ata.hip) and for a block of vectors
// (gemv_ata_multi.hip) share: a lane's loads of one row, its share of a row's dot product, and the
// host's cut of m rows into bands.
#pragma once
#include "common.h"

namespace mvg {

// One row's CPL values of a lane: row = A[i, 0] (wave-uniform), c0 = the first column of the lane's
// wave, k the row's length. EDGE (k cuts the columns): buffer loads through a descriptor of the
// row's k * 8 bytes, whose range check answers +0.0 for a column beyond k without a memory access;
// the addressing stays one per-lane offset plus immediates, as in the whole-row form.
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));
template <int CPL, bool EDGE>
__device__ __forceinline__ void ata_load_row(const double* __restrict__ row, int c0, int lane, int k, double (&v)[CPL]) {
    if constexpr (EDGE) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(row), 0, k * 8, 0x00020000);
#pragma unroll
        for (int j = 0; j < CPL; ++j)  // aux 2: non-temporal
            v[j] = __builtin_bit_cast(double, (uint2v)__builtin_amdgcn_raw_buffer_load_b64(rs, (c0 + j * 64 + lane) * 8, 0, 2));
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) v[j] = __builtin_nontemporal_load(row + c0 + j * 64 + lane);
    }
}

// the lane's share of one row's dot product: one FMA chain, left to right
template <int CPL>
__device__ __forceinline__ double ata_dot(const double (&v)[CPL], const double (&x)[CPL]) {
    double d = v[0] * x[0];
#pragma unroll
    for (int j = 1; j < CPL; ++j) d = __builtin_fma(v[j], x[j], d);
    return d;
}

constexpr int64_t kAMinBandRows = 32;   // workspace share 2 / band_rows <= 6.25 %
constexpr int64_t kABandRows = 256;     // workspace traffic 16*bands*k <= 0.8 % of 8*m*k
constexpr int64_t kATallRows = 25600;   // from here on bands never get shorter than kABandRows
constexpr int64_t kAMaxBandRows = 2048;
constexpr int64_t kATallBlocks = 4096;  // a taller band must still leave this many workgroups

// How a fused variant (workgroups of `threads`, `fill` of them fill the chip) cuts m rows into
// bands (one workgroup each), from the arguments alone:
//  (a) m < 25600: bands shrink from 256 rows down to 32 until the grid has `fill` workgroups;
//  (b) m >= 25600: 256-row bands, or taller ones (up to 2048 rows) while 4096 workgroups remain;
//  (c) the grid cap (gridDim.x * blockDim.x < 2^32): bands grow until the grid fits.
struct APlan {
    int64_t band_rows, bands;
};
inline APlan plan_ata(int threads, int64_t fill, int64_t m) {
    const int64_t max_blocks = (1ll << 31) / threads;
    auto bands_of = [&](int64_t b) { return (m + b - 1) / b; };
    int64_t b = kABandRows;
    if (m < kATallRows) {
        while (b > kAMinBandRows && bands_of(b) < fill) b /= 2;
    } else {
        while (b < kAMaxBandRows && bands_of(2 * b) >= kATallBlocks) b *= 2;
    }
    if (bands_of(b) > max_blocks) b = ((m + max_blocks - 1) / max_blocks + kAMinBandRows - 1) / kAMinBandRows * kAMinBandRows;
    return {b, bands_of(b)};
}

}  // namespace mvg
