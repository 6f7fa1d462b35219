// Cross-lane sums of an fp64 value with DPP, shared by the tree kernels (gemv.hip) and the fused
// A^T A kernels (gemv_ata.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace mvg {

// One DPP lane permutation of an fp64 value (two 32-bit v_mov_b32_dpp): a VALU op, no LDS
// round trip, unlike the ds_bpermute_b32 pair __shfl_xor compiles to.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double readlane_d(double v, int lane) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Sum over each group of LPR lanes with DPP: quad xor 1, quad xor 2, row half-mirror (8 lanes),
// row mirror (16 lanes) — after each step every lane of the span holds the same value, since
// fp64 addition is commutative (a + b == b + a bit for bit) — then one xor-16 shuffle for
// 32-lane groups, or the four 16-lane row sums read as scalars for the whole wave.
// Fixed order throughout: deterministic, and the same value in every lane of a group (lane 0
// of the group stores it; for LPR = 64 the result is wave-uniform).
template <int LPR>
__device__ __forceinline__ double group_sum_dpp(double v) {
    static_assert(LPR == 8 || LPR == 16 || LPR == 32 || LPR == 64, "DPP group size");
    v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_d<0x141>(v);  // row_half_mirror
    if constexpr (LPR >= 16) v += dpp_d<0x140>(v);  // row_mirror
    if constexpr (LPR == 32) v += __shfl_xor(v, 16, 64);
    if constexpr (LPR == 64)
        v = (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
    return v;
}

}  // namespace mvg
