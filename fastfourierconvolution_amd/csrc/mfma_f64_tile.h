// The fp64 MFMA tile loop shared by metric_kernels.hip and prc_kernels.hip: a workgroup of four waves owns a
// 64 x 64 output tile, each wave 2 x 2 v_mfma_f64_16x16x4_f64 tiles, k staged through LDS in chunks of MT_KC.
//
// Fragment maps (16x16x4): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], one double each;
// C/D register r of lane l is row (l >> 4) + 4 r, column l & 15 -- not the f32 map.
#pragma once
#include <hip/hip_runtime.h>

typedef double doublex4 __attribute__((ext_vector_type(4)));

namespace ffc {

constexpr int MT_KC = 32;        // k per staged chunk

// one staged chunk of MT_KC k on the wave's 2 x 2 tiles; element (i, k) of an operand image is at i * SI + k * SK
template <int SI, int SK>
__device__ __forceinline__ void mma_chunk(const double* As, const double* Bs, int wi, int wj, doublex4 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, e = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < MT_KC; kk += 4) {
        const int k = kk + kq;
        const double a0 = As[(wi + e) * SI + k * SK], a1 = As[(wi + 16 + e) * SI + k * SK];
        const double b0 = Bs[(wj + e) * SI + k * SK], b1 = Bs[(wj + 16 + e) * SI + k * SK];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ void zero_acc(doublex4 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = doublex4{0.0, 0.0, 0.0, 0.0};
}

}  // namespace ffc
