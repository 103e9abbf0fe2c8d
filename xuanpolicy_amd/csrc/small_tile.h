// The 32 x 32 f32 MFMA tile and the activation helpers of the one-launch small kernels (K30 smallmlp.hip, K34
// smallq.hip): LDS operands with per-operand strides, one wave per tile, on v_mfma_f32_32x32x2_f32.
#pragma once
#include "xpa_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int ACT>
__device__ __forceinline__ float sm_act(float z, float slope) {
    if (ACT == 1) return z > 0.f ? z : z * slope;
    if (ACT == 2) return tanhf(z);
    return z;
}
template <int ACT>
__device__ __forceinline__ float sm_grad(float y, float slope) {   // d act / d z from the output y
    if (ACT == 1) return y > 0.f ? 1.f : slope;
    if (ACT == 2) return 1.f - y * y;
    return 1.f;
}

// One 32 x 32 tile D[m][n] = sum_{k < kred} A(m, k) B(k, n) with A(m, k) = pa[k ak + m am], B(k, n) = pb[k bk + n bn]
// (LDS), rows m >= mvalid / columns n >= nvalid of the operands read as 0.  Lane (i, h) feeds A(i, k + h) and
// B(k + h, i); D element r of lane (i, h) is D[(r & 3) + 8 (r >> 2) + 4 h][i].
__device__ __forceinline__ f32x16 sm_tile(const float *pa, int am, int ak, int mvalid, const float *pb, int bk, int bn,
                                          int nvalid, int kred) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const bool av = i < mvalid, bv = i < nvalid;
    const float *qa = pa + (av ? i : 0) * am + h * ak, *qb = pb + (bv ? i : 0) * bn + h * bk;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // 8 k-steps per group: the 16 operand reads issued before the group's MFMAs (a plain loop ran load, wait,
    // MFMA per k-step: one LDS round trip per MFMA)
    int k = 0;
    for (; k + 16 <= kred; k += 16) {
        float x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = qa[(k + 2 * u) * ak];
            y[u] = qb[(k + 2 * u) * bk];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av ? x[u] : 0.f, bv ? y[u] : 0.f, acc, 0, 0, 0);
    }
    for (; k < kred; k += 2) {
        const float x = qa[k * ak], y = qb[k * bk];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av ? x : 0.f, bv ? y : 0.f, acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ int sm_row(int r) { return (r & 3) + 8 * (r >> 2) + 4 * ((threadIdx.x & 63) >> 5); }

}  // namespace
