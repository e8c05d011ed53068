// Small device helpers shared by the mixture kernels (vmp_mix.hip, vmp_score.hip, vmp_impute.hip, vmp_missfit.hip) and the K-sized
// parameter maps (vmp_prep_parts.h): row loads and stores, a 64-bit lane read, digamma and the register-resident fp64
// factorisations of the K-sized kernels.
#pragma once
#include "vmp_common.h"

namespace vmp {

template <int D>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&o)[D], bool vec) {
    if constexpr (D % 4 == 0) {
        if (vec) {
#pragma unroll
            for (int j = 0; j < D / 4; ++j) {
                float4 v = reinterpret_cast<const float4*>(p)[j];
                o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
            }
            return;
        }
    } else if constexpr (D % 2 == 0) {
        if (vec) {
#pragma unroll
            for (int j = 0; j < D / 2; ++j) {
                float2 v = reinterpret_cast<const float2*>(p)[j];
                o[2 * j] = v.x; o[2 * j + 1] = v.y;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = p[j];
}

template <int D>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&o)[D], bool vec) {
    if constexpr (D % 4 == 0) {
        if (vec) {
#pragma unroll
            for (int j = 0; j < D / 4; ++j) reinterpret_cast<float4*>(p)[j] = make_float4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = o[j];
}

__device__ __forceinline__ double readlane_d(double v, int src_lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, src_lane);
    hi = __builtin_amdgcn_readlane(hi, src_lane);
    return __hiloint2double(hi, lo);
}

// digamma(x), x > 0: the recurrence up to x >= 10, then the asymptotic series
__device__ inline double digamma_d(double x) {
    double r = 0.0;
    while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
    const double f = 1.0 / (x * x);
    return r + log(x) - 0.5 / x
           - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760))))));
}

// Cholesky of SPD A (DxD, row-major) -> lower L (in place, upper zeroed).  Returns false if not SPD.
// Fully unrolled so that the matrix lives in registers (runtime-indexed local arrays would go to scratch).
template <int D>
__device__ __forceinline__ bool chol_lower(double (&A)[D * D]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double s = A[j * D + j];
#pragma unroll
        for (int p = 0; p < j; ++p) s -= A[j * D + p] * A[j * D + p];
        ok = ok && (s > 0.0);
        const double d = sqrt(s);
        const double rd = 1.0 / d;
        A[j * D + j] = d;
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            double t = A[i * D + j];
#pragma unroll
            for (int p = 0; p < j; ++p) t -= A[i * D + p] * A[j * D + p];
            A[i * D + j] = t * rd;
        }
#pragma unroll
        for (int i = 0; i < j; ++i) A[i * D + j] = 0.0;
    }
    return ok;
}

// inverse of lower-triangular L -> Li (lower)
template <int D>
__device__ __forceinline__ void tri_inv_lower(const double (&L)[D * D], double (&Li)[D * D]) {
#pragma unroll
    for (int i = 0; i < D * D; ++i) Li[i] = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        Li[j * D + j] = 1.0 / L[j * D + j];
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            double s = 0.0;
#pragma unroll
            for (int p = j; p < i; ++p) s += L[i * D + p] * Li[p * D + j];
            Li[i * D + j] = -s / L[i * D + i];
        }
    }
}

// S (DxD fp32, symmetrised here) = L L^T:  W = L^-1 (lower), sumlog = sum_i log L_ii; false when S is not SPD
template <int D>
__device__ __forceinline__ bool spd_factor_inverse(const float* S, double (&W)[D * D], double& sumlog) {
    double A[D * D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) A[i * D + j] = 0.5 * ((double)S[i * D + j] + (double)S[j * D + i]);
    const bool ok = chol_lower<D>(A);
    sumlog = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) sumlog += log(A[i * D + i]);
    tri_inv_lower<D>(A, W);
    return ok;
}

// out[i (i + 1) / 2 + j] = scale (S^-1)_ij, j <= i, from W = L^-1 of spd_factor_inverse: (S^-1)_ij = sum_{q >= i} W_qi W_qj;
// quiet NaN in every word when !ok
template <int D>
__device__ __forceinline__ void packed_inverse_from_factor(const double (&W)[D * D], double scale, bool ok, float* out) {
    const float qnan = __builtin_nanf("");
    int idx = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
#pragma unroll
            for (int q = i; q < D; ++q) s += W[q * D + i] * W[q * D + j];
            out[idx++] = ok ? (float)(scale * s) : qnan;
        }
}

}  // namespace vmp
