// The impute pack, built by the two pack kernels of vmp_impute.hip and read by impute_kernel (vmp_impute.hip) and sample_kernel
// (vmp_sample.hip): its geometry and a component's registers.  The two cells (impute_cell, sample_cell) stay in their files.
//
// impute pack:  [ mu_k (D) | Lambda_k lower, row-major packed (D(D+1)/2) | log w | nu | log det Lambda | 1 / nu | G_k[0..D] ]
//   G_k[j] = lgamma((nu + j) / 2) - lgamma(nu / 2) - (j / 2) log(pi nu)        (natural-log units)
#pragma once
#include "vmp_mix_stream.h"

namespace vmp {

template <int D>
struct ImputeGeo {
    static constexpr int TRI  = D * (D + 1) / 2;
    static constexpr int LW   = D + TRI;           // log w
    static constexpr int NU   = LW + 1;
    static constexpr int LDET = LW + 2;
    static constexpr int INU  = LW + 3;
    static constexpr int G    = LW + 4;
    static constexpr int PACK = G + D + 1;
    static constexpr int STRIDE = PACK | 1;        // LDS stride: odd, so that the 16 components of a tile fall into 16 banks
};

inline int impute_pack_words(int D) { return 2 * D + D * (D + 1) / 2 + 5; }

// a component of the pack in registers
template <int D>
struct ImputeParams {
    float mu[D], lam[ImputeGeo<D>::TRI], lw, nu, ldet, inu;     // G[] stays in LDS: it is indexed by the row's D_o
    __device__ __forceinline__ void load(const float* src) {
        using G = ImputeGeo<D>;
#pragma unroll
        for (int d = 0; d < D; ++d) mu[d] = src[d];
#pragma unroll
        for (int i = 0; i < G::TRI; ++i) lam[i] = src[D + i];
        lw = src[G::LW]; nu = src[G::NU]; ldet = src[G::LDET]; inu = src[G::INU];
    }
    __device__ __forceinline__ float L(int i, int j) const { return lam[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i]; }
};

}  // namespace vmp
