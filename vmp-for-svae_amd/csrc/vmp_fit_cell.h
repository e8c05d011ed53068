// What the streaming kernels on the fit pack share (vmp_missfit.hip: the fit on partly observed rows, vmp_wfit.hip: the fit on
// weighted rows, vmp_bound.hip: the data term of the lower bound): the pack's geometry and a component's registers, the (row,
// component) cell of a complete and of a partly observed row, the moment accumulation of either, the flush of a wave's fp32 moments
// to its fp64 words, the row load, the fixed-order reduction with its un-shift, the block geometry of the two fits and their
// iteration on the host.  Each of the three files states its own feature's mathematics and lane map and holds its own kernels; every
// kernel is its own instantiation of the text below, which is forced inline.  vmp_bound.hip takes the geometry and the registers only:
// its two cells are the log rho part of the cells here and stay written out in that file (its comment says why).
//
// fit pack, built by fit_pack_kernel (vmp_missfit.hip): [ m_k (D) | Lbar_k = v_k C_k^-1 lower, row-major packed (D(D+1)/2) | c_k ]
#pragma once
#include "vmp_mix_stream.h"

namespace vmp {

template <int D>
struct FitGeo {
    static constexpr int TRI  = D * (D + 1) / 2;
    static constexpr int C    = D + TRI;
    static constexpr int PACK = C + 1;
    static constexpr int STRIDE = PACK | 1;        // LDS stride: odd, so that the 16 components of a tile fall into 16 banks
    static constexpr int MW   = 1 + D + TRI;       // moment words per component: Nk | s1 (D) | s2 lower packed
    static constexpr int SW   = 2 + D + D * D;     // public stats words
};

inline int fit_pack_words(int D) { return D + D * (D + 1) / 2 + 1; }
inline int fit_moment_words(int D) { return 1 + D + D * (D + 1) / 2; }

// block geometry of the two fits (fit_kernel, wfit_pass_kernel and their reductions); vmp_bound.hip keeps no moments and has its own.
// FIT_CHUNK is the cadence of the tiled pass_kernel of vmp_mix.hip (VMP_MOM_FLUSH = 2 tiles of 64 rows; the XDL pass of that file
// flushes every VMP_XDL_MOM_FLUSH = 16th tile).
constexpr int FIT_NW = 4;                 // waves per block
constexpr int FIT_MAX_BLOCKS = 512;
constexpr int FIT_CHUNK = 128;            // rows of a wave between two fp32 -> fp64 flushes
constexpr int FIT_RED_GROUPS = 16;        // wave groups of the reduction block

inline int fit_blocks(int64_t N) { return stream_blocks(N, (int64_t)FIT_NW * FIT_CHUNK, FIT_MAX_BLOCKS); }
// the fp64 moments of every wave
inline size_t fit_slab_bytes(int64_t N, int D, int K) { return (size_t)fit_blocks(N) * FIT_NW * K * fit_moment_words(D) * sizeof(double); }

// a component of the pack in registers
template <int D>
struct FitParams {
    float mu[D], lam[FitGeo<D>::TRI], c;
    __device__ __forceinline__ void load(const float* src) {
        using G = FitGeo<D>;
#pragma unroll
        for (int d = 0; d < D; ++d) mu[d] = src[d];
#pragma unroll
        for (int i = 0; i < G::TRI; ++i) lam[i] = src[D + i];
        c = src[G::C];
    }
    __device__ __forceinline__ float L(int i, int j) const { return lam[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i]; }
};

// x and, under a mask, which of its entries are missing; returns the number of observed entries.  `a` is the kernel's own argument
// struct (x, mask, vec_in), taken by reference as fit_unshift_reduce takes its: with the fields passed as values the compiler
// schedules every fit kernel differently (profiles/NOTES_mix_fit_shared.md).
template <int D, bool MASKED, class Args>
__device__ __forceinline__ int fit_load_row(const Args& a, long long nr, float (&xr)[D], bool (&miss)[D]) {
    load_row<D>(a.x + nr * D, xr, a.vec_in != 0);
    int n_obs = D;
    if constexpr (MASKED) {
        n_obs = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) { miss[d] = a.mask[nr * D + d] != 0; n_obs += miss[d] ? 0 : 1; }
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) miss[d] = false;
    }
    return n_obs;
}

// complete row: d = x - m_k and log rho = c - 1/2 d^T Lbar d, the quadratic form over the lower triangle (the diagonal halved, the
// rest counted once)
template <int D>
__device__ __forceinline__ float fit_cell_full(const FitParams<D>& p, const float (&x)[D], float (&d)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) d[i] = x[i] - p.mu[i];
    float h = 0.f;                               // 1/2 d^T Lbar d
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float s = 0.5f * p.lam[i * (i + 1) / 2 + i] * d[i];
#pragma unroll
        for (int j = 0; j < i; ++j) s = fmaf(p.lam[i * (i + 1) / 2 + j], d[j], s);
        h = fmaf(d[i], s, h);
    }
    h = h < 0.f ? 0.f : h;                       // rounding of an indefinite-looking sum; a NaN stays a NaN
    return p.c - h;
}

// acc += r [ 1 | d | d d^T ]
template <int D>
__device__ __forceinline__ void fit_moments_full(const float (&d)[D], float r, float (&acc)[FitGeo<D>::MW]) {
    acc[0] += r;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float rd = r * d[i];
        acc[1 + i] += rd;
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[1 + D + i * (i + 1) / 2 + j] = fmaf(rd, d[j], acc[1 + D + i * (i + 1) / 2 + j]);
    }
}

// partly observed row (the header of vmp_missfit.hip): log rho; dh[] = xhat - m_k (x_o - m_k,o in the observed slots, -R^-T y in the
// missing ones); A[] the off-diagonal entries of the Cholesky factor of A~ = M Lbar M + (I - M) and rd[] its reciprocal diagonal, for
// fit_moments.
template <int D>
__device__ __forceinline__ float fit_cell(const FitParams<D>& p, const float (&x)[D], const bool (&miss)[D], float (&dh)[D],
                                          float (&A)[FitGeo<D>::TRI], float (&rd)[D]) {
    float dt[D], v[D];
#pragma unroll
    for (int d = 0; d < D; ++d) dt[d] = miss[d] ? 0.f : x[d] - p.mu[d];
    float qo = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float s = p.L(i, 0) * dt[0];
#pragma unroll
        for (int j = 1; j < D; ++j) s = fmaf(p.L(i, j), dt[j], s);
        v[i] = miss[i] ? s : 0.f;
        qo = fmaf(dt[i], s, qo);                 // dt[i] = 0 in the missing rows
    }
    float piv[D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = (miss[i] && miss[j]) ? p.lam[i * (i + 1) / 2 + j] : (i == j ? 1.f : 0.f);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        float s = A[j * (j + 1) / 2 + j];
#pragma unroll
        for (int q = 0; q < j; ++q) s = fmaf(-A[j * (j + 1) / 2 + q], A[j * (j + 1) / 2 + q], s);
        piv[j] = s;
        rd[j] = __builtin_amdgcn_rsqf(s);
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            float t = A[i * (i + 1) / 2 + j];
#pragma unroll
            for (int q = 0; q < j; ++q) t = fmaf(-A[i * (i + 1) / 2 + q], A[j * (j + 1) / 2 + q], t);
            A[i * (i + 1) / 2 + j] = t * rd[j];
        }
    }
    float slog = 0.f;                            // sum_i log R_ii = 1/2 sum log pivot, two pivots per logarithm
#pragma unroll
    for (int j = 0; j + 1 < D; j += 2) slog += logf(piv[j] * piv[j + 1]);
    if constexpr (D % 2) slog += logf(piv[D - 1]);
    slog *= 0.5f;
    float yy = 0.f;                              // y = R^-1 t (in v), |y|^2, z = R^-T y (in v)
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float s = v[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s = fmaf(-A[i * (i + 1) / 2 + q], v[q], s);
        v[i] = s * rd[i];
        yy = fmaf(v[i], v[i], yy);
    }
#pragma unroll
    for (int i = D - 1; i >= 0; --i) {
        float s = v[i];
#pragma unroll
        for (int q = i + 1; q < D; ++q) s = fmaf(-A[q * (q + 1) / 2 + i], v[q], s);
        v[i] = s * rd[i];
    }
#pragma unroll
    for (int d = 0; d < D; ++d) dh[d] = dt[d] - v[d];        // one of the two is an exact zero
    float q = qo - yy;
    q = q < 0.f ? 0.f : q;                       // rounding of the difference; a NaN stays a NaN
    return (p.c - slog) - 0.5f * q;
}

// acc += r [ 1 | dh | dh dh^T + Cov ]:  W = R^-1 in place of the factor (column by column: an entry of R is last read when its own
// slot is written), Cov = W^T W with the observed diagonal (exactly 1) dropped.
template <int D>
__device__ __forceinline__ void fit_moments(const float (&dh)[D], const bool (&miss)[D], float (&A)[FitGeo<D>::TRI], const float (&rd)[D],
                                            float r, float (&acc)[FitGeo<D>::MW]) {
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            float s = A[i * (i + 1) / 2 + j] * rd[j];
#pragma unroll
            for (int q = j + 1; q < i; ++q) s = fmaf(A[i * (i + 1) / 2 + q], A[q * (q + 1) / 2 + j], s);
            A[i * (i + 1) / 2 + j] = -s * rd[i];
        }
    acc[0] += r;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[1 + d] = fmaf(r, dh[d], acc[1 + d]);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float cv = (i == j ? rd[i] : A[i * (i + 1) / 2 + j]) * rd[i];                 // q = i: W_ii W_ij
#pragma unroll
            for (int q = i + 1; q < D; ++q) cv = fmaf(A[q * (q + 1) / 2 + i], A[q * (q + 1) / 2 + j], cv);
            if (i == j) cv = miss[i] ? cv : 0.f;
            acc[1 + D + i * (i + 1) / 2 + j] = fmaf(r, fmaf(dh[i], dh[j], cv), acc[1 + D + i * (i + 1) / 2 + j]);
        }
}

// the four lanes that own component k add their sums; lane kk = 0 adds the result to the wave's fp64 words (first: replaces them)
template <int D>
__device__ __forceinline__ void fit_flush(float (&acc)[FitGeo<D>::MW], double* __restrict__ dst, bool first, bool owner) {
#pragma unroll
    for (int i = 0; i < FitGeo<D>::MW; ++i) {
        const float s = rows4_sum(acc[i]);
        if (owner) dst[i] = (first ? 0.0 : dst[i]) + (double)s;
        acc[i] = 0.f;
    }
}

// The body of a reduction kernel of FIT_RED_GROUPS waves, one block per component: wave group j adds waves j, j + 16, ... of the slab
// in that order, the 16 group sums are added in group order, then the shift by m_k (the fp32 words of the pack, exact in fp64) is
// undone:
//   sx = s1 + Nk m,   sxx = s2 + s1 m^T + m s1^T + Nk m m^T;   word 1 = word 0 (Nk).
// The kernel itself stays in each fit's file under its own name (fit_reduce_kernel, wfit_unshift_kernel), as with block_sum; `a` is
// its argument struct (slab, pack, stats, nwaves, K).
template <int D, class Args>
__device__ __forceinline__ void fit_unshift_reduce(const Args& a) {
    using G = FitGeo<D>;
    __shared__ double part[FIT_RED_GROUPS][WAVE];
    __shared__ double red[WAVE];
    const int k = blockIdx.x, grp = threadIdx.x >> 6, i = threadIdx.x & 63;
    double s = 0.0;
    if (i < G::MW)
        for (int w = grp; w < a.nwaves; w += FIT_RED_GROUPS) s += a.slab[((long long)w * a.K + k) * G::MW + i];
    part[grp][i] = s;
    __syncthreads();
    if (grp == 0) {
        double t = part[0][i];
#pragma unroll
        for (int j = 1; j < FIT_RED_GROUPS; ++j) t += part[j][i];
        red[i] = t;
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= G::SW) return;
    const float* pk = a.pack + k * G::PACK;
    const double Nk = red[0];
    double out;
    if (j < 2) out = Nk;
    else if (j < 2 + D) { const int d = j - 2; out = red[1 + d] + Nk * (double)pk[d]; }
    else {
        const int d = (j - 2 - D) / D, e = (j - 2 - D) % D;
        const int hi = d > e ? d : e, lo = d > e ? e : d;
        const double md = pk[d], me = pk[e];
        out = red[1 + D + hi * (hi + 1) / 2 + lo] + red[1 + d] * me + md * red[1 + e] + Nk * md * me;
    }
    a.stats[(long long)k * G::SW + j] = out;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// The iteration of a fit, after the caller's own pass check: `iterations` times finalize -> fit pack -> pass(), all enqueued on the
// stream without host work.  `nulls` names the pointers checked here in the refusal's text.
template <class Pass>
inline int fit_iterate(const char* who, const char* nulls, int D, int K, const float* alpha0, const float* beta0, const float* m0,
                       const float* C0, const float* v0, float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S,
                       float* pi, float* pack, double* stats, int iterations, void* stream, Pass pass) {
    if (iterations < 0) { set_error("%s: iterations must not be negative (got %d)", who, iterations); return VMP_E_BADARG; }
    if (!alpha0 || !beta0 || !m0 || !C0 || !v0 || !alpha || !beta || !m || !C || !v || !stats) {
        set_error("%s: null pointer (%s)", who, nulls);
        return VMP_E_BADARG;
    }
    for (int it = 0; it < iterations; ++it) {
        int rc = vmp_mix_finalize(stats, D, K, VMP_GMM, alpha0, beta0, m0, C0, v0, nullptr, alpha, beta, m, C, v, xbar, S, pi, nullptr, stream);
        if (rc) return rc;
        if ((rc = vmp_mixture_fit_pack(D, K, alpha, beta, m, C, v, pack, stream)) != 0) return rc;
        if ((rc = pass()) != 0) return rc;
    }
    return 0;
}

}  // namespace vmp
