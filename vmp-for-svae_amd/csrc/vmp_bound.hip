// Variational lower bound (free energy) of the Gaussian-mixture fit, complete or partly observed rows (include/vmp_hip.h
// "Variational lower bound"):
//   bound = data - kl_pi - sum_k kl_nw_k,
//   data    = sum_n [ logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi ],
//   log rho_nk = c_k - 1/2 q_o - sum_i log R_ii            the cell of vmp_missfit.hip, from the fit pack [m | Lbar = v C^-1 | c_k]:
//                R R^T = Lbar_mm,  t = Lbar_mo d_o,  y = R^-1 t,  q_o = d_o^T Lbar_oo d_o - |y|^2,  d_o = x_o - m_k,o,
//   kl_pi   = KL(Dir(alpha) || Dir(alpha0)) = lgamma(sum alpha) - sum lgamma(alpha) - lgamma(sum alpha0) + sum lgamma(alpha0)
//             + sum_k (alpha_k - alpha0_k) E log pi_k,
//   kl_nw_k = KL(N(mu | m, (beta Lambda)^-1) W(Lambda | C^-1, v) || the same family at (beta0, m0, C0, v0))
//           = 1/2 D log(beta / beta0) - 1/2 D + 1/2 D beta0 / beta + 1/2 beta0 (m - m0)^T Lbar (m - m0)
//             + logB(C, v) - logB(C0, v0) + 1/2 (v - v0) E log|Lambda| - 1/2 v D + 1/2 tr(C0 Lbar),
//   logB(C, nu) = 1/2 nu log|C| - 1/2 nu D log 2 - 1/4 D (D - 1) log pi - sum_{i=1..D} lgamma((nu + 1 - i) / 2),
// with E log pi and E log|Lambda| the expectations of fit_pack_kernel (digamma arguments (v + 1 + i) / 2, the det <= 1e-20 guard).
//
// Streaming kernel: the lane map of vmp_mix_stream.h - lane l = (i16 = l & 15, kk = l >> 4) owns component i16 + 16 t of every tile
// and the data row n4 + kk; a wave walks a contiguous range of rows - and the row sum of that header: no atomics, one geometry
// whichever outputs are requested, bit-identical from run to run.  The cell is the part of fit_cell (vmp_fit_cell.h) that log rho
// needs, in the same operations: the factor and the forward substitution, no back-substitution, no xhat, no inverse; without a mask
// there is nothing to factor and log rho = c - 1/2 d^T Lbar d.  What a missing slot of x holds never enters arithmetic.
// K-sized kernel: one thread per component, fp64 inside; the sums over k are taken by one thread in k order.
#include "vmp_fit_cell.h"

using namespace vmp;

namespace {

// not the FIT_* geometry of the two fits: no moments to flush, so more and smaller blocks (that of vmp_impute.hip)
constexpr int BND_NW = 4;                 // waves per block
constexpr int BND_MAX_BLOCKS = 2048;      // 8 waves per SIMD on 256 CUs
constexpr int BND_ROWS_PER_BLOCK = 64 * BND_NW;       // below that a block is not worth its launch slot

inline int bound_blocks(int64_t N) { return stream_blocks(N, BND_ROWS_PER_BLOCK, BND_MAX_BLOCKS); }

// The two cells below are fit_cell_full and fit_cell (vmp_fit_cell.h) without the outputs that log rho does not need.  Calling those
// with the outputs dropped computes the same bits, but the compiler orders the instructions of 26 of the 32 bound_kernel forms
// differently (profiles/NOTES_mix_fit_shared.md), so the text stays here, as does the row load with its hoisted `vec`.

// complete row: c - 1/2 d^T Lbar d, the quadratic form over the lower triangle (the diagonal halved, the rest counted once)
template <int D>
__device__ __forceinline__ float bound_cell_full(const FitParams<D>& p, const float (&x)[D]) {
    float d[D];
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

// partly observed row: fit_cell of vmp_fit_cell.h up to |y|^2 - the factor of A~ = M Lbar M + (I - M), sum log R_ii from its pivots,
// the forward substitution y = R^-1 t - in the same operations
template <int D>
__device__ __forceinline__ float bound_cell_masked(const FitParams<D>& p, const float (&x)[D], const bool (&miss)[D]) {
    using G = FitGeo<D>;
    float dt[D], v[D], A[G::TRI], rd[D], piv[D];
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
    float yy = 0.f;                              // y = R^-1 t, |y|^2
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float s = v[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s = fmaf(-A[i * (i + 1) / 2 + q], v[q], s);
        v[i] = s * rd[i];
        yy = fmaf(v[i], v[i], yy);
    }
    float q = qo - yy;
    q = q < 0.f ? 0.f : q;                       // rounding of the difference; a NaN stays a NaN
    return (p.c - slog) - 0.5f * q;
}

struct BoundArgs {
    const float* x;
    const uint8_t* mask;  // (N,D) or NULL
    const float* pack;
    float* lse;           // (N) or NULL
    double* partials;     // (blocks)
    long long N;
    long long rpw;        // rows per wave (multiple of 4): wave g owns rows [g rpw, min(N, (g+1) rpw))
    int K;
    int vec_in;           // x 16-byte aligned
};

template <int D, int KTMAX, bool MASKED>
__global__ __launch_bounds__(BND_NW * WAVE) void bound_kernel(BoundArgs a) {
    using G = FitGeo<D>;
    __shared__ float lds[KTMAX * 16 * G::STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, kk = lane >> 4;
    const int KT = KTMAX == 1 ? 1 : (a.K + 15) / 16;

    for (int i = threadIdx.x; i < a.K * G::PACK; i += BND_NW * WAVE) lds[(i / G::PACK) * G::STRIDE + i % G::PACK] = a.pack[i];
    __syncthreads();
    FitParams<D> p;
    if constexpr (KTMAX == 1) p.load(lds + (i16 < a.K ? i16 : 0) * G::STRIDE);   // lanes beyond K: a readable component, its term forced to -inf

    const long long g = (long long)blockIdx.x * BND_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;                  // a wave without rows: r0 >= r1, its sum stays 0
    const bool vec = a.vec_in != 0;
    const double HALF_LOG_2PI = 0.91893853320467274178;
    double acc = 0.0;
    for (long long n4 = r0; n4 < r1; n4 += 4) {
        const long long n = n4 + kk;
        const bool valid = n < r1;
        const long long nr = valid ? n : r1 - 1;                               // rows past the range: a row of the range, discarded
        float x[D];
        load_row<D>(a.x + nr * D, x, vec);
        bool miss[D];
        int n_obs = D;
        if constexpr (MASKED) {
            n_obs = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) { miss[d] = a.mask[nr * D + d] != 0; n_obs += miss[d] ? 0 : 1; }
        }
        // lane-local online log-sum-exp over the lane's tiles: ml = running maximum, s = sum e
        float ml = -INFINITY, s = 0.f;
#pragma unroll 1
        for (int t = 0; t < KT; ++t) {
            const int k = t * 16 + i16;
            if constexpr (KTMAX > 1) p.load(lds + (k < a.K ? k : 0) * G::STRIDE);
            float l;
            if constexpr (MASKED) l = bound_cell_masked<D>(p, x, miss);
            else                  l = bound_cell_full<D>(p, x);
            l = k < a.K ? l : -INFINITY;
            const float mn = fmaxf(ml, l);
            const float sh = mn == -INFINITY ? 0.f : mn;                       // every term so far -inf: -inf - (-inf) would be NaN
            s = fmaf(s, __expf(ml - sh), __expf(l - sh));
            ml = mn;
        }
        const float mx = row16_max(ml);
        const float shift = mx == -INFINITY ? 0.f : mx;
        const float S = row16_sum(s * __expf(ml - shift));
        const float lse = shift + logf(S);                                     // every term -inf: S = 0, lse = -inf; a NaN term: NaN
        if (valid) acc += (double)lse - HALF_LOG_2PI * (double)n_obs;          // lanes i16 = 0 are the ones the row sum reads
        if (a.lse && valid && i16 == 0) a.lse[n] = lse;
    }
    wave_block_sum<BND_NW>(acc, lane, wave, a.partials);
}

__global__ __launch_bounds__(WAVE) void bound_sum_kernel(const double* partials, int nblk, double* out) { block_sum(partials, nblk, out); }

template <int D, bool MASKED>
int launch_bound(const BoundArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(BND_NW * WAVE);
    if (a.K <= 16) hipLaunchKernelGGL((bound_kernel<D, 1, MASKED>), grid, block, 0, s, a);
    else           hipLaunchKernelGGL((bound_kernel<D, 4, MASKED>), grid, block, 0, s, a);
    return check_launch("bound_kernel");
}

struct BoundTermsArgs {
    int K;
    const float *alpha0, *beta0, *m0, *C0, *v0;
    const float *alpha, *beta, *m, *C, *v;
    double* out;          // [kl_pi | sum_k kl_nw_k | kl_nw_0 .. kl_nw_{K-1}]
};

// log B(C, nu) of the Wishart W(Lambda | C^-1, nu), logdetC = log|C|
template <int D>
__device__ __forceinline__ double log_B(double logdetC, double nu) {
    double s = 0.5 * nu * logdetC - 0.5 * nu * D * 0.69314718055994530942 - 0.25 * D * (D - 1) * 1.14472988584940017414;
    for (int i = 1; i <= D; ++i) s -= lgamma(0.5 * (nu + 1.0 - i));
    return s;
}

// One block of VMP_MAX_K threads, thread k owns component k; thread 0 adds in k order.  A component whose C or C0 is not symmetric
// positive definite gets NaN, and so do the sums.
template <int D>
__global__ __launch_bounds__(WAVE) void bound_terms_kernel(BoundTermsArgs a) {
    __shared__ double nw[WAVE], dir[WAVE];
    const int k = threadIdx.x;
    double asum = 0.0, a0sum = 0.0;
    for (int j = 0; j < a.K; ++j) { asum += a.alpha[j]; a0sum += a.alpha0[j]; }
    if (k < a.K) {
        const double qnan = __builtin_nan("");
        double ld0;                                                            // log|C0|
        bool ok;
        {
            double A0[D * D];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) A0[i * D + j] = 0.5 * ((double)a.C0[(k * D + i) * D + j] + (double)a.C0[(k * D + j) * D + i]);
            ok = chol_lower<D>(A0);
            ld0 = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) ld0 += log(A0[i * D + i]);
            ld0 *= 2.0;
        }
        double W[D * D], sumlog;                                               // C = L L^T, W = L^-1: C^-1 = W^T W, log|C| = 2 sumlog
        ok = spd_factor_inverse<D>(a.C + k * D * D, W, sumlog) && ok;
        const double vk = a.v[k], bk = a.beta[k], v0 = a.v0[k], b0 = a.beta0[k], al = a.alpha[k], al0 = a.alpha0[k];
        const double logdetP = -2.0 * sumlog;
        const double ld = (logdetP > log(1e-20)) ? logdetP : 0.0;
        double sdg = 0.0;
        for (int i = 0; i < D; ++i) sdg += digamma_d(0.5 * (vk + 1.0 + i));
        const double eld = sdg + D * 0.69314718055994530942 + ld;              // E log|Lambda|
        const double elp = digamma_d(al) - digamma_d(asum);                    // E log pi
        double dm[D];
#pragma unroll
        for (int i = 0; i < D; ++i) dm[i] = (double)a.m[k * D + i] - (double)a.m0[k * D + i];
        // (m - m0)^T C^-1 (m - m0) = |W dm|^2;  tr(C0 C^-1) = sum_q w_q^T C0 w_q over the rows w_q of W
        double maha = 0.0, tr = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            double y = 0.0, t = 0.0;
#pragma unroll
            for (int i = 0; i <= q; ++i) {
                y += W[q * D + i] * dm[i];
                double u = 0.0;
#pragma unroll
                for (int j = 0; j <= q; ++j) u += 0.5 * ((double)a.C0[(k * D + i) * D + j] + (double)a.C0[(k * D + j) * D + i]) * W[q * D + j];
                t += W[q * D + i] * u;
            }
            maha += y * y;
            tr += t;
        }
        const double kl = 0.5 * D * log(bk / b0) - 0.5 * D + 0.5 * D * b0 / bk + 0.5 * b0 * vk * maha
                          + log_B<D>(2.0 * sumlog, vk) - log_B<D>(ld0, v0) + 0.5 * (vk - v0) * eld - 0.5 * vk * D + 0.5 * vk * tr;
        nw[k] = ok ? kl : qnan;
        dir[k] = lgamma(al0) - lgamma(al) + (al - al0) * elp;
        a.out[2 + k] = nw[k];
    }
    __syncthreads();
    if (k == 0) {
        double snw = 0.0, sdir = lgamma(asum) - lgamma(a0sum);
        for (int j = 0; j < a.K; ++j) { snw += nw[j]; sdir += dir[j]; }
        a.out[0] = sdir;
        a.out[1] = snw;
    }
}

// every refusal of the pass, decided on the host
int bound_pass_check(const char* who, const float* x, int64_t N, int D, int K, const float* pack, const double* data_out, const void* ws,
                     size_t ws_bytes) {
    int rc = stream_dims(who, D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !pack || !data_out) { set_error("%s: null pointer (%s)", who, !x ? "x" : !pack ? "fit_pack" : "data_out"); return VMP_E_BADARG; }
    return workspace_check(who, ws, ws_bytes, vmp_mixture_bound_workspace_bytes(N, D, K));
}

}  // namespace

extern "C" {

size_t vmp_mixture_bound_workspace_bytes(int64_t N, int D, int K) {
    if (D < 1 || D > VMP_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    return (size_t)bound_blocks(N) * sizeof(double);           // one fp64 partial per block
}

int vmp_mixture_bound_pass(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* fit_pack, float* lse_out,
                           double* data_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = bound_pass_check("vmp_mixture_bound_pass", x, N, D, K, fit_pack, data_out, ws, ws_bytes);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = bound_blocks(N);
    BoundArgs a{};
    a.x = x; a.mask = mask; a.pack = fit_pack; a.lse = lse_out; a.partials = static_cast<double*>(ws);
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, (long long)blocks * BND_NW, 4);
    a.vec_in = aligned16(x);
    rc = -1;
    if (mask) { VMP_SWITCH_DIM(D, DD, rc = (launch_bound<DD, true>(a, blocks, s))); }
    else      { VMP_SWITCH_DIM(D, DD, rc = (launch_bound<DD, false>(a, blocks, s))); }
    if (rc) return rc;
    hipLaunchKernelGGL(bound_sum_kernel, dim3(1), dim3(WAVE), 0, s, a.partials, blocks, data_out);
    return check_launch("bound_sum_kernel");
}

int vmp_mixture_bound_terms(int D, int K, const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                            const float* alpha, const float* beta, const float* m, const float* C, const float* v, double* out,
                            void* stream) {
    int rc = stream_dims("vmp_mixture_bound_terms", D, K);
    if (rc) return rc;
    if (!alpha0 || !beta0 || !m0 || !C0 || !v0 || !alpha || !beta || !m || !C || !v || !out) {
        set_error("vmp_mixture_bound_terms: null pointer (prior, posterior or out)");
        return VMP_E_BADARG;
    }
    BoundTermsArgs a{K, alpha0, beta0, m0, C0, v0, alpha, beta, m, C, v, out};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((bound_terms_kernel<DD>), dim3(1), dim3(WAVE), 0, static_cast<hipStream_t>(stream), a);
        rc = check_launch("bound_terms_kernel");
    });
    return rc;
}

}  // extern "C"
