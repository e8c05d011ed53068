// Fitting the variational Gaussian mixture on partly observed rows (missing at random): the E-step of the factor
// q(z_n, x_n,m) = q(z_n) q(x_n,m | z_n) and the sufficient statistics of the completed rows, in one streaming pass over (x, mask).
//
// Per (row, component) cell, with Lbar = v_k C_k^-1 the expected precision, o / m the observed / missing index sets of the row,
// d_o = x_o - m_k,o:
//   R R^T = Lbar_mm,  t = Lbar_mo d_o,  y = R^-1 t,  q_o = d_o^T Lbar_oo d_o - |y|^2,
//   xhat_m^(k) = m_k,m - R^-T y,   xhat_o^(k) = x_o,   Cov^(k) = Lbar_mm^-1 on the (m,m) block, 0 elsewhere,
//   log rho_nk = c_k - 1/2 q_o - sum_i log R_ii,   c_k = E log pi_k + 1/2 E log|Lambda_k| - D / (2 beta_k),
//   r_nk = softmax_k log rho_nk,   x_fill_m = sum_k r_nk xhat_m^(k),
//   Nk = sum_n r_nk,  sx = sum_n r_nk xhat^(k),  sxx = sum_n r_nk (xhat^(k) xhat^(k)^T + Cov^(k)).
// As in vmp_impute.hip the kernel factors A~ = M Lbar M + (I - M), M = diag(miss): a D x D factorisation with static indices whose
// observed rows and columns are those of the identity.  Its inverse is M Lbar_mm^-1 M + (I - M): the missing block of R^-1 (R^-1)^T is
// Cov^(k), the observed diagonal (exactly 1) is dropped by a select, everything else is a product of exact zeros.  The value in a
// missing slot of x never enters arithmetic.
//
// Moments.  The products are formed in fp32 on xhat - m_k: the shift is the component's own location, which is in the pack, costs
// nothing (x_o - m_k is d_o, xhat_m - m_k is -R^-T y) and is the centre of the rows that carry the component's weight.  Every lane
// adds its rows in fp32; every FIT_CHUNK rows of a wave the four lanes that own a component are added (rows4_sum) and flushed to the
// wave's own fp64 words in the workspace - a plain read-modify-write of words no other wave touches, no atomics.  A second launch adds
// the waves in a fixed order and un-shifts in fp64 into the (K, vmp_mix_stats_words(D)) layout of vmp_mix_stats.
//
// Lane map: lane l = (i16 = l & 15, kk = l >> 4) owns component k = i16 + 16 t of every component tile t and, per loop iteration, the
// data row n4 + kk (vmp_impute.hip).  K <= 16: the component is resident in VGPRs and a cell is evaluated once.  K > 16: a chunk of
// rows is walked twice - first all tiles of a row for the softmax (r, log r and x_fill are written), then tile by tile with the cell
// evaluated again and r read back (the lane's own store), so that one set of accumulators serves every tile.
//
// The cell (fit_cell), the moments (fit_moments), the flush, the row load, the body of the reduction and the block geometry (FIT_*)
// are in vmp_fit_cell.h, which vmp_wfit.hip shares (vmp_bound.hip: the pack's geometry and registers).
#include "vmp_fit_cell.h"

using namespace vmp;

namespace {

struct FitPackArgs {
    int K;
    const float *alpha, *beta, *m, *C, *v;
    float* pack;
};

// One thread per component, fp64 inside, rounded once: P = C^-1 through the Cholesky factor, Lbar = v P, and the constant of
// log rho as compute_log_pi / compute_expct_log_det_prec give it (gmm.py:117-138, the det <= 1e-20 guard included).
template <int D>
__global__ __launch_bounds__(WAVE) void fit_pack_kernel(FitPackArgs a) {
    using G = FitGeo<D>;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    const float qnan = __builtin_nanf("");
    double asum = 0.0;
    for (int j = 0; j < a.K; ++j) asum += a.alpha[j];
    double W[D * D], sumlog;
    const bool ok = spd_factor_inverse<D>(a.C + k * D * D, W, sumlog);
    const double vk = a.v[k], bk = a.beta[k];
    float* p = a.pack + k * G::PACK;
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = ok ? a.m[k * D + j] : qnan;
    packed_inverse_from_factor<D>(W, vk, ok, p + D);
    const double logdetP = -2.0 * sumlog;
    const double ld = (logdetP > log(1e-20)) ? logdetP : 0.0;
    double sdg = 0.0;
    for (int i = 0; i < D; ++i) sdg += digamma_d(0.5 * (vk + 1.0 + i));
    const double elp = digamma_d((double)a.alpha[k]) - digamma_d(asum);
    const double c = elp + 0.5 * (sdg + D * 0.69314718055994530942 + ld) - 0.5 * (D / bk);
    p[G::C] = ok ? (float)c : qnan;
}

struct FitArgs {
    const float* x;
    const uint8_t* mask;
    const float* pack;
    float* r;             // (N,K)
    float* logr;          // (N,K) or NULL
    float* x_fill;        // (N,D) or NULL
    double* slab;         // (waves, K, MW) fp64: the moments of a wave's rows
    long long N;
    long long rpw;        // rows per wave (multiple of 4): wave g owns rows [g rpw, min(N, (g+1) rpw))
    int K;
    int vec_in, vec_out;  // x / x_fill 16-byte aligned
};

template <int D, int KTMAX>
__global__ __launch_bounds__(FIT_NW * WAVE) void fit_kernel(FitArgs a) {
    using G = FitGeo<D>;
    __shared__ float lds[KTMAX * 16 * G::STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, kk = lane >> 4;
    const int KT = KTMAX == 1 ? 1 : (a.K + 15) / 16;

    for (int i = threadIdx.x; i < a.K * G::PACK; i += FIT_NW * WAVE) lds[(i / G::PACK) * G::STRIDE + i % G::PACK] = a.pack[i];
    __syncthreads();
    FitParams<D> p;
    if constexpr (KTMAX == 1) p.load(lds + (i16 < a.K ? i16 : 0) * G::STRIDE);   // lanes beyond K: a readable component, its term forced to -inf

    const long long g = (long long)blockIdx.x * FIT_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    double* slab = a.slab + g * a.K * G::MW;
    if (r0 >= r1) {                                                          // a wave without rows: its moments are zero
        for (int i = lane; i < a.K * G::MW; i += WAVE) slab[i] = 0.0;
        return;
    }
    float acc[G::MW];
#pragma unroll
    for (int i = 0; i < G::MW; ++i) acc[i] = 0.f;

    for (long long c0 = r0; c0 < r1; c0 += FIT_CHUNK) {
        const long long c1 = c0 + FIT_CHUNK < r1 ? c0 + FIT_CHUNK : r1;
        for (long long n4 = c0; n4 < c1; n4 += 4) {
            const long long n = n4 + kk;
            const bool valid = n < c1;
            const long long nr = valid ? n : c1 - 1;                         // rows past the range: a row of the range, discarded
            float x[D];
            bool miss[D];
            fit_load_row<D, true>(a, nr, x, miss);

            // lane-local online log-sum-exp over the lane's tiles: ml = running maximum, s = sum e, ax = sum e xhat
            float ml = -INFINITY, s = 0.f, ax[D], lt[KTMAX], dh[D], A[G::TRI], rd[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ax[d] = 0.f;
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) lt[j] = -INFINITY;
#pragma unroll 1
            for (int t = 0; t < KT; ++t) {
                const int k = t * 16 + i16;
                if constexpr (KTMAX > 1) p.load(lds + (k < a.K ? k : 0) * G::STRIDE);
                float l = fit_cell<D>(p, x, miss, dh, A, rd);
                l = k < a.K ? l : -INFINITY;
#pragma unroll
                for (int j = 0; j < KTMAX; ++j) lt[j] = t == j ? l : lt[j];
                const float mn = fmaxf(ml, l);
                const float sh = mn == -INFINITY ? 0.f : mn;                 // every term so far -inf: -inf - (-inf) would be NaN
                const float c = __expf(ml - sh), e = __expf(l - sh);
                s = fmaf(s, c, e);
#pragma unroll
                for (int d = 0; d < D; ++d) ax[d] = fmaf(ax[d], c, e == 0.f ? 0.f : e * (p.mu[d] + dh[d]));
                ml = mn;
            }
            const float mx = row16_max(ml);
            const float shift = mx == -INFINITY ? 0.f : mx;
            const float f = __expf(ml - shift);
            const float S = row16_sum(s * f);
            const float inv = S == 0.f ? 0.f : 1.0f / S;                     // a row without mass: r = 0, filled entries 0
            const float lp = shift + logf(S);
            if (a.x_fill) {
                float o[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float xs = row16_sum(ax[d] * f) * inv;
                    o[d] = miss[d] ? xs : x[d];
                }
                if (valid && i16 == 0) store_row<D>(a.x_fill + n * D, o, a.vec_out != 0);
            }
            float rk = 0.f;
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) {
                const int k = j * 16 + i16;
                rk = __expf(lt[j] - shift) * inv;
                if (valid && k < a.K) {
                    a.r[n * a.K + k] = rk;
                    if (a.logr) a.logr[n * a.K + k] = lt[j] - lp;
                }
            }
            if constexpr (KTMAX == 1) fit_moments<D>(dh, miss, A, rd, (valid && i16 < a.K) ? rk : 0.f, acc);
        }
        if constexpr (KTMAX == 1) {
            fit_flush<D>(acc, slab + i16 * G::MW, c0 == r0, kk == 0 && i16 < a.K);
        } else {
#pragma unroll 1
            for (int t = 0; t < KT; ++t) {
                const int k = t * 16 + i16;
                p.load(lds + (k < a.K ? k : 0) * G::STRIDE);
                for (long long n4 = c0; n4 < c1; n4 += 4) {
                    const long long n = n4 + kk;
                    const bool valid = n < c1;
                    const long long nr = valid ? n : c1 - 1;
                    float x[D], dh[D], A[G::TRI], rd[D];
                    bool miss[D];
                    fit_load_row<D, true>(a, nr, x, miss);
                    fit_cell<D>(p, x, miss, dh, A, rd);
                    const float rk = (valid && k < a.K) ? a.r[n * a.K + k] : 0.f;      // the lane's own store of the first walk
                    fit_moments<D>(dh, miss, A, rd, rk, acc);
                }
                fit_flush<D>(acc, slab + (k < a.K ? k : 0) * G::MW, c0 == r0, kk == 0 && k < a.K);
            }
        }
    }
}

struct FitReduceArgs {
    const double* slab;
    const float* pack;
    double* stats;        // (K, SW)
    int nwaves, K;
};

// the waves of the slab added in a fixed order and un-shifted by m_k: fit_unshift_reduce (vmp_fit_cell.h)
template <int D>
__global__ __launch_bounds__(FIT_RED_GROUPS * WAVE) void fit_reduce_kernel(FitReduceArgs a) {
    fit_unshift_reduce<D>(a);
}

template <int D>
int launch_fit(const FitArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(FIT_NW * WAVE);
    if (a.K <= 16) hipLaunchKernelGGL((fit_kernel<D, 1>), grid, block, 0, s, a);
    else           hipLaunchKernelGGL((fit_kernel<D, 4>), grid, block, 0, s, a);
    return check_launch("fit_kernel");
}

// every refusal of the pass, decided on the host
int fit_pass_check(const char* who, const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, const float* r_out,
                   const void* ws, size_t ws_bytes) {
    int rc = stream_dims(who, D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !mask || !pack) { set_error("%s: null pointer (%s)", who, !x ? "x" : !mask ? "mask" : "pack"); return VMP_E_BADARG; }
    if (!r_out) { set_error("%s: no output requested (r_out is required)", who); return VMP_E_BADARG; }
    return workspace_check(who, ws, ws_bytes, vmp_mixture_fit_workspace_bytes(N, D, K));
}

}  // namespace

extern "C" {

int vmp_mixture_fit_pack_words(int D) { return (D < 1 || D > VMP_MAX_D) ? 0 : fit_pack_words(D); }

int vmp_mixture_fit_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* C, const float* v,
                         float* pack, void* stream) {
    int rc = stream_dims("vmp_mixture_fit_pack", D, K);
    if (rc) return rc;
    if (!alpha || !beta || !m || !C || !v || !pack) { set_error("vmp_mixture_fit_pack: null pointer"); return VMP_E_BADARG; }
    FitPackArgs a{K, alpha, beta, m, C, v, pack};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((fit_pack_kernel<DD>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
        rc = check_launch("fit_pack_kernel");
    });
    return rc;
}

size_t vmp_mixture_fit_workspace_bytes(int64_t N, int D, int K) {
    if (D < 1 || D > VMP_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    return fit_slab_bytes(N, D, K);
}

int vmp_mixture_fit_pass(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* r_out,
                         float* logr_out, float* x_fill_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = fit_pass_check("vmp_mixture_fit_pass", x, mask, N, D, K, pack, r_out, ws, ws_bytes);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = fit_blocks(N);
    const long long waves = (long long)blocks * FIT_NW;
    FitArgs a{};
    a.x = x; a.mask = mask; a.pack = pack; a.r = r_out; a.logr = logr_out; a.x_fill = x_fill_out;
    a.slab = static_cast<double*>(ws);
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, waves, 4);
    a.vec_in = aligned16(x); a.vec_out = aligned16(x_fill_out);
    rc = -1;
    VMP_SWITCH_DIM(D, DD, rc = launch_fit<DD>(a, blocks, s));
    if (rc || !stats_out) return rc;
    FitReduceArgs ra{a.slab, pack, stats_out, (int)waves, K};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((fit_reduce_kernel<DD>), dim3(K), dim3(FIT_RED_GROUPS * WAVE), 0, s, ra);
        rc = check_launch("fit_reduce_kernel");
    });
    return rc;
}

int vmp_mixture_fit_iterate(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* alpha0, const float* beta0,
                            const float* m0, const float* C0, const float* v0, float* r, float* logr, float* x_fill, float* alpha,
                            float* beta, float* m, float* C, float* v, float* xbar, float* S, float* pi, float* pack, double* stats,
                            void* ws, size_t ws_bytes, int iterations, void* stream) {
    int rc = fit_pass_check("vmp_mixture_fit_iterate", x, mask, N, D, K, pack, r, ws, ws_bytes);
    if (rc) return rc;
    return fit_iterate("vmp_mixture_fit_iterate", "prior, posterior or stats", D, K, alpha0, beta0, m0, C0, v0, alpha, beta, m, C, v, xbar,
                       S, pi, pack, stats, iterations, stream,
                       [&] { return vmp_mixture_fit_pass(x, mask, N, D, K, pack, r, logr, x_fill, stats, ws, ws_bytes, stream); });
}

}  // extern "C"
