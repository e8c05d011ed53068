// Mixture imputation: marginal log density of the observed part of a row, the responsibilities that follow from it and the
// conditional location of the missing part, under a mixture of Student-t densities, in one streaming pass over (x, mask).
//
// Per (row, component) cell, with Lambda = Sigma^-1, o / m the observed / missing index sets of the row, d_o = x_o - mu_o:
//   R R^T = Lambda_mm,  t = Lambda_mo d_o,  y = R^-1 t,  q = d_o^T Lambda_oo d_o - |y|^2  (= d_o^T Sigma_oo^-1 d_o),
//   log det Sigma_oo = -log det Lambda + 2 sum_i log R_ii,
//   l_k = log w_k + G_k[D_o] - 1/2 log det Sigma_oo - (nu + D_o)/2 log1p(q / nu),   xhat_m^(k) = mu_m - R^-T y,
//   logp = logsumexp_k l_k,  r_k = exp(l_k - logp),  xhat_m = sum_k r_k xhat_m^(k).
// The shape of the Cholesky depends on the row's own missing pattern; with M = diag(miss) the kernel factors
// A~ = M Lambda M + (I - M) instead: a D x D factorisation with static indices whose observed rows and columns are those of the
// identity (pivot 1, log 0, solution 0), so log det A~ = log det Lambda_mm and no permutation or dynamic register index is needed.
// The value in a missing slot of x never enters arithmetic: d~ = miss ? 0 : x - mu is a select.
//
// Two K-sized kernels build the impute pack (fp64 inside, rounded once on the way out, one thread per component as the score packs
// of vmp_score.hip); the streaming kernel evaluates no lgamma: the D + 1 constants G_k[j] are in the pack.
//
// Lane map of the streaming kernel (the scoring kernel's): lane l = (i16 = l & 15, kk = l >> 4) owns component k = i16 + 16 t of
// every component tile t and, per loop iteration, the data row n4 + kk: the 16 lanes of a DPP row cover one data row, a wave
// advances 4 rows per iteration over a contiguous range of rows that depends on (N, blocks) only.  The packs are staged in LDS once per block
// (K = 64, D = 8: 14.6 KB).  K <= 16: the lane's component is resident in its VGPRs, loaded once per kernel; only G_k[D_o] is read
// from LDS per cell.  K > 16: the lane reloads its component per tile and walks its tiles with a lane-local online log-sum-exp that rescales its running sum_k e_k xhat^(k); the 16 lanes are combined once per row
// (row16_max, then D + 1 row16_sum).  The row sum is the deterministic one of vmp_mix_stream.h.
#include "vmp_impute_pack.h"

using namespace vmp;

namespace {

constexpr int IMP_NW = 4;                 // waves per block
constexpr int IMP_MAX_BLOCKS = 2048;
constexpr int IMP_ROWS_PER_BLOCK = 64 * IMP_NW;

inline int impute_blocks(int64_t N) { return stream_blocks(N, IMP_ROWS_PER_BLOCK, IMP_MAX_BLOCKS); }

// ---------------------------------------------------------------------------------------------------------
// impute packs (layout: vmp_impute_pack.h)
// ---------------------------------------------------------------------------------------------------------
struct ImputePackArgs {
    int K;
    const float *w, *beta, *m, *S, *nu;     // NIW: alpha, beta, m, C, v;  explicit: log_w, -, mu, sigma, nu
    float* pack;
};

// pack row of a component with scale matrix S / scale (precision scale S^-1), log weight lw and nu degrees of freedom
template <int D>
__device__ __forceinline__ void write_impute_pack(const ImputePackArgs& a, int k, double scale, double lw, double nu, bool ok) {
    using G = ImputeGeo<D>;
    const double PI = 3.14159265358979323846;
    const float qnan = __builtin_nanf("");
    double W[D * D], sumlog;
    ok = spd_factor_inverse<D>(a.S + k * D * D, W, sumlog) && ok;
    float* p = a.pack + k * G::PACK;
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = ok ? a.m[k * D + j] : qnan;
    packed_inverse_from_factor<D>(W, scale, ok, p + D);
    p[G::LW] = ok ? (float)lw : qnan;
    p[G::NU] = ok ? (float)nu : qnan;
    p[G::LDET] = ok ? (float)(D * log(scale) - 2.0 * sumlog) : qnan;
    p[G::INU] = ok ? (float)(1.0 / nu) : qnan;
    const double lg0 = lgamma(0.5 * nu), lpn = log(PI * nu);
    for (int j = 0; j <= D; ++j) p[G::G + j] = ok ? (float)(lgamma(0.5 * (nu + j)) - lg0 - 0.5 * j * lpn) : qnan;
}

// posterior predictive of the NIW posterior (alpha, beta, m, C, v): w = alpha / sum alpha, mu = m, nu' = v + 1 - D,
// Sigma = C (1 + beta) / (beta nu') - the mapping of score_pack_niw_kernel (vmp_score.hip)
template <int D>
__global__ __launch_bounds__(WAVE) void impute_pack_niw_kernel(ImputePackArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    double asum = 0.0;
    for (int j = 0; j < a.K; ++j) asum += a.w[j];
    const double beta = a.beta[k], nup = (double)a.nu[k] + 1.0 - D;
    const bool ok = nup > 0.0;
    write_impute_pack<D>(a, k, nup * beta / (1.0 + beta), log((double)a.w[k] / asum), nup, ok);
}

// explicit Student-t parameters (log_w, mu, sigma, nu)
template <int D>
__global__ __launch_bounds__(WAVE) void impute_pack_t_kernel(ImputePackArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    const double nu = a.nu[k];
    write_impute_pack<D>(a, k, 1.0, (double)a.w[k], nu, nu > 0.0);
}

// ---------------------------------------------------------------------------------------------------------
// streaming kernel
// ---------------------------------------------------------------------------------------------------------
struct ImputeArgs {
    const float* x;
    const uint8_t* mask;
    const float* pack;
    float* x_out;         // (N,D) or NULL; may be x
    float* logp;          // (N) or NULL
    float* resp;          // (N,K) or NULL
    double* partials;     // (blocks) or NULL
    long long N;
    long long rpw;        // rows per wave (multiple of 4): wave g owns rows [g rpw, min(N, (g+1) rpw))
    int K;
    int vec_in, vec_out;  // x / x_out 16-byte aligned
};

// One (row, component) cell: the term l_k and the conditional location xh[] (mu - z; meaningful in the missing slots only);
// g = G_k[n_obs].  x[] holds whatever the caller's buffer holds in the missing slots: it is read through the select only.
template <int D>
__device__ __forceinline__ float impute_cell(const ImputeParams<D>& p, const float (&x)[D], const bool (&miss)[D], int n_obs,
                                             float g, float (&xh)[D]) {
    float dt[D], v[D];
#pragma unroll
    for (int d = 0; d < D; ++d) dt[d] = miss[d] ? 0.f : x[d] - p.mu[d];
    // v = Lambda d~;  observed rows: the quadratic form d_o^T Lambda_oo d_o,  missing rows: t = Lambda_mo d_o
    float qo = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float s = p.L(i, 0) * dt[0];
#pragma unroll
        for (int j = 1; j < D; ++j) s = fmaf(p.L(i, j), dt[j], s);
        v[i] = miss[i] ? s : 0.f;
        qo = fmaf(dt[i], s, qo);                 // dt[i] = 0 in the missing rows
    }
    // A~ = M Lambda M + (I - M), lower Cholesky in place (off-diagonal entries; the diagonal is kept as 1 / R_jj)
    float A[ImputeGeo<D>::TRI], rd[D], piv[D];
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
    // sum_i log R_ii = 1/2 sum log pivot, two pivots per logarithm
    float slog = 0.f;
#pragma unroll
    for (int j = 0; j + 1 < D; j += 2) slog += logf(piv[j] * piv[j + 1]);
    if constexpr (D % 2) slog += logf(piv[D - 1]);
    slog *= 0.5f;
    // y = R^-1 t (in v), |y|^2, z = R^-T y (in v)
    float yy = 0.f;
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
    for (int d = 0; d < D; ++d) xh[d] = p.mu[d] - v[d];
    float q = qo - yy;
    q = q < 0.f ? 0.f : q;                       // rounding of the difference; a NaN stays a NaN
    const float h = 0.5f * (p.nu + (float)n_obs);
    const float l = (p.lw + g) + (0.5f * p.ldet - slog) - h * log1p_f(q * p.inu);
    return n_obs == 0 ? p.lw : l;                // nothing observed: the weight alone (log det Lambda_mm = log det Lambda exactly)
}

// The packs are staged in LDS once per block.  KTMAX = 1: K <= 16, the lane's component is loaded from there into registers once per
// kernel;  KTMAX = 4: the lane walks ceil(K / 16) tiles and reloads per tile.  G_k[D_o] is read from LDS per cell in both forms (a
// select chain over registers is turned into an indexed private-memory load by the compiler: scratch inside the row loop).
template <int D, int KTMAX>
__global__ __launch_bounds__(IMP_NW * WAVE) void impute_kernel(ImputeArgs a) {
    using G = ImputeGeo<D>;
    __shared__ float lds[KTMAX * 16 * G::STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, kk = lane >> 4;
    const int KT = KTMAX == 1 ? 1 : (a.K + 15) / 16;

    for (int i = threadIdx.x; i < a.K * G::PACK; i += IMP_NW * WAVE) lds[(i / G::PACK) * G::STRIDE + i % G::PACK] = a.pack[i];
    __syncthreads();
    ImputeParams<D> p;
    if constexpr (KTMAX == 1) p.load(lds + (i16 < a.K ? i16 : 0) * G::STRIDE);   // lanes beyond K: a readable component, its term forced to -inf

    const long long g = (long long)blockIdx.x * IMP_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    double acc = 0.0;
    for (long long n4 = r0; n4 < r1; n4 += 4) {
        const long long n = n4 + kk;
        const bool valid = n < r1;
        const long long nr = valid ? n : r1 - 1;                         // rows past the range: a row of the range, discarded
        float x[D];
        load_row<D>(a.x + nr * D, x, a.vec_in != 0);
        bool miss[D];
        int n_obs = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) { miss[d] = a.mask[nr * D + d] != 0; n_obs += miss[d] ? 0 : 1; }

        // lane-local online log-sum-exp over the lane's tiles: ml = running maximum, s = sum e, ax = sum e xhat
        float ml = -INFINITY, s = 0.f, ax[D], lt[KTMAX];
#pragma unroll
        for (int d = 0; d < D; ++d) ax[d] = 0.f;
#pragma unroll
        for (int j = 0; j < KTMAX; ++j) lt[j] = -INFINITY;
#pragma unroll 1
        for (int t = 0; t < KT; ++t) {
            const int k = t * 16 + i16;
            const float* row = lds + (k < a.K ? k : 0) * G::STRIDE;
            if constexpr (KTMAX > 1) p.load(row);
            float xh[D];
            float l = impute_cell<D>(p, x, miss, n_obs, row[G::G + n_obs], xh);
            l = k < a.K ? l : -INFINITY;
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) lt[j] = t == j ? l : lt[j];
            const float mn = fmaxf(ml, l);
            const float sh = mn == -INFINITY ? 0.f : mn;                 // every term so far -inf: -inf - (-inf) would be NaN
            const float c = __expf(ml - sh), e = __expf(l - sh);
            s = fmaf(s, c, e);
#pragma unroll
            for (int d = 0; d < D; ++d) ax[d] = fmaf(ax[d], c, e == 0.f ? 0.f : e * xh[d]);
            ml = mn;
        }
        const float mx = row16_max(ml);
        const float shift = mx == -INFINITY ? 0.f : mx;
        const float f = __expf(ml - shift);
        const float S = row16_sum(s * f);
        const float inv = S == 0.f ? 0.f : 1.0f / S;                     // a row without mass: resp = 0, filled entries 0
        const float lp = shift + logf(S);
        if (valid) acc += (double)lp;
        if (a.x_out) {
            float o[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float xs = row16_sum(ax[d] * f) * inv;
                o[d] = miss[d] ? xs : x[d];
            }
            if (valid && i16 == 0) store_row<D>(a.x_out + n * D, o, a.vec_out != 0);
        }
        if (a.logp && valid && i16 == 0) a.logp[n] = lp;
        if (a.resp) {
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) {
                const int k = j * 16 + i16;
                if (valid && k < a.K) a.resp[n * a.K + k] = __expf(lt[j] - shift) * inv;
            }
        }
    }
    if (a.partials) wave_block_sum<IMP_NW>(acc, lane, wave, a.partials);
}

__global__ __launch_bounds__(WAVE) void impute_sum_kernel(const double* partials, int nblk, double* out) { block_sum(partials, nblk, out); }

template <int D>
int launch_impute(const ImputeArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(IMP_NW * WAVE);
    if (a.K <= 16) hipLaunchKernelGGL((impute_kernel<D, 1>), grid, block, 0, s, a);
    else           hipLaunchKernelGGL((impute_kernel<D, 4>), grid, block, 0, s, a);
    return check_launch("impute_kernel");
}

}  // namespace

extern "C" {

int vmp_mixture_impute_pack_words(int D) { return (D < 1 || D > VMP_MAX_D) ? 0 : impute_pack_words(D); }

int vmp_mixture_impute_pack_niw(int D, int K, const float* alpha, const float* beta, const float* m, const float* C, const float* v,
                                float* pack, void* stream) {
    int rc = stream_dims("vmp_mixture_impute_pack_niw", D, K);
    if (rc) return rc;
    if (!alpha || !beta || !m || !C || !v || !pack) { set_error("vmp_mixture_impute_pack_niw: null pointer"); return VMP_E_BADARG; }
    ImputePackArgs a{K, alpha, beta, m, C, v, pack};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((impute_pack_niw_kernel<DD>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
        rc = check_launch("impute_pack_niw_kernel");
    });
    return rc;
}

int vmp_mixture_impute_pack_t(int D, int K, const float* log_w, const float* mu, const float* sigma, const float* nu, float* pack,
                              void* stream) {
    int rc = stream_dims("vmp_mixture_impute_pack_t", D, K);
    if (rc) return rc;
    if (!log_w || !mu || !sigma || !nu || !pack) { set_error("vmp_mixture_impute_pack_t: null pointer"); return VMP_E_BADARG; }
    ImputePackArgs a{K, log_w, nullptr, mu, sigma, nu, pack};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((impute_pack_t_kernel<DD>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
        rc = check_launch("impute_pack_t_kernel");
    });
    return rc;
}

size_t vmp_mixture_impute_workspace_bytes(int64_t N, int D, int K) {
    (void)D; (void)K;
    return (size_t)impute_blocks(N) * sizeof(double);         // one fp64 partial per block
}

int vmp_mixture_impute(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* x_out,
                       float* logp_out, float* resp_out, double* sum_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = stream_dims("vmp_mixture_impute", D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("vmp_mixture_impute: N must be positive (got %lld)", (long long)N); return VMP_E_BADARG; }
    if (!x || !mask || !pack) { set_error("vmp_mixture_impute: null pointer (%s)", !x ? "x" : !mask ? "mask" : "pack"); return VMP_E_BADARG; }
    if (!x_out && !logp_out && !resp_out && !sum_out) { set_error("vmp_mixture_impute: no output requested"); return VMP_E_BADARG; }
    if ((rc = sum_workspace_check("vmp_mixture_impute", sum_out, ws, ws_bytes, vmp_mixture_impute_workspace_bytes(N, D, K))) != 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = impute_blocks(N);
    const long long waves = (long long)blocks * IMP_NW;
    ImputeArgs a{};
    a.x = x; a.mask = mask; a.pack = pack; a.x_out = x_out; a.logp = logp_out; a.resp = resp_out;
    a.partials = sum_out ? static_cast<double*>(ws) : nullptr;
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, waves, 4);
    a.vec_in = aligned16(x); a.vec_out = aligned16(x_out);
    rc = -1;
    VMP_SWITCH_DIM(D, DD, rc = launch_impute<DD>(a, blocks, s));
    if (rc || !sum_out) return rc;
    hipLaunchKernelGGL(impute_sum_kernel, dim3(1), dim3(WAVE), 0, s, a.partials, blocks, sum_out);
    return check_launch("impute_sum_kernel");
}

}  // extern "C"
