// Mixture scoring: log p(x_n) = logsumexp_k [ c_k - h_k log1p(a_k q_nk) ],  q_nk = |W_k (x_n - m_k)|^2, in one streaming pass.
//
// Both scores of the pure mixtures are mixtures of Student-t densities of this form:
//   variational GMM  - the posterior predictive (Bishop, PRML 10.81-10.82) of the NIW posterior gmm.inference returns
//                      (reference models/gmm.py:230-269; C_k is the inverse scale, P_k = C_k^-1 at gmm.py:260);
//   Student-t mixture - the plug-in mixture of reference distributions/student_t.py:31-37, 42-56 + a log-sum-exp over k.
// Two K-sized kernels build the score pack (fp64 inside, rounded once on the way out, one thread per component as pack_kernel of
// vmp_mix.hip); one streaming kernel reads x once and writes N numbers (and, on request, the (N,K) predictive responsibilities).
//
// Lane map of the streaming kernel (vmp_mix_stream.h; the E-part's, vmp_mix.hip): the lane's components - W_k, m_k, c_k, h_k, a_k of
// every tile t < KT = ceil(K / 16) - are resident in its VGPRs, loaded once per kernel, and per loop iteration it owns the two data
// rows n8 + kk and n8 + 4 + kk: a wave advances 8 rows per iteration.  No LDS in the loop, no scalar loads in the loop, no packed
// fp32 (Makefile).  The row sum is the deterministic one of vmp_mix_stream.h.
#include "vmp_mix_stream.h"

using namespace vmp;

namespace {

constexpr int SCORE_NW = 4;               // waves per block
constexpr int SCORE_MAX_BLOCKS = 2048;    // 8 waves per SIMD on 256 CUs
constexpr int SCORE_ROWS_PER_BLOCK = 64 * SCORE_NW;   // below that a block is not worth its launch slot

inline int score_blocks(int64_t N) { return stream_blocks(N, SCORE_ROWS_PER_BLOCK, SCORE_MAX_BLOCKS); }

// ---------------------------------------------------------------------------------------------------------
// score packs:  [ m_k (D) | W_k lower, row-major packed (D(D+1)/2) | c_k | h_k | a_k | 0 ]   (natural-log units)
// ---------------------------------------------------------------------------------------------------------
struct ScorePackArgs {
    int K;
    const float *w, *beta, *m, *S, *nu;     // NIW: alpha, beta, m, C, v;  explicit: log_w, -, mu, sigma, nu
    float* pack;
};

template <int D>
__device__ __forceinline__ void write_score_pack(float* pack, int k, const float* m, const double (&W)[D * D], bool ok,
                                                 double c, double h, double a) {
    float* p = pack + k * Geo<D>::PACK;
    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = m[k * D + j];
    int idx = D;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) p[idx++] = ok ? (float)W[i * D + j] : qnan;
    p[idx++] = ok ? (float)c : qnan;
    p[idx++] = ok ? (float)h : qnan;
    p[idx++] = ok ? (float)a : qnan;
    p[idx++] = 0.f;
}

// posterior predictive of the NIW posterior (alpha, beta, m, C, v): Student-t with nu' = v + 1 - D degrees of freedom and
// precision nu' beta / (1 + beta) C^-1 (Bishop 10.81-10.82 with (nu, W) = (v, C^-1), as gmm.py:84-94 reads the pair)
template <int D>
__global__ __launch_bounds__(WAVE) void score_pack_niw_kernel(ScorePackArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    const double PI = 3.14159265358979323846;
    double asum = 0.0;
    for (int j = 0; j < a.K; ++j) asum += a.w[j];
    double W[D * D], sumlog;
    bool ok = spd_factor_inverse<D>(a.S + k * D * D, W, sumlog);
    const double beta = a.beta[k], nup = (double)a.nu[k] + 1.0 - D;
    ok = ok && nup > 0.0;
    const double sa = beta / (1.0 + beta), h = 0.5 * (nup + D), s = nup * sa;
    const double c = log((double)a.w[k] / asum) + lgamma(h) - lgamma(0.5 * nup) - 0.5 * D * log(PI * nup) + 0.5 * D * log(s)
                     - sumlog;
    write_score_pack<D>(a.pack, k, a.m, W, ok, c, h, sa);
}

// explicit Student-t parameters (log_w, mu, sigma, nu): reference distributions/student_t.py:31-37
template <int D>
__global__ __launch_bounds__(WAVE) void score_pack_t_kernel(ScorePackArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    const double PI = 3.14159265358979323846;
    double W[D * D], sumlog;
    bool ok = spd_factor_inverse<D>(a.S + k * D * D, W, sumlog);
    const double nu = a.nu[k];
    ok = ok && nu > 0.0;
    const double h = 0.5 * (nu + D);
    const double c = (double)a.w[k] + lgamma(h) - lgamma(0.5 * nu) - 0.5 * D * log(PI * nu) - sumlog;
    write_score_pack<D>(a.pack, k, a.m, W, ok, c, h, 1.0 / nu);
}

// ---------------------------------------------------------------------------------------------------------
// streaming score kernel
// ---------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const float* x;
    const float* pack;
    float* logp;          // (N) or NULL
    float* resp;          // (N,K) or NULL
    double* partials;     // (blocks) or NULL
    long long N;
    long long rpw;        // rows per wave (multiple of 8): wave g owns rows [g rpw, min(N, (g+1) rpw))
    int K;
    int vec_ok;           // x 16-byte aligned (vector row loads allowed)
};

template <int D, int KT>
struct ScoreParams {
    float m[KT][D], W[KT][Geo<D>::TRI], c[KT], h[KT], a[KT];
};

// c - h log1p(a |W (x - m)|^2) of one (row, component) cell
template <int D, int KT>
__device__ __forceinline__ float score_cell(const ScoreParams<D, KT>& p, int t, const float (&x)[D]) {
    float u[D];
#pragma unroll
    for (int d = 0; d < D; ++d) u[d] = x[d] - p.m[t][d];
    float q = 0.f;
    int idx = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float y = p.W[t][idx++] * u[0];
#pragma unroll
        for (int j = 1; j <= i; ++j) y = fmaf(p.W[t][idx++], u[j], y);
        q = fmaf(y, y, q);
    }
    return p.c[t] - p.h[t] * log1p_f(p.a[t] * q);
}

// One data row against all components: per-lane terms t[] in, row value out; e[] = exp(t - shift), inv = 1 / sum (0 for a row
// without mass).  The shift is the row maximum unless that is -inf (every term -inf): -inf - (-inf) would be NaN where the
// answer is exp(-inf) = 0 and log p = -inf.
template <int KT>
__device__ __forceinline__ float score_row(const float (&t)[KT], float (&e)[KT], float& inv) {
    float mx = t[0];
#pragma unroll
    for (int j = 1; j < KT; ++j) mx = fmaxf(mx, t[j]);
    mx = row16_max(mx);
    const float shift = mx == -INFINITY ? 0.f : mx;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < KT; ++j) { e[j] = __expf(t[j] - shift); s += e[j]; }
    s = row16_sum(s);
    inv = s == 0.f ? 0.f : 1.0f / s;
    return shift + logf(s);
}

template <int D, int KT>
__global__ __launch_bounds__(SCORE_NW * WAVE) void score_kernel(ScoreArgs a) {
    using G = Geo<D>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, kk = lane >> 4;

    ScoreParams<D, KT> p;
    bool kvalid[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int k = t * 16 + i16;
        kvalid[t] = k < a.K;
        const float* src = a.pack + (kvalid[t] ? k : 0) * G::PACK;      // lanes beyond K: a readable row, never used
#pragma unroll
        for (int d = 0; d < D; ++d) p.m[t][d] = kvalid[t] ? src[d] : 0.f;
#pragma unroll
        for (int i = 0; i < G::TRI; ++i) p.W[t][i] = kvalid[t] ? src[D + i] : 0.f;
        p.c[t] = kvalid[t] ? src[D + G::TRI] : -INFINITY;
        p.h[t] = kvalid[t] ? src[D + G::TRI + 1] : 0.f;
        p.a[t] = kvalid[t] ? src[D + G::TRI + 2] : 0.f;
    }

    const long long g = (long long)blockIdx.x * SCORE_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    const bool vec = a.vec_ok != 0;
    double acc = 0.0;
    for (long long n8 = r0; n8 < r1; n8 += 8) {
        const long long na = n8 + kk, nb = n8 + 4 + kk;
        const bool va = na < r1, vb = nb < r1;
        float xa[D], xb[D];
        load_row<D>(a.x + (va ? na : r1 - 1) * D, xa, vec);              // rows past the range: a row of the range, discarded
        load_row<D>(a.x + (vb ? nb : r1 - 1) * D, xb, vec);
        float ta[KT], tb[KT], ea[KT], eb[KT], inva, invb;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const float sa = score_cell<D, KT>(p, t, xa), sb = score_cell<D, KT>(p, t, xb);
            ta[t] = kvalid[t] ? sa : -INFINITY;
            tb[t] = kvalid[t] ? sb : -INFINITY;
        }
        const float lpa = score_row<KT>(ta, ea, inva);
        const float lpb = score_row<KT>(tb, eb, invb);
        if (va) acc += (double)lpa;
        if (vb) acc += (double)lpb;
        if (a.logp && i16 < 2) {                                         // lanes (0, kk), (1, kk): 8 consecutive floats per wave
            if (i16 == 0 ? va : vb) a.logp[i16 == 0 ? na : nb] = i16 == 0 ? lpa : lpb;
        }
        if (a.resp) {
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const int k = t * 16 + i16;
                if (va && kvalid[t]) a.resp[na * a.K + k] = ea[t] * inva;
                if (vb && kvalid[t]) a.resp[nb * a.K + k] = eb[t] * invb;
            }
        }
    }
    if (a.partials) wave_block_sum<SCORE_NW>(acc, lane, wave, a.partials);
}

__global__ __launch_bounds__(WAVE) void score_sum_kernel(const double* partials, int nblk, double* out) { block_sum(partials, nblk, out); }

template <int D>
int launch_score(const ScoreArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(SCORE_NW * WAVE);
    switch ((a.K + 15) / 16) {
        case 1: hipLaunchKernelGGL((score_kernel<D, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((score_kernel<D, 2>), grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL((score_kernel<D, 3>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((score_kernel<D, 4>), grid, block, 0, s, a); break;
    }
    return check_launch("score_kernel");
}

}  // namespace

extern "C" {

int vmp_mix_score_pack_niw(int D, int K, const float* alpha, const float* beta, const float* m, const float* C, const float* v,
                           float* pack, void* stream) {
    int rc = stream_dims("vmp_mix_score_pack_niw", D, K);
    if (rc) return rc;
    if (!alpha || !beta || !m || !C || !v || !pack) { set_error("vmp_mix_score_pack_niw: null pointer"); return VMP_E_BADARG; }
    ScorePackArgs a{K, alpha, beta, m, C, v, pack};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((score_pack_niw_kernel<DD>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
        rc = check_launch("score_pack_niw_kernel");
    });
    return rc;
}

int vmp_mix_score_pack_t(int D, int K, const float* log_w, const float* mu, const float* sigma, const float* nu, float* pack,
                         void* stream) {
    int rc = stream_dims("vmp_mix_score_pack_t", D, K);
    if (rc) return rc;
    if (!log_w || !mu || !sigma || !nu || !pack) { set_error("vmp_mix_score_pack_t: null pointer"); return VMP_E_BADARG; }
    ScorePackArgs a{K, log_w, nullptr, mu, sigma, nu, pack};
    rc = -1;
    VMP_SWITCH_DIM(D, DD, {
        hipLaunchKernelGGL((score_pack_t_kernel<DD>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
        rc = check_launch("score_pack_t_kernel");
    });
    return rc;
}

size_t vmp_mix_score_workspace_bytes(int64_t N, int D, int K) {
    (void)D; (void)K;
    return (size_t)score_blocks(N) * sizeof(double);          // one fp64 partial per block
}

int vmp_mix_score(const float* x, int64_t N, int D, int K, const float* pack, float* logp_out, float* resp_out,
                  double* sum_out, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0) { set_error("vmp_mix_score: N must be positive (got %lld)", (long long)N); return VMP_E_BADARG; }
    int rc = stream_dims("vmp_mix_score", D, K);
    if (rc) return rc;
    if (!x || !pack) { set_error("vmp_mix_score: null pointer (%s)", !x ? "x" : "pack"); return VMP_E_BADARG; }
    if (!logp_out && !resp_out && !sum_out) { set_error("vmp_mix_score: no output requested"); return VMP_E_BADARG; }
    if ((rc = sum_workspace_check("vmp_mix_score", sum_out, ws, ws_bytes, vmp_mix_score_workspace_bytes(N, D, K))) != 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = score_blocks(N);
    const long long waves = (long long)blocks * SCORE_NW;
    ScoreArgs a{};
    a.x = x; a.pack = pack; a.logp = logp_out; a.resp = resp_out; a.partials = sum_out ? static_cast<double*>(ws) : nullptr;
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, waves, 8);
    a.vec_ok = aligned16(x);
    rc = -1;
    VMP_SWITCH_DIM(D, DD, rc = launch_score<DD>(a, blocks, s));
    if (rc || !sum_out) return rc;
    hipLaunchKernelGGL(score_sum_kernel, dim3(1), dim3(WAVE), 0, s, a.partials, blocks, sum_out);
    return check_launch("score_sum_kernel");
}

}  // extern "C"
