// Scalar tail of the SVAE ELBO and the optimiser update as single launches.
//
// At the reference's operating point (minibatches of 64-100 rows, experiments.py:26) a training step is bound by the NUMBER
// of launches.  Between the decoder kernel and the E-step backward kernel the step evaluates (reference svae.py:216-254,
// vae.py:232-250)
//     rec = -1/(2S) sum_nk r_nk A_nk - N Dy/2 log(2 pi),   reg = sum_nk r_nk (T'_nk + log z_nk),   elbo = rec - reg
// with r = exp(log z) and A_nk = sum_s ll_nks, and autograd runs the same chain backwards: ~24 elementwise / reduction
// launches of 2 us each for (N,K)-sized tensors.  elbo_tail_kernel produces r, the gradients of sigma * elbo w.r.t. log z
// and T' and per-block partial sums of the three scalars in one launch; elbo_final_kernel (one wave) adds the partials.  adam_kernel is tf.train.AdamOptimizer's update (TF 1.3:
// lr_t = lr sqrt(1-b2^t)/(1-b1^t); var -= lr_t m / (sqrt(v) + eps)) for ALL parameter tensors in one launch.
#include "vmp_common.h"
#include "vmp_tail.h"
#include "vmp_step_parts.h"
#include "vmp_prep_parts.h"

using namespace vmp;

namespace {

constexpr int TAIL_THREADS = 256;

__global__ __launch_bounds__(TAIL_THREADS) void elbo_tail_kernel(TailArgs a) { elbo_tail_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(WAVE) void elbo_final_kernel(TailArgs a, unsigned ntb) { elbo_final_body(a, ntb); }

// ---- Adam ------------------------------------------------------------------------------------------------------------
constexpr int ADAM_MAX_TENSORS = 32;
constexpr int ADAM_CHUNK = 1024;       // elements per block
constexpr int ADAM_THREADS = 256;

struct AdamArgs {
    float* p[ADAM_MAX_TENSORS];
    const float* g[ADAM_MAX_TENSORS];
    float* m[ADAM_MAX_TENSORS];
    float* v[ADAM_MAX_TENSORS];
    unsigned n[ADAM_MAX_TENSORS];
    unsigned end_block[ADAM_MAX_TENSORS];   // inclusive prefix sums of ceil(n / ADAM_CHUNK)
    const float* lr_t_dev;
    float lr_t, b1, b2, c1, c2, eps;   // c = 1 - b, rounded from the fp64 difference
    int nt;
};

__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(AdamArgs a) {
    int t = 0;
    while (t < a.nt - 1 && blockIdx.x >= a.end_block[t]) ++t;
    const unsigned first = t ? a.end_block[t - 1] : 0u;
    const unsigned base = (blockIdx.x - first) * ADAM_CHUNK;
    const float lr_t = a.lr_t_dev ? *a.lr_t_dev : a.lr_t;
    const float c1 = a.c1, c2 = a.c2;
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    const unsigned n = a.n[t];
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / ADAM_THREADS; ++j) {
        const unsigned i = base + j * ADAM_THREADS + threadIdx.x;
        if (i >= n) break;
        adam_update(p, m, v, i, g[i], lr_t, a.b1, a.b2, c1, c2, a.eps);
    }
}

// ---- data-parallel step: one packed fp64 buffer [moments | all gradients | scalars] ------------------------------------
// (the reference gathers per-tower gradients and averages them tensor by tensor, experiments.py:247-260 / tf_utils.py:52-87;
//  here every rank packs once, ONE all-reduce sums the buffer, and Adam reads the averaged gradients straight from it)
struct PackArgs {
    const void* src[ADAM_MAX_TENSORS];
    unsigned n[ADAM_MAX_TENSORS];
    unsigned off[ADAM_MAX_TENSORS];         // element offset in dst
    unsigned end_block[ADAM_MAX_TENSORS];
    unsigned f64mask;                        // bit t: src[t] holds doubles (else floats)
    double* dst;
    int nt;
};
__global__ __launch_bounds__(ADAM_THREADS) void pack_f64_kernel(PackArgs a) {
    int t = 0;
    while (t < a.nt - 1 && blockIdx.x >= a.end_block[t]) ++t;
    const unsigned first = t ? a.end_block[t - 1] : 0u;
    const unsigned base = (blockIdx.x - first) * ADAM_CHUNK;
    const unsigned n = a.n[t];
    double* __restrict__ d = a.dst + a.off[t];
    const bool f64 = (a.f64mask >> t) & 1u;
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / ADAM_THREADS; ++j) {
        const unsigned i = base + j * ADAM_THREADS + threadIdx.x;
        if (i >= n) break;
        d[i] = f64 ? static_cast<const double*>(a.src[t])[i] : (double)static_cast<const float*>(a.src[t])[i];
    }
}

struct AdamPackedArgs {
    float* p[ADAM_MAX_TENSORS];
    float* gout[ADAM_MAX_TENSORS];          // nullable: the averaged gradient is also written here (fp32)
    float* m[ADAM_MAX_TENSORS];
    float* v[ADAM_MAX_TENSORS];
    unsigned n[ADAM_MAX_TENSORS];
    unsigned off[ADAM_MAX_TENSORS];         // element offset of the tensor's gradient in gbuf
    unsigned end_block[ADAM_MAX_TENSORS];
    const double* gbuf;
    const float* lr_t_dev;
    double gscale;
    float lr_t, b1, b2, c1, c2, eps;
    int nt;
};
__global__ __launch_bounds__(ADAM_THREADS) void adam_packed_kernel(AdamPackedArgs a) {
    int t = 0;
    while (t < a.nt - 1 && blockIdx.x >= a.end_block[t]) ++t;
    const unsigned first = t ? a.end_block[t - 1] : 0u;
    const unsigned base = (blockIdx.x - first) * ADAM_CHUNK;
    const float lr_t = a.lr_t_dev ? *a.lr_t_dev : a.lr_t;
    const float c1 = a.c1, c2 = a.c2;
    float* __restrict__ p = a.p[t];
    const double* __restrict__ g = a.gbuf + a.off[t];
    float* __restrict__ go = a.gout[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    const unsigned n = a.n[t];
#pragma unroll
    for (int j = 0; j < ADAM_CHUNK / ADAM_THREADS; ++j) {
        const unsigned i = base + j * ADAM_THREADS + threadIdx.x;
        if (i >= n) break;
        const float gi = (float)(g[i] * a.gscale);          // mean over the ranks in fp64, rounded once (tf_utils.py:79)
        if (go) go[i] = gi;
        adam_update(p, m, v, i, gi, lr_t, a.b1, a.b2, c1, c2, a.eps);
    }
}

// [Philox key | CVI step size | Adam step size] of a graph-captured training step: the values travel in the launch packet
// (by value), so the caller needs no staging buffer that an asynchronous copy could still be reading when it is rewritten.
struct Words16 { unsigned long long key; float rho, lr_t; };
__global__ void step_scalars_kernel(Words16* dst, Words16 v) { *dst = v; }
// the same, and the minibatch copied into the captured step's static input by the same launch (round 6: one eager launch per replay, not two)
constexpr int INPUT_THREADS = 256;
__global__ __launch_bounds__(INPUT_THREADS) void step_inputs_kernel(Words16* dst, Words16 v, const float* __restrict__ src, float* __restrict__ y,
                                                                    unsigned n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = v;
    for (unsigned i = blockIdx.x * INPUT_THREADS + threadIdx.x; i < n; i += gridDim.x * INPUT_THREADS) y[i] = src[i];
}

// ---- the closing launch of the minibatch training step (round 6) -------------------------------------------------------------
// Everything that waits for the encoder's backward kernel and for nothing else, as ONE grid whose blocks take roles:
//   [decoder net | encoder net]  64 parameters per block: reduce the fused MLP backward kernel's per-block partials (dec_reduce_sum:
//                                the order of dec_reduce_kernel), store the gradient, apply Adam to the 64 parameters
//   [K blocks]                   phi_gmm: component k's rows of the E-step backward kernel's partials summed, the backward of the
//                                recognition unpacking on them, Adam on component k's elements (phi_prep_body<L, true, true>)
//   [K blocks]                   M-step moments of the minibatch + CVI update of theta_k (stats_cvi_body: vmp_svae_stats_cvi)
//   [1 block]                    the three ELBO scalars from the per-tile sums of vmp_svae_estep_bwd_tail (elbo_final_body)
// It replaces dec_reduce_tail_kernel's reduce blocks, svae_bwd_reduce_kernel, phi_prep_kernel<L, true>, dec_reduce_kernel,
// stats_cvi_kernel and adam_kernel: 6 launches -> 1.
// theta and the parameters are only written here; every role reads what the step's earlier launches left (experiments.py:267: the
// CVI update and the Adam step both read OLD values).
constexpr int FIN_THREADS = 64 * DEC_RED_GROUPS;
constexpr int FIN_NET_TENSORS = 9;
static_assert(FIN_THREADS == 64 * RED_GROUPS, "the phi role's reduction uses the block shape of svae_bwd_reduce_kernel");
struct FinNet {
    DecRedArgs red;                          // (out unused)
    float* p[FIN_NET_TENSORS];
    float* m[FIN_NET_TENSORS];
    float* v[FIN_NET_TENSORS];
    float* g[FIN_NET_TENSORS];               // reduced gradients out
    int off[FIN_NET_TENSORS + 1];            // flat offsets of the tensors inside a partial row
    int nb;                                  // blocks
};
// SMM-SVAE (vmp_svae_step_final_smm / vmp_svae_step_pack_smm): the K moment / CVI blocks become the theta blocks of the Student-t
// model - block k sums the THETA half of component k's partial rows (vmp_svae_bwd_reduce's order), differentiates the Student-t theta
// packing (svae._theta_pack: m = mu_k, W = L_k^-1, kappa's -sum log diag L_k, tril / softplus), applies Adam to theta/mu_k and
// theta/L_k, and does the SMM M-step: N_k = sum_n r_nk (fp64), alpha* = prior + N_k and the CVI update of alpha (svae.py:179-196,
// experiments.py:252-256).
struct SmmFin {
    float* p[2];                             // theta/mu_k (K,L), theta/L_k raw (K,L,L)
    float* m[2];                             // Adam slots (NULL: data-parallel form, no update)
    float* v[2];
    float* g[2];                             // gradients out (fp32)
    double* gx[2];                           // data-parallel form: the gradients as doubles into the exchange buffer
    const float* r;                          // (N,K) exp(log z) of vmp_svae_estep_bwd_tail_t
    int N;
    const float* prior_alpha;                // (K) natural Dirichlet prior
    float* alpha;                            // (K) theta[0], updated in place (NULL: N_k only)
    float* alpha_star;                       // (K) may be NULL
    const float* rho_dev;
    float rho;
    double* nk;                              // (K) N_k out
};
struct FinArgs {
    FinNet net[2];
    PhiArgs phi;                             // (backward form: mu, Lraw, piraw, logpi in; g_mu, g_Lraw, g_piraw out)
    PhiAdam phi_adam;
    const float* partials;                   // (nblk, K, 2 (L + TRI + 1)) of the E-step backward kernel
    int nblk;
    SmallStatsArgs sa;
    CviArgs cvi;
    TailArgs tail;
    unsigned tail_n;
    const float* lr_t_dev;
    float lr_t, b1, b2, c1, c2, eps;
    // data-parallel form (vmp_svae_step_pack): nothing is updated - moments, gradients and scalars go, as doubles, into the packed
    // exchange buffer [moments | gradients in parameter order | elbo, rec, reg] that the step's ONE all-reduce sums
    double* xnet[2];                         // where the two nets' gradients start in the buffer (NULL: the single-process form)
    double* xscal;
    SmmFin smm;                              // (step_final_kernel<L, true> only)
};

template <int L>
__device__ __forceinline__ void smm_theta_final_body(const FinArgs& a, const int k, double (*part)[64], const float lr_t) {
    constexpr int TRI = L * (L + 1) / 2, TH = L + TRI + 1, PW = 2 * TH;
    static_assert(TH <= 64 && L * L <= 64, "one lane per partial word / matrix element");
    const SmmFin& q = a.smm;
    const int K = a.phi.K, tid = threadIdx.x, eg = tid & 63, bg = tid >> 6;
    __shared__ double nkw[FIN_THREADS / WAVE];
    __shared__ double Ls[L][L + 1], Wm[L][L + 1], Gw[L][L + 1], Am[L][L + 1], inv_d[L];
    __shared__ double gkap;
    __shared__ float gms[L];
    part[bg][eg] = eg < TH ? red_group_sum(a.partials + (size_t)k * PW + TH + eg, (size_t)K * PW, a.nblk, bg) : 0.0;
    double rv = tid < q.N ? (double)q.r[(size_t)tid * K + k] : 0.0;        // N <= SMALL_STATS_MAX_N <= FIN_THREADS rows
    rv = wave_sum_d(rv);
    if (eg == 0) nkw[bg] = rv;
    __syncthreads();
    if (tid >= WAVE) return;
    const int lane = tid, i = lane / L, j = lane % L;
    const bool in = lane < L * L;
    double s = part[0][lane];
    for (int g2 = 1; g2 < RED_GROUPS; ++g2) s += part[g2][lane];
    const float v = (float)s;                                               // rounded as vmp_svae_bwd_reduce's tensors
    if (lane < L) gms[lane] = v;
    else if (lane < L + TRI) {
        const int idx = lane - L;
        int ii = 0;
        while ((ii + 1) * (ii + 2) / 2 <= idx) ++ii;
        Gw[ii][idx - ii * (ii + 1) / 2] = (double)v;
    } else if (lane == L + TRI) gkap = (double)v;
    const float* raw = q.p[1] + (size_t)k * L * L;           // (no restrict: Adam writes these elements below)
    double rawd = 0.0, lij = 0.0;
    if (in) {
        rawd = (double)raw[i * L + j];
        lij = j < i ? rawd : (j == i ? (double)(float)softplus_d(rawd) : 0.0);
        Ls[i][j] = lij;
        if (i == j) inv_d[i] = 1.0 / lij;
        if (j > i) Gw[i][j] = 0.0;                           // W is lower: no gradient above the diagonal
    }
    prep_sync<true>();
    if (lane < L) {                                          // W = L_k^-1, lane c: column c
        const int c = lane;
        double w[L];
#pragma unroll
        for (int r = 0; r < L; ++r) {
            double t = r == c ? 1.0 : 0.0;
#pragma unroll
            for (int p = 0; p < r; ++p) t -= Ls[r][p] * w[p];
            w[r] = r < c ? 0.0 : t * inv_d[r];
            Wm[r][c] = w[r];
        }
    }
    prep_sync<true>();
    if (in) {                                                // A = W^T G_W
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < L; ++p) t += p >= i ? Wm[p][i] * Gw[p][j] : 0.0;
        Am[i][j] = t;
    }
    prep_sync<true>();
    const float rho = q.rho_dev ? *q.rho_dev : q.rho;
    if (in) {
        // d/dL_k of W = L_k^-1: -W^T G_W W^T (lower part); kappa has -log L_ii; then the softplus of the diagonal (tril: 0 above)
        double g = 0.0;
        if (j <= i) {
#pragma unroll
            for (int p = 0; p < L; ++p) g -= p <= j ? Am[i][p] * Wm[j][p] : 0.0;
            if (i == j) {
                g -= gkap * inv_d[i];
                g *= 1.0 / (1.0 + exp(-rawd));               // softplus'
            }
        }
        const float gf = (float)g;
        const unsigned e = (unsigned)(k * L * L + lane);
        q.g[1][e] = gf;
        if (q.gx[1]) q.gx[1][e] = (double)gf;
        if (q.m[1]) adam_update(q.p[1], q.m[1], q.v[1], e, gf, lr_t, a.b1, a.b2, a.c1, a.c2, a.eps);
    }
    if (lane < L) {                                          // m = mu_k
        const float gf = gms[lane];
        const unsigned e = (unsigned)(k * L + lane);
        q.g[0][e] = gf;
        if (q.gx[0]) q.gx[0][e] = (double)gf;
        if (q.m[0]) adam_update(q.p[0], q.m[0], q.v[0], e, gf, lr_t, a.b1, a.b2, a.c1, a.c2, a.eps);
    }
    if (lane == 0) {
        double nk = 0.0;
        for (int w = 0; w < FIN_THREADS / WAVE; ++w) nk += nkw[w];
        q.nk[k] = nk;
        if (q.alpha) cvi_one(q.alpha, q.alpha_star, q.prior_alpha[k] + (float)nk, rho, (size_t)k);
    }
}
template <int L, bool SMM = false>
__global__ __launch_bounds__(FIN_THREADS) void step_final_kernel(FinArgs a) {
    __shared__ double part[DEC_RED_GROUPS][64];
    __shared__ double spart[SMALL_STATS_GROUPS][80];
    __shared__ double st[80];
    static_assert(SMALL_STATS_GROUPS * 80 <= FIN_THREADS, "the moment role needs 12 x 80 threads");
    const float lr_t = a.lr_t_dev ? *a.lr_t_dev : a.lr_t;
    int b = blockIdx.x;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const FinNet& q = a.net[n];
        if (b < q.nb) {
            const double s = dec_reduce_sum(q.red, b, part);
            const int i = b * 64 + (threadIdx.x & 63);
            if ((threadIdx.x >> 6) == 0 && i < q.red.PW) {
                int t = 0;
                while (t < FIN_NET_TENSORS - 1 && i >= q.off[t + 1]) ++t;
                const unsigned j = (unsigned)(i - q.off[t]);
                const float gi = (float)s;
                q.g[t][j] = gi;
                if (a.xnet[n]) a.xnet[n][i] = (double)gi;
                else adam_update(q.p[t], q.m[t], q.v[t], j, gi, lr_t, a.b1, a.b2, a.c1, a.c2, a.eps);
            }
            return;
        }
        b -= q.nb;
    }
    if (b < a.phi.K) {
        PhiAdam ad = a.phi_adam;
        ad.lr_t = lr_t;
        phi_prep_body<L, true, true>(a.phi, b, a.partials, a.nblk, &ad);
        return;
    }
    b -= a.phi.K;
    if constexpr (SMM) {
        if (b < a.phi.K) {
            smm_theta_final_body<L>(a, b, part, lr_t);
            return;
        }
        b -= a.phi.K;
    } else {
        if (b < a.cvi.K) {
            stats_cvi_body(a.sa, a.cvi, b, spart, st, a.xscal == nullptr);
            return;
        }
    }
    if (threadIdx.x < WAVE) {
        elbo_final_body(a.tail, a.tail_n);
        if (threadIdx.x == 0 && a.xscal) {
#pragma unroll
            for (int i = 0; i < 3; ++i) a.xscal[i] = (double)a.tail.scal[i];       // (this thread wrote them: program order)
        }
    }
}

// ---- host side of the closing launch ------------------------------------------------------------------------------
// One closing launch, described by name: the four entry points below fill this and call step_final_launch.  `pack` (data-parallel
// form: nothing is updated; moments, gradients and scalars go into xbuf) and `smm` (Student-t theta) say which form it is.  A field
// that the form does not use stays NULL and never reaches FinArgs.
struct FinSpec {
    const char* what;
    bool pack, smm;
    struct Tensors { float* const* p; float* const* g; float* const* m; float* const* v; };   // values, gradients out; Adam's slots: !pack
    struct Net {
        const float* part;                   // per-block partial rows of the fused MLP backward kernel
        int blocks, in, units, out;
        Tensors w;                           // 9 tensors, the reference's variable order
    } net[2];                                // decoder, encoder
    Tensors phi;                             // phi_gmm/mu_k (K,L), L_k (K,L,L), log_pi_k (K)
    const float* partials; int nblk; const double* logpi;      // partial rows of the E-step backward kernel, the forward pass's log pi
    const float* x_samples;                  // (!smm)
    const float* const* prior;               // (!smm, !pack) 5 tensors
    float* const* theta;                     // (!smm, !pack) 5 tensors
    float* const* theta_star;                // (!smm, !pack) may be NULL
    Tensors th;                              // (smm) theta/mu_k (K,L), theta/L_k (K,L,L)
    const float* prior_alpha; float* alpha;  // (smm, !pack)
    float* alpha_star;                       // (smm, !pack) may be NULL
    const float* r; int64_t N; int K, L;
    const float* rho_dev; float rho;         // CVI step size: device word, or by value
    double* stats_out;                       // (!pack)
    const double* tail_part; int tail_n, Dy; float* scalars;
    double beta1, beta2, eps, lr_t; const float* lr_t_dev;
    double* xbuf; size_t xbuf_doubles;       // (pack)
    void* stream;
};

// The fp64 exchange buffer of a data-parallel step, offsets in doubles: [moments (K, 2+L+L*L; SMM: N_k (K, 1)) | phi_gmm/mu_k, L_k,
// log_pi_k | SMM: theta/mu_k, theta/L_k | encoder net | decoder net | elbo, rec, reg] - the parameter order of
// SVAETrainer.trainables() (experiments.py:160-181), as training.exchange_layout lays it out.
struct XLayout { size_t phi[3], theta[2], net[2], scal, total; };       // (net: decoder, encoder - the order of FinArgs)
XLayout exchange_layout(int K, int L, int enc_words, int dec_words, bool smm) {
    XLayout x{};
    const size_t KL = (size_t)K * L;
    size_t o = smm ? (size_t)K : (size_t)K * (2 + L + L * L);
    x.phi[0] = o; o += KL;
    x.phi[1] = o; o += KL * L;
    x.phi[2] = o; o += K;
    if (smm) {
        x.theta[0] = o; o += KL;
        x.theta[1] = o; o += KL * L;
    }
    x.net[1] = o; o += enc_words;
    x.net[0] = o; o += dec_words;
    x.scal = o;
    x.total = o + 3;
    return x;
}

template <bool SMM>
void step_final_dispatch(int L, unsigned blocks, void* stream, const FinArgs& a) {
    VMP_SWITCH_DIM(L, LL, hipLaunchKernelGGL((step_final_kernel<LL, SMM>), dim3(blocks), dim3(FIN_THREADS), 0, static_cast<hipStream_t>(stream), a));
}

template <class T>
bool all_set(T* const* a, int n) {           // the array and its n pointers
    for (int t = 0; a && t < n; ++t)
        if (!a[t]) return false;
    return a != nullptr;
}
bool tensors_set(const FinSpec::Tensors& w, int n, bool adam) {
    return all_set(w.p, n) && all_set(w.g, n) && (!adam || (all_set(w.m, n) && all_set(w.v, n)));
}

int step_final_launch(const FinSpec& s) {
    const bool upd = !s.pack;
    const int K = s.K, L = s.L;
    // pointers first, by what the form reads, then sizes: nothing is launched before both have passed
    bool ok = s.partials && s.nblk >= 1 && s.logpi && s.r && s.tail_part && s.scalars && tensors_set(s.phi, 3, upd);
    for (const FinSpec::Net& n : s.net) ok = ok && n.part && n.blocks >= 1 && tensors_set(n.w, FIN_NET_TENSORS, upd);
    ok = ok && (s.pack ? s.xbuf != nullptr : s.stats_out != nullptr);
    if (s.smm) ok = ok && tensors_set(s.th, 2, upd) && (s.pack || (s.prior_alpha && s.alpha));
    else ok = ok && s.x_samples && (s.pack || (all_set(s.prior, 5) && all_set(s.theta, 5)));
    if (!ok) {
        set_error("%s: NULL argument", s.what);
        return VMP_E_BADARG;
    }
    if (K < 1 || K > VMP_MAX_K || L < 1 || L > VMP_MAX_D || s.N < 1 || s.N > SMALL_STATS_MAX_N || s.tail_n < 1 || s.tail_n > TAIL_MAX_BLOCKS ||
        s.Dy < 1) {
        set_error("%s: K=%d L=%d N=%lld tail_n=%d outside the minibatch step's range (N <= %d)", s.what, K, L, (long long)s.N, s.tail_n,
                  SMALL_STATS_MAX_N);
        return VMP_E_DIM;
    }
    FinArgs a{};
    for (int n = 0; n < 2; ++n) {
        const FinSpec::Net& w = s.net[n];
        const int Li = w.in, U = w.units, Do = w.out;
        if (Li < 1 || Li > 8 || Do < 1 || Do > 8 || U < 1 || U > 64) {
            set_error("%s: net %d sizes in=%d units=%d out=%d outside the fused MLP's range", s.what, n, Li, U, Do);
            return VMP_E_DIM;
        }
        const int sizes[FIN_NET_TENSORS] = {Li * U, U, U * U, U, U * 2 * Do, 2 * Do, Li * Do, Do, Do};   // the reference's variable order
        FinNet& q = a.net[n];
        int o = 0;
        for (int t = 0; t < FIN_NET_TENSORS; ++t) {
            q.p[t] = w.w.p[t]; q.g[t] = w.w.g[t];
            if (upd) { q.m[t] = w.w.m[t]; q.v[t] = w.w.v[t]; }
            q.off[t] = o;
            o += sizes[t];
        }
        q.off[FIN_NET_TENSORS] = o;
        if (o != vmp_decoder_param_words(Li, U, Do)) {
            set_error("%s: parameter layout mismatch (%d != %d words)", s.what, o, vmp_decoder_param_words(Li, U, Do));
            return VMP_E_DIM;
        }
        q.red = DecRedArgs{w.part, q.p[FIN_NET_TENSORS - 1], nullptr, w.blocks, o, o - Do, Do};
        q.nb = (o + 63) / 64;
    }
    const XLayout x = exchange_layout(K, L, a.net[1].red.PW, a.net[0].red.PW, s.smm);
    if (s.pack && s.xbuf_doubles < x.total) {
        set_error("%s: exchange buffer too small (%zu < %zu doubles)", s.what, s.xbuf_doubles, x.total);
        return VMP_E_WS;
    }
    for (int t = 0; t < 3; ++t) {
        if (upd) { a.phi_adam.p[t] = s.phi.p[t]; a.phi_adam.m[t] = s.phi.m[t]; a.phi_adam.v[t] = s.phi.v[t]; }
        else a.phi_adam.gx[t] = s.xbuf + x.phi[t];
    }
    if (s.pack) {
        for (int n = 0; n < 2; ++n) a.xnet[n] = s.xbuf + x.net[n];
        a.xscal = s.xbuf + x.scal;
    }
    a.phi.mu = s.phi.p[0]; a.phi.Lraw = s.phi.p[1]; a.phi.piraw = s.phi.p[2]; a.phi.logpi = s.logpi;
    a.phi.g_mu = s.phi.g[0]; a.phi.g_Lraw = s.phi.g[1]; a.phi.g_piraw = s.phi.g[2]; a.phi.K = K; a.phi.L = L;
    a.partials = s.partials; a.nblk = s.nblk;
    double* const moments = s.pack ? s.xbuf : s.stats_out;  // (the exchange buffer starts with them)
    if (s.smm) {
        SmmFin& q = a.smm;
        for (int t = 0; t < 2; ++t) {
            q.p[t] = s.th.p[t]; q.g[t] = s.th.g[t];
            if (upd) { q.m[t] = s.th.m[t]; q.v[t] = s.th.v[t]; }
            else q.gx[t] = s.xbuf + x.theta[t];
        }
        if (upd) { q.prior_alpha = s.prior_alpha; q.alpha = s.alpha; q.alpha_star = s.alpha_star; }
        q.r = s.r; q.N = (int)s.N; q.nk = moments;
        q.rho_dev = s.rho_dev; q.rho = s.rho;
    } else {
        a.sa = SmallStatsArgs{s.x_samples, s.r, nullptr, moments, (int)s.N, L, K};
        a.cvi.K = K; a.cvi.L = L;
        if (upd) {
            const float* const* pr = s.prior;
            float* const* th = s.theta;
            float* const* ts = s.theta_star;
            a.cvi = CviArgs{moments, pr[0], pr[1], pr[2], pr[3], pr[4], th[0], th[1], th[2], th[3], th[4], ts ? ts[0] : nullptr,
                            ts ? ts[1] : nullptr, ts ? ts[2] : nullptr, ts ? ts[3] : nullptr, ts ? ts[4] : nullptr, s.rho_dev, s.rho, K, L};
        }
    }
    a.tail.part = const_cast<double*>(s.tail_part);
    a.tail.scal = s.scalars;
    a.tail.cst = (double)s.N * s.Dy * 0.5 * 1.8378770664093453;        // log(2 pi): as tail_setup
    a.tail_n = (unsigned)s.tail_n;
    a.lr_t_dev = s.lr_t_dev; a.lr_t = (float)s.lr_t; a.b1 = (float)s.beta1; a.b2 = (float)s.beta2;
    a.c1 = (float)(1.0 - s.beta1); a.c2 = (float)(1.0 - s.beta2); a.eps = (float)s.eps;
    a.phi_adam.b1 = a.b1; a.phi_adam.b2 = a.b2; a.phi_adam.c1 = a.c1; a.phi_adam.c2 = a.c2; a.phi_adam.eps = a.eps;
    const unsigned blocks = (unsigned)(a.net[0].nb + a.net[1].nb + 2 * K + 1);     // the roles of step_final_kernel, in its order
    if (s.smm) step_final_dispatch<true>(L, blocks, s.stream, a);
    else step_final_dispatch<false>(L, blocks, s.stream, a);
    return check_launch(s.what);
}
}  // namespace

extern "C" {

int vmp_svae_step_scalars(void* dst16, uint64_t philox_key, float cvi_step, float adam_step, void* stream) {
    if (!dst16 || (reinterpret_cast<uintptr_t>(dst16) & 7)) {
        set_error("vmp_svae_step_scalars: dst16 must be an 8-byte aligned device pointer to 16 bytes");
        return VMP_E_BADARG;
    }
    hipLaunchKernelGGL(step_scalars_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), static_cast<Words16*>(dst16),
                       Words16{(unsigned long long)philox_key, cvi_step, adam_step});
    return check_launch("vmp_svae_step_scalars");
}

int vmp_svae_step_inputs(void* dst16, uint64_t philox_key, float cvi_step, float adam_step, const float* y_src, float* y_dst,
                         int64_t n_floats, void* stream) {
    if (!dst16 || (reinterpret_cast<uintptr_t>(dst16) & 7)) {
        set_error("vmp_svae_step_inputs: dst16 must be an 8-byte aligned device pointer to 16 bytes");
        return VMP_E_BADARG;
    }
    if (n_floats < 0 || n_floats >= 4294967296LL || (n_floats > 0 && (!y_src || !y_dst))) {
        set_error("vmp_svae_step_inputs: bad minibatch copy (n = %lld)", (long long)n_floats);
        return VMP_E_BADARG;
    }
    long long blocks = (n_floats + INPUT_THREADS - 1) / INPUT_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(step_inputs_kernel, dim3((unsigned)blocks), dim3(INPUT_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<Words16*>(dst16), Words16{(unsigned long long)philox_key, cvi_step, adam_step}, y_src, y_dst,
                       (unsigned)n_floats);
    return check_launch("vmp_svae_step_inputs");
}

int vmp_svae_step_final(const float* dec_part, int dec_blocks, int dec_in, int dec_units, int dec_out, float* const* dec_p,
                        float* const* dec_m, float* const* dec_v, float* const* dec_g, const float* enc_part, int enc_blocks,
                        int enc_in, int enc_units, int enc_out, float* const* enc_p, float* const* enc_m, float* const* enc_v,
                        float* const* enc_g, const float* partials, int nblk, const double* logpi, float* const* phi_p,
                        float* const* phi_g, float* const* phi_m, float* const* phi_v, const float* x_samples, const float* r, int64_t N,
                        const float* const* prior, float* const* theta, float* const* theta_star, const float* rho_dev, float rho, int K,
                        int L, double* stats_out, const double* tail_part, int tail_n, int Dy, float* scalars, double beta1, double beta2,
                        double eps, double lr_t, const float* lr_t_dev, void* stream) {
    return step_final_launch(FinSpec{
        .what = "vmp_svae_step_final",
        .net = {{dec_part, dec_blocks, dec_in, dec_units, dec_out, {.p = dec_p, .g = dec_g, .m = dec_m, .v = dec_v}},
                {enc_part, enc_blocks, enc_in, enc_units, enc_out, {.p = enc_p, .g = enc_g, .m = enc_m, .v = enc_v}}},
        .phi = {.p = phi_p, .g = phi_g, .m = phi_m, .v = phi_v}, .partials = partials, .nblk = nblk, .logpi = logpi,
        .x_samples = x_samples, .prior = prior, .theta = theta, .theta_star = theta_star,
        .r = r, .N = N, .K = K, .L = L, .rho_dev = rho_dev, .rho = rho, .stats_out = stats_out,
        .tail_part = tail_part, .tail_n = tail_n, .Dy = Dy, .scalars = scalars,
        .beta1 = beta1, .beta2 = beta2, .eps = eps, .lr_t = lr_t, .lr_t_dev = lr_t_dev, .stream = stream});
}

// The closing launch of a DATA-PARALLEL minibatch step: the same block roles, but nothing is updated - this rank's moments, its 21
// gradients and its three scalars go as doubles into xbuf (exchange_layout above), the packed buffer the step's one all-reduce sums
// (experiments.py:247-260); vmp_svae_cvi_update and vmp_adam_step_packed follow the all-reduce.  The fp32 gradients are also left in *_g.
int vmp_svae_step_pack(double* xbuf, size_t xbuf_doubles, const float* dec_part, int dec_blocks, int dec_in, int dec_units, int dec_out,
                       float* const* dec_p, float* const* dec_g, const float* enc_part, int enc_blocks, int enc_in, int enc_units,
                       int enc_out, float* const* enc_p, float* const* enc_g, const float* partials, int nblk, const double* logpi,
                       float* const* phi_p, float* const* phi_g, const float* x_samples, const float* r, int64_t N, int K, int L,
                       const double* tail_part, int tail_n, int Dy, float* scalars, void* stream) {
    return step_final_launch(FinSpec{
        .what = "vmp_svae_step_pack", .pack = true,
        .net = {{dec_part, dec_blocks, dec_in, dec_units, dec_out, {.p = dec_p, .g = dec_g}},
                {enc_part, enc_blocks, enc_in, enc_units, enc_out, {.p = enc_p, .g = enc_g}}},
        .phi = {.p = phi_p, .g = phi_g}, .partials = partials, .nblk = nblk, .logpi = logpi,
        .x_samples = x_samples,
        .r = r, .N = N, .K = K, .L = L,
        .tail_part = tail_part, .tail_n = tail_n, .Dy = Dy, .scalars = scalars,
        .xbuf = xbuf, .xbuf_doubles = xbuf_doubles, .stream = stream});
}

// The closing launch of the SMM-SVAE's minibatch step: vmp_svae_step_final's roles with the Student-t model's theta (see SmmFin):
// Adam on the 23 tensors of SVAETrainer.trainables() (phi_gmm (3), theta/mu_k, theta/L_k, encoder (9), decoder (9)), the N_k-only
// M-step and the CVI update of alpha; stats_out (K, 1) fp64 = N_k.  partials: vmp_svae_estep_bwd_tail_t's (theta half included).
int vmp_svae_step_final_smm(const float* dec_part, int dec_blocks, int dec_in, int dec_units, int dec_out, float* const* dec_p,
                            float* const* dec_m, float* const* dec_v, float* const* dec_g, const float* enc_part, int enc_blocks,
                            int enc_in, int enc_units, int enc_out, float* const* enc_p, float* const* enc_m, float* const* enc_v,
                            float* const* enc_g, const float* partials, int nblk, const double* logpi, float* const* phi_p,
                            float* const* phi_g, float* const* phi_m, float* const* phi_v, float* const* theta_p, float* const* theta_g,
                            float* const* theta_m, float* const* theta_v, const float* r, int64_t N, const float* prior_alpha,
                            float* alpha, float* alpha_star, const float* rho_dev, float rho, int K, int L, double* stats_out,
                            const double* tail_part, int tail_n, int Dy, float* scalars, double beta1, double beta2, double eps,
                            double lr_t, const float* lr_t_dev, void* stream) {
    return step_final_launch(FinSpec{
        .what = "vmp_svae_step_final_smm", .smm = true,
        .net = {{dec_part, dec_blocks, dec_in, dec_units, dec_out, {.p = dec_p, .g = dec_g, .m = dec_m, .v = dec_v}},
                {enc_part, enc_blocks, enc_in, enc_units, enc_out, {.p = enc_p, .g = enc_g, .m = enc_m, .v = enc_v}}},
        .phi = {.p = phi_p, .g = phi_g, .m = phi_m, .v = phi_v}, .partials = partials, .nblk = nblk, .logpi = logpi,
        .th = {.p = theta_p, .g = theta_g, .m = theta_m, .v = theta_v}, .prior_alpha = prior_alpha, .alpha = alpha, .alpha_star = alpha_star,
        .r = r, .N = N, .K = K, .L = L, .rho_dev = rho_dev, .rho = rho, .stats_out = stats_out,
        .tail_part = tail_part, .tail_n = tail_n, .Dy = Dy, .scalars = scalars,
        .beta1 = beta1, .beta2 = beta2, .eps = eps, .lr_t = lr_t, .lr_t_dev = lr_t_dev, .stream = stream});
}

// Data-parallel form of vmp_svae_step_final_smm: xbuf as exchange_layout above gives it for the SMM step; nothing is updated.
int vmp_svae_step_pack_smm(double* xbuf, size_t xbuf_doubles, const float* dec_part, int dec_blocks, int dec_in, int dec_units,
                           int dec_out, float* const* dec_p, float* const* dec_g, const float* enc_part, int enc_blocks, int enc_in,
                           int enc_units, int enc_out, float* const* enc_p, float* const* enc_g, const float* partials, int nblk,
                           const double* logpi, float* const* phi_p, float* const* phi_g, float* const* theta_p, float* const* theta_g,
                           const float* r, int64_t N, int K, int L, const double* tail_part, int tail_n, int Dy, float* scalars,
                           void* stream) {
    return step_final_launch(FinSpec{
        .what = "vmp_svae_step_pack_smm", .pack = true, .smm = true,
        .net = {{dec_part, dec_blocks, dec_in, dec_units, dec_out, {.p = dec_p, .g = dec_g}},
                {enc_part, enc_blocks, enc_in, enc_units, enc_out, {.p = enc_p, .g = enc_g}}},
        .phi = {.p = phi_p, .g = phi_g}, .partials = partials, .nblk = nblk, .logpi = logpi,
        .th = {.p = theta_p, .g = theta_g},
        .r = r, .N = N, .K = K, .L = L,
        .tail_part = tail_part, .tail_n = tail_n, .Dy = Dy, .scalars = scalars,
        .xbuf = xbuf, .xbuf_doubles = xbuf_doubles, .stream = stream});
}

size_t vmp_svae_elbo_tail_workspace_bytes(void) { return tail_workspace_bytes(); }

int vmp_svae_elbo_tail(const float* log_z, const float* T_prime, const float* ll, int64_t N, int K, int S, int Dy, float sigma,
                       float* scalars, float* g_log_z, float* g_T_prime, float* r, void* ws, size_t ws_bytes, void* stream) {
    if (N < 0 || K < 1 || S < 1 || Dy < 1) {
        set_error("vmp_svae_elbo_tail: bad sizes N=%lld K=%d S=%d Dy=%d", (long long)N, K, S, Dy);
        return VMP_E_DIM;
    }
    if (!scalars || !ws || (N > 0 && (!log_z || !T_prime || !ll || !g_log_z || !g_T_prime || !r))) {
        set_error("vmp_svae_elbo_tail: NULL argument");
        return VMP_E_BADARG;
    }
    if (ws_bytes < tail_workspace_bytes()) {
        set_error("vmp_svae_elbo_tail: workspace too small (%zu < %zu bytes)", ws_bytes, tail_workspace_bytes());
        return VMP_E_WS;
    }
    TailArgs a{};
    const unsigned blocks = tail_setup(a, log_z, T_prime, ll, N, K, S, Dy, sigma, scalars, g_log_z, g_T_prime, r, ws, TAIL_THREADS);
    hipLaunchKernelGGL(elbo_tail_kernel, dim3(blocks), dim3(TAIL_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (blocks > 1) hipLaunchKernelGGL(elbo_final_kernel, dim3(1), dim3(WAVE), 0, static_cast<hipStream_t>(stream), a, blocks);   // one block: it wrote the scalars itself
    return check_launch("vmp_svae_elbo_tail");
}

int vmp_pack_f64(int n_tensors, const void* const* src, const int* src_is_f64, const int64_t* sizes, double* dst, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!src || !src_is_f64 || !sizes || !dst))) {
        set_error("vmp_pack_f64: bad arguments");
        return VMP_E_BADARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int t = 0;
    unsigned long long off = 0;
    while (t < n_tensors) {
        PackArgs a{};
        unsigned blocks = 0;
        int nt = 0;
        for (; t < n_tensors && nt < ADAM_MAX_TENSORS; ++t) {
            if (sizes[t] < 0 || off + (unsigned long long)sizes[t] >= 4294967296ULL || (sizes[t] > 0 && !src[t])) {
                set_error("vmp_pack_f64: tensor %d: NULL pointer or size out of range", t);
                return VMP_E_BADARG;
            }
            if (sizes[t] == 0) continue;
            a.src[nt] = src[t]; a.n[nt] = (unsigned)sizes[t]; a.off[nt] = (unsigned)off;
            if (src_is_f64[t]) a.f64mask |= 1u << nt;
            off += (unsigned long long)sizes[t];
            blocks += (unsigned)((sizes[t] + ADAM_CHUNK - 1) / ADAM_CHUNK);
            a.end_block[nt] = blocks;
            ++nt;
        }
        if (!nt) continue;
        a.nt = nt; a.dst = dst;
        hipLaunchKernelGGL(pack_f64_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, s, a);
    }
    return check_launch("vmp_pack_f64");
}

int vmp_adam_step_packed(int n_tensors, float* const* params, const double* gbuf, const int64_t* goffsets, double gscale,
                         float* const* grads_out, float* const* m, float* const* v, const int64_t* sizes, double beta1,
                         double beta2, double eps, double lr_t, const float* lr_t_dev, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!params || !gbuf || !goffsets || !m || !v || !sizes))) {
        set_error("vmp_adam_step_packed: bad arguments");
        return VMP_E_BADARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int t = 0;
    while (t < n_tensors) {
        AdamPackedArgs a{};
        unsigned blocks = 0;
        int nt = 0;
        for (; t < n_tensors && nt < ADAM_MAX_TENSORS; ++t) {
            if (sizes[t] < 0 || sizes[t] >= 2147483648LL || goffsets[t] < 0 || goffsets[t] + sizes[t] >= 4294967296LL || !params[t] ||
                !m[t] || !v[t]) {
                set_error("vmp_adam_step_packed: tensor %d: NULL pointer or size / offset out of range", t);
                return VMP_E_BADARG;
            }
            if (sizes[t] == 0) continue;
            a.p[nt] = params[t]; a.gout[nt] = grads_out ? grads_out[t] : nullptr; a.m[nt] = m[t]; a.v[nt] = v[t];
            a.n[nt] = (unsigned)sizes[t]; a.off[nt] = (unsigned)goffsets[t];
            blocks += (unsigned)((sizes[t] + ADAM_CHUNK - 1) / ADAM_CHUNK);
            a.end_block[nt] = blocks;
            ++nt;
        }
        if (!nt) continue;
        a.nt = nt; a.gbuf = gbuf; a.gscale = gscale; a.lr_t_dev = lr_t_dev; a.lr_t = (float)lr_t; a.b1 = (float)beta1;
        a.b2 = (float)beta2; a.c1 = (float)(1.0 - beta1); a.c2 = (float)(1.0 - beta2); a.eps = (float)eps;
        hipLaunchKernelGGL(adam_packed_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, s, a);
    }
    return check_launch("vmp_adam_step_packed");
}

int vmp_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* m, float* const* v,
                  const int64_t* sizes, double beta1, double beta2, double eps, double lr_t, const float* lr_t_dev, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!params || !grads || !m || !v || !sizes))) {
        set_error("vmp_adam_step: bad arguments");
        return VMP_E_BADARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int t = 0;
    while (t < n_tensors) {
        AdamArgs a{};
        unsigned blocks = 0;
        int nt = 0;
        for (; t < n_tensors && nt < ADAM_MAX_TENSORS; ++t) {
            if (sizes[t] < 0 || sizes[t] >= 2147483648LL || !params[t] || !grads[t] || !m[t] || !v[t]) {
                set_error("vmp_adam_step: tensor %d: NULL pointer or size out of range", t);
                return VMP_E_BADARG;
            }
            if (sizes[t] == 0) continue;
            a.p[nt] = params[t]; a.g[nt] = grads[t]; a.m[nt] = m[t]; a.v[nt] = v[t];
            a.n[nt] = (unsigned)sizes[t];
            blocks += (unsigned)((sizes[t] + ADAM_CHUNK - 1) / ADAM_CHUNK);
            a.end_block[nt] = blocks;
            ++nt;
        }
        if (!nt) continue;
        a.nt = nt; a.lr_t_dev = lr_t_dev; a.lr_t = (float)lr_t; a.b1 = (float)beta1; a.b2 = (float)beta2;
        a.c1 = (float)(1.0 - beta1); a.c2 = (float)(1.0 - beta2); a.eps = (float)eps;
        hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, s, a);
    }
    return check_launch("vmp_adam_step");
}

}  // extern "C"
