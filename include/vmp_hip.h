/*
 * vmp_hip.h - C ABI of libvmp_hip.so: the MI355X (gfx950) implementation of the VMP hot path of
 * emtiyaz/vmp-for-svae (GMM / SMM structured VAE).
 *
 * The reference has no FFI: its boundary is the Python function surface of distributions/{gaussian,niw,dirichlet,student_t}.py and
 * models/{gmm,smm,svae,vae}.py.  This library sits UNDER the package's mirror of that
 * surface (vmp-for-svae_amd/{distributions,models}); each entry point names the reference code it replaces.
 *
 * Conventions (all entry points)
 *   - plain C symbols; every pointer is a DEVICE pointer unless the name ends in _host;
 *   - row-major, batch-leading fp32 tensors exactly as the reference lays them out: x (N,D), r (N,K),
 *     (K,D,D), (N,K,S,L) ...; integer sizes: N int64, everything else int;
 *   - caller allocates inputs, outputs and workspace; the library never allocates device memory (one exception: vmp_exch_alloc, the uncached IPC exchange buffer of the peer form);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return 0 = ok, <0 = invalid argument (VMP_E_*), >0 = hipError_t of a failed launch;
 *     vmp_last_error() returns a thread-local message for the last non-zero return;
 *   - no global mutable state: callable concurrently from any host thread.
 */
#ifndef VMP_HIP_H
#define VMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMP_ABI_VERSION 1

#define VMP_E_BADARG   (-1)   /* null pointer / non-positive size            */
#define VMP_E_DIM      (-2)   /* D or K outside the compiled range           */
#define VMP_E_WS       (-3)   /* workspace too small                         */
#define VMP_E_NOIMPL   (-4)   /* no kernel of this form for these sizes      */

#define VMP_MAX_D 8           /* latent / data dimension of the mixture (compiled range 1..8)  */
#define VMP_MAX_K 64          /* mixture components                                             */
#define VMP_DIAG_MAX_D 64     /* data dimension of the diagonal-covariance mixture (compiled range 1..64) */

/* mixture flavour */
#define VMP_GMM 0             /* models/gmm.py  (Bishop 10.2)                */
#define VMP_SMM 1             /* models/smm.py  (Archambeau & Verleysen)     */

int         vmp_abi_version(void);
const char* vmp_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * T1: pure mixture VMP (models/gmm.py:25-269, models/smm.py:25-245)
 * ------------------------------------------------------------------------------------------------ */

/* Number of fp32 words per component of the E-step parameter pack written by vmp_mix_finalize and
 * consumed by vmp_mix_estep: [ m_k (D) | W_k packed lower-triangular, row-major (D(D+1)/2) | c | h | ua | ub ]
 * with  q_nk = || W_k (x_n - m_k) ||^2,  log rho_nk = c - h*q_nk,  u_nk = ua / (q_nk + ub).           */
int    vmp_mix_pack_words(int D);

/* Raw sufficient statistics layout (fp64), per component k:  [ Nk | Wk | sx (D) | sxx (D*D, symmetric) ].
 * Nk = sum_n r_nk, Wk = sum_n w_nk, sx = sum_n w_nk x_n, sxx = sum_n w_nk x_n x_n^T, w = r (GMM) or r*u (SMM). */
int    vmp_mix_stats_words(int D);

/* Bytes of workspace needed by vmp_mix_stats / vmp_mix_estep(with stats) for N rows. */
size_t vmp_mix_workspace_bytes(int64_t N, int D, int K);

/* M-pass over the data: weighted raw moments.
 * Replaces the N-sized part of gmm.update_Nk/xk/Sk (models/gmm.py:25-46) and smm.update_Nk/Wk/xk/Sk
 * (models/smm.py:25-50); the centring (x - x_k) the reference does in a second pass is done in fp64 in
 * vmp_mix_finalize / on the host side from the raw moments.
 *   x (N,D), r (N,K), u (N,K) or NULL (then w = r).   stats: (K, vmp_mix_stats_words(D)) fp64, overwritten.  */
int    vmp_mix_stats(const float* x, const float* r, const float* u, const float* pivot, int64_t N, int D, int K,
                     double* stats, void* ws, size_t ws_bytes, void* stream);

/* Pivot for the moment accumulation (D floats): the mean of up to 4096 evenly strided rows of x.  The moment
 * kernels accumulate products of (x - pivot) in fp32 and the finalize kernels un-shift exactly in fp64, which
 * makes the one-pass raw-moment form as accurate as the reference's two-pass centred update_Sk (gmm.py:39-46)
 * for data far from the origin.  `pivot` arguments below may be NULL (no shift).                           */
int    vmp_mix_pivot(const float* x, int64_t N, int D, float* pivot_out, void* stream);

/* K-sized posterior update + E-step parameter pack, all in fp64 on the device, rounded to fp32 on output.
 * Replaces gmm.update_alphak/betak/mk/Ck/vk (models/gmm.py:49-81), P_k = matrix_inverse(C_k) (gmm.py:260),
 * compute_expct_log_det_prec (gmm.py:117-131, including its det<=1e-20 guard), compute_log_pi (gmm.py:134-138);
 * SMM flavour: models/smm.py:53-85, 99-116 and the constants of compute_rnk/compute_expct_unk (smm.py:119-137).
 *   prior (standard form): alpha0 (K), beta0 (K), m0 (K,D), C0 (K,D,D), v0 (K); kappa (K) or NULL (GMM).
 *   outputs (any may be NULL): alpha,beta,v (K); m, xbar (K,D); C, S (K,D,D); pi = exp(E log pi) (K);
 *   pack (K, vmp_mix_pack_words(D)).                                                                     */
int    vmp_mix_finalize(const double* stats, int D, int K, int flavour,
                        const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                        const float* kappa,
                        float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S, float* pi,
                        float* pack, void* stream);

/* E-step parameter pack from explicit posterior parameters (for the stand-alone e_step API):
 * gmm.e_step(x, alpha_k, beta_k, m_k, P_k, v_k) (models/gmm.py:154-174) / smm.e_step (models/smm.py:140-164).
 *   P (K,D,D) is the precision the reference passes in.                                                   */
int    vmp_mix_pack_from_params(int D, int K, int flavour, const float* alpha, const float* beta, const float* m,
                                const float* P, const float* v, const float* kappa, float* pack, float* pi,
                                void* stream);

/* E-pass over the data: responsibilities (and SMM scales), optionally FUSED with the raw moments of the
 * NEW responsibilities (= the next M-pass), so that one VMP iteration streams x once and writes r once.
 * Replaces compute_expct_mahalanobis_dist + compute_rnk (models/gmm.py:84-94,141-151), the missing-data variant
 * (gmm.py:97-114) when miss_mask != NULL, and smm.expct_mahalanobis_dist/compute_rnk/compute_expct_unk
 * (models/smm.py:88-96,119-137).
 *   x (N,D); pack from vmp_mix_finalize / vmp_mix_pack_from_params; miss_mask (N,D) uint8 or NULL;
 *   r_out (N,K); u_out (N,K) (SMM, else NULL); logr_out (N,K) or NULL (= log r_out as gmm.py:267);
 *   stats_out (K, vmp_mix_stats_words(D)) fp64 or NULL; ws needed only when stats_out != NULL.            */
int    vmp_mix_estep(const float* x, int64_t N, int D, int K, int flavour, const float* pack,
                     const uint8_t* miss_mask, float* r_out, float* u_out, float* logr_out,
                     const float* pivot, double* stats_out, void* ws, size_t ws_bytes, void* stream);

/* Fast path of the VMP iteration - exactly two launches per iteration, no intermediate stats buffer:
 *   vmp_mix_estep_fused : the E-pass kernel with fused raw moments; leaves per-block fp64 partials in `ws`
 *   vmp_mix_finalize_ws : reduces those partials in a fixed order (deterministic), then does what
 *                         vmp_mix_finalize does; stats_out (K, stats_words) is optional.
 * Both must be given the same (N, D, K, flavour) and the same ws.  vmp_mix_stats_ws is the stand-alone
 * M-pass leaving partials in ws (first iteration).  Reference: the loop body of gmm.inference
 * (models/gmm.py:258-263) / smm.inference (models/smm.py:232-238).                                          */
int    vmp_mix_estep_fused(const float* x, int64_t N, int D, int K, int flavour, const float* pack,
                           float* r_out, float* u_out, float* logr_out, const float* pivot,
                           void* ws, size_t ws_bytes, void* stream);
int    vmp_mix_stats_ws(const float* x, const float* r, const float* u, const float* pivot, int64_t N, int D, int K,
                        void* ws, size_t ws_bytes, void* stream);
int    vmp_mix_finalize_ws(const void* ws, const float* pivot, int64_t N, int D, int K, int flavour,
                           const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                           const float* kappa,
                           float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S, float* pi,
                           float* pack, double* stats_out, void* stream);

/* `iterations` VMP iterations enqueued back-to-back from one call (2 launches each, no host round trip):
 * the loop `for i in range(nb_iters): sess.run(update)` of models/gmm.py:377-379.  ws must hold the partial moments
 * of the current (r, u) (vmp_mix_stats_ws or a previous iteration).                                             */
/* Opt-in ACCURATE E-part (round 6).  The SMM's log rho_nk = c_k - (D + kappa)/2 q_nk (models/smm.py:119-128) is LINEAR in the
 * expected Mahalanobis distance with a factor 6.5 at D = 8, kappa = 5: rows without a close component have |log rho| ~ 1e2..1e3,
 * where an fp32 q (absolute error 1e-7 q) and an fp32 log rho cost 1..4e-5 on r_nk - above the 1e-5 the north-star states.
 * vmp_mix_finalize_ws64 = vmp_mix_finalize_ws that also writes the E-step pack in fp64 (pack64: K x vmp_mix_pack_words(D) doubles);
 * vmp_mix_estep_accurate evaluates compute_expct_mahalanobis_dist / compute_rnk / compute_expct_unk (models/gmm.py:84-94,141-151,
 * models/smm.py:88-96,119-137) from it entirely in fp64 and rounds r (u, log r) once on the way out.  It does NOT accumulate
 * moments: follow it with vmp_mix_stats_ws_accurate - gmm.update_Nk/xk/Sk (gmm.py:25-46) / smm.update_* (smm.py:25-50) with every
 * product and sum in fp64, into the same workspace partials vmp_mix_stats_ws leaves (a 5e-8 relative error of P_k, the level of the
 * default moments, is 1e-4 on the SMM's log rho of rows without a close component).  Three streaming launches per iteration
 * instead of one - the default stays the fused pass.                                                                       */
int    vmp_mix_finalize_ws64(const void* ws, const float* pivot, int64_t N, int D, int K, int flavour,
                             const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                             const float* kappa, float* alpha, float* beta, float* m, float* C, float* v, float* xbar,
                             float* S, float* pi, float* pack, double* pack64, double* stats_out, void* stream);
int    vmp_mix_estep_accurate(const float* x, int64_t N, int D, int K, int flavour, const double* pack64, float* r_out,
                              float* u_out, float* logr_out, void* stream);
int    vmp_mix_stats_ws_accurate(const float* x, const float* r, const float* u, const float* pivot, int64_t N, int D, int K,
                                 void* ws, size_t ws_bytes, void* stream);
int    vmp_mix_iterate(const float* x, int64_t N, int D, int K, int flavour,
                       const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                       const float* kappa, const float* pivot, float* r, float* u,
                       float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S, float* pi,
                       float* pack, void* ws, size_t ws_bytes, int iterations, void* stream);
/* Host query, no launch and no device: the launch plan of a streaming pass of the mixture.  estep / stats / mask name the pass: the M-pass
 * of vmp_mix_stats* is (0,1,0), vmp_mix_estep runs (1,0,0), with stats_out (1,1,0) - the pass of vmp_mix_estep_fused - and with a
 * miss_mask (1,0,1).  out = [form (1 tiled, 2 XDL) | KT (tiled: 16-component tiles per wave) or MT (XDL: bf16 terms of the moment
 * operands) | waves per block | blocks = partial rows the finalize launches reduce | rows per wave | rows per wave of a block's second
 * half | parallel block reduction | dynamic LDS bytes].  Returns 0, or what the pass would return and out zeroed: VMP_E_DIM,
 * VMP_E_BADARG (N < 1, a flavour that is neither, a combination no kernel exists for: a mask with VMP_SMM or with stats).  */
int    vmp_mix_pass_plan(int64_t N, int D, int K, int flavour, int estep, int stats, int mask, int64_t* out);

/* The fused pass of an iteration that nobody reads r from: vmp_mix_estep_fused without r_out, u_out and logr_out.  Within an
 * iteration nothing reads them - vmp_mix_finalize_ws takes the partials in `ws`, the next pass forms r again from x and the new
 * pack - so the kernel issues no store of them: per iteration the launch reads x and writes the partials, where the storing pass
 * also writes N K floats of r (and of u).  Same launch plan, same rows per wave, same order: the partials are the bits
 * vmp_mix_estep_fused leaves.  r (u) of the current pack, when wanted: vmp_mix_estep with the same pack and pivot, which gives the
 * bits the fused pass would have stored.  Instances exist where the fused pass runs the XDL form (vmp_mix_pass_plan(.., 1, 1, 0):
 * form 2, K <= 16); otherwise VMP_E_NOIMPL and nothing is launched - call vmp_mix_estep_fused.
 * (The two names carry the vmp_mixture_ prefix of the newer entry points although they live beside vmp_mix_estep_fused: the set of
 * vmp_mix_* symbols is closed - tests/test_abi.py holds every one of them to a table of NULL-pointer codes.)
 * vmp_mixture_iterate_nostore: vmp_mix_iterate over this pass (no r, no u); everything either launch refuses is refused before the
 * first one.  Errors (decided before any launch): VMP_E_DIM, VMP_E_BADARG (N < 1, x, pack or ws NULL, a flavour that is neither,
 * iterations < 0), VMP_E_WS, VMP_E_NOIMPL.                                                                                     */
int    vmp_mixture_estep_fused_nostore(const float* x, int64_t N, int D, int K, int flavour, const float* pack, const float* pivot,
                                       void* ws, size_t ws_bytes, void* stream);
int    vmp_mixture_iterate_nostore(const float* x, int64_t N, int D, int K, int flavour,
                                   const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                                   const float* kappa, const float* pivot,
                                   float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S, float* pi,
                                   float* pack, void* ws, size_t ws_bytes, int iterations, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture scoring (csrc/vmp_score.hip): held-out log predictive density of the pure mixtures in one streaming pass
 * ------------------------------------------------------------------------------------------------
 *   log p(x_n) = logsumexp_k [ c_k - h_k log1p(a_k q_nk) ],   q_nk = || W_k (x_n - m_k) ||^2,  W_k lower-triangular.
 * Score pack: (K, vmp_mix_pack_words(D)) fp32 = [ m_k (D) | W_k packed lower-triangular, row-major (D(D+1)/2) | c | h | a | 0 ]
 * (natural-log units; NOT interchangeable with the E-step pack of vmp_mix_finalize).  A component whose matrix is not
 * symmetric positive definite, or whose degrees of freedom are not positive, gets NaN in W, c, h, a: every row scores NaN.
 *
 * vmp_mix_score_pack_niw: the posterior predictive of a variational GMM (Bishop, PRML 10.81-10.82) from the NIW posterior
 *   (alpha (K), beta (K), m (K,D), C (K,D,D), v (K)) - the theta of gmm.inference (models/gmm.py:230-269); C is the inverse
 *   scale (P_k = C_k^-1, gmm.py:260) and (v_k, P_k) the Wishart (nu, W) pair as gmm.py:84-94 reads it:
 *   nu' = v + 1 - D,  C = L L^T,  W = L^-1,  a = beta / (1 + beta),  h = (nu' + D) / 2,
 *   c = log(alpha / sum alpha) + lgamma(h) - lgamma(nu' / 2) - D/2 log(pi nu') + D/2 log(nu' beta / (1 + beta)) - sum_i log L_ii.
 * vmp_mix_score_pack_t: explicit Student-t mixture (log_w (K), mu (K,D), sigma (K,D,D), nu (K)): student_t.log_probability
 *   (distributions/student_t.py:31-37) + log_w, i.e. the (N,K) terms of logprob_smm_mixture (student_t.py:42-56):
 *   sigma = L L^T,  W = L^-1,  a = 1 / nu,  h = (nu + D) / 2,  c = log_w + lgamma(h) - lgamma(nu / 2) - D/2 log(pi nu) - sum_i log L_ii. */
int    vmp_mix_score_pack_niw(int D, int K, const float* alpha, const float* beta, const float* m, const float* C,
                              const float* v, float* pack, void* stream);
int    vmp_mix_score_pack_t(int D, int K, const float* log_w, const float* mu, const float* sigma, const float* nu,
                            float* pack, void* stream);
/* The streaming pass: the log-sum-exp over k the reference leaves to its caller after student_t.py:42-56 (and, for the GMM,
 * the predictive density its models/gmm.py does not have).  x (N,D) (any alignment), pack from one of the builders above.
 * Outputs, each optional but not all NULL: logp_out (N); resp_out (N,K) = exp(term_nk - logp_n), the predictive
 * responsibilities (0 in a row whose every term is -inf, where logp = -inf); sum_out = sum_n logp_n, one fp64 word:
 * per-block fp64 partials in `ws` (vmp_mix_score_workspace_bytes, needed only with sum_out) added in a fixed order by a
 * second one-wave launch - no atomics, bit-identical from run to run and whichever other outputs are requested.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1, x or pack
 * NULL, no output), VMP_E_WS.                                                                                        */
size_t vmp_mix_score_workspace_bytes(int64_t N, int D, int K);
int    vmp_mix_score(const float* x, int64_t N, int D, int K, const float* pack, float* logp_out, float* resp_out,
                     double* sum_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture imputation (csrc/vmp_impute.hip): partly observed rows under a mixture of Student-t densities in one streaming pass
 * ------------------------------------------------------------------------------------------------
 * For a row x with observed entries o (D_o of them) and missing entries m, a component (log w, mu, Sigma, nu), Lambda = Sigma^-1,
 * d_o = x_o - mu_o:   R R^T = Lambda_mm,  t = Lambda_mo d_o,  y = R^-1 t,
 *   q = d_o^T Sigma_oo^-1 d_o = d_o^T Lambda_oo d_o - |y|^2,    log det Sigma_oo = -log det Lambda + 2 sum_i log R_ii,
 *   l_k = log w + lgamma((nu + D_o)/2) - lgamma(nu/2) - D_o/2 log(pi nu) - 1/2 log det Sigma_oo - (nu + D_o)/2 log1p(q / nu),
 *   xhat_m^(k) = mu_m - R^-T y   (the conditional mean for nu > 1; for nu <= 1 the mean does not exist and this is the
 *                                 conditional location - it is what is returned either way),
 *   logp = logsumexp_k l_k,   resp_k = exp(l_k - logp),   xhat_m = sum_k resp_k xhat_m^(k).
 * A row with nothing missing: logp and resp of vmp_mix_score; a row with nothing observed: l_k = log w_k.
 * Impute pack: (K, vmp_mixture_impute_pack_words(D)) fp32 =
 *   [ mu (D) | Lambda packed lower-triangular, row-major (D(D+1)/2) | log w | nu | log det Lambda | 1 / nu | G[0..D] ],
 *   G[j] = lgamma((nu + j)/2) - lgamma(nu/2) - j/2 log(pi nu)  - the streaming kernel evaluates no lgamma.  A component whose matrix is
 *   not symmetric positive definite, or whose degrees of freedom are not positive, gets a NaN pack row: every row's logp is NaN.
 * (These entry points are named vmp_mixture_*: the vmp_mix_* prefix is the closed set of csrc/vmp_mix.hip and the scoring pass.)
 *
 * vmp_mixture_impute_pack_niw: the posterior predictive of the NIW posterior (alpha (K), beta (K), m (K,D), C (K,D,D), v (K)) of
 *   gmm.inference: w = alpha / sum alpha, mu = m, nu' = v + 1 - D, Sigma = C (1 + beta) / (beta nu') - the mapping of
 *   vmp_mix_score_pack_niw.
 * vmp_mixture_impute_pack_t: explicit (log_w (K), mu (K,D), sigma (K,D,D), nu (K)), as vmp_mix_score_pack_t.              */
int    vmp_mixture_impute_pack_words(int D);
int    vmp_mixture_impute_pack_niw(int D, int K, const float* alpha, const float* beta, const float* m, const float* C,
                                   const float* v, float* pack, void* stream);
int    vmp_mixture_impute_pack_t(int D, int K, const float* log_w, const float* mu, const float* sigma, const float* nu,
                                 float* pack, void* stream);
/* The streaming pass.  x (N,D) (any alignment); mask (N,D) uint8, nonzero = missing (the convention of missing_data_mask,
 * models/gmm.py:97-114); pack from one of the builders above.  The value in a missing slot of x never enters arithmetic (NaN and
 * +-Inf there are as good as 0).  Outputs, each optional but not all NULL: x_out (N,D) - the observed entries of x copied bit for
 * bit, the missing ones filled with xhat; x_out == x fills in place; logp_out (N); resp_out (N,K); sum_out = sum_n logp_n, one
 * fp64 word: per-block fp64 partials in `ws` (vmp_mixture_impute_workspace_bytes, needed only with sum_out) added in a fixed order
 * by a second one-wave launch - no atomics, bit-identical from run to run.  Every output has the same bits whichever others are
 * requested.  log w_k = -inf: resp_k = 0; every log w = -inf: logp = -inf, resp = 0 and the filled entries are 0 (the observed ones
 * are still copied) - no NaN.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1, x, mask or pack
 * NULL, no output), VMP_E_WS.                                                                                              */
size_t vmp_mixture_impute_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_impute(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* x_out,
                          float* logp_out, float* resp_out, double* sum_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture sampling (csrc/vmp_sample.hip): seeded draws and multiple imputation under a mixture of Student-t densities, one launch
 * ------------------------------------------------------------------------------------------------
 * `draws` independent draws of the missing entries of every row from p(x_m | x_o) under an impute pack (the notation of "Mixture
 * imputation" above); a row with nothing observed is a draw from the mixture itself.  For row n and draw s:
 *   component  resp_k = exp(l_k - logsumexp l), the numbers vmp_mixture_impute returns;  z = the first k with
 *              sum_{j<=k} resp_j > u_z, or, if rounding leaves the total below u_z, the last k with resp_k > 0;
 *   scale      g ~ Gamma(shape a = (nu_z + D_o)/2, rate 1/2) (chi-square with nu_z + D_o degrees of freedom) by Marsaglia-Tsang
 *              (2000) on a' = a (a >= 1) or a + 1 (a < 1): d = a' - 1/3, c = 1/sqrt(9 d); attempt t = 0 .. 7 takes a normal n_t and a
 *              uniform u_t, w = 1 + c n_t, v = w^3, and is accepted if w > 0 and log u_t < n_t^2/2 + d - d v + d log v; gamma = d v of
 *              the first accepted attempt (d itself if all 8 are rejected: probability <= 0.0484^8 < 3.1e-11, 0.0484 being the
 *              rejection probability at a' = 1, where it is largest); g = 2 gamma, times u_b^(1/a) when a < 1; g >= FLT_MIN;
 *   entries    x_m = xhat_m^(z) + sqrt((nu_z + q_z) / g) R_z^-T eps, eps_i standard normal, indexed by the coordinate i (observed
 *              coordinates discard theirs); observed entries are copied bit for bit.
 * This is the conditional Student-t t_{nu+D_o}(xhat, (nu + q)/(nu + D_o) Lambda_mm^-1) of each component, mixed by resp.
 * Random stream: Philox4x32-7 (the generator of the in-kernel noise below), key = seed, counter = (row low, row high, s, 0x6d78a500 + b)
 * with row = row0 + n the absolute row index and b the block - nothing else enters, so rows [a, b) drawn with row0 = a are rows a .. b
 * of the whole call.  A uniform is (top 24 bits of a word + 1/2) 2^-24, rounded once to fp32 and kept at most 1 - 2^-24 (the one
 * value that would round to 1.0): never 0, never 1; a normal pair is
 * r (cos, sin) with r = sqrt(-2 log((top 20 bits + 1/2) 2^-20)) and the angle = low 12 bits x 2^-12 revolutions of ONE word
 * (oracle/philox.py box_muller8).
 *   b = 0:       word 0 -> u_z, word 1 -> u_b
 *   b = 1:       word t -> (eps_2t, eps_2t+1), t = 0 .. 3
 *   b = 16 + t:  attempt t: word 0 -> n_t (the cosine of its pair), word 1 -> u_t
 * x (N,D), mask (N,D) uint8, nonzero = missing; x == NULL && mask == NULL: every entry of every row is missing (plain draws from the
 * mixture).  What a missing slot of x holds never enters arithmetic.  x_out (draws,N,D); z_out (draws,N) int32 or NULL.  A row whose
 * every log w is -inf gets 0 in its missing entries and z = -1; a NaN pack row as the builders write it (log w
 * included) makes every l_k term of the row's softmax NaN: NaN draws and z = -1.  With nothing observed (D_o = 0, and always when
 * x == NULL) l_k = log w_k alone, so a pack row with a finite log w but NaN in mu, Lambda or nu is chosen with its weight and gives NaN
 * entries with z = that k, while the other components draw normally.  No workspace, no atomics,
 * one launch: every output is bit-identical from run to run and whether or not z_out is requested.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1, draws < 1, row0 < 0,
 * exactly one of x and mask NULL, pack or x_out NULL).                                                                       */
int    vmp_mixture_sample(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* impute_pack, uint64_t seed,
                          int64_t row0, int draws, float* x_out, int32_t* z_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture fitting on partly observed rows (csrc/vmp_missfit.hip): variational Bayes with the missing entries as latent variables
 * ------------------------------------------------------------------------------------------------
 * The variational GMM of models/gmm.py (NIW posterior (alpha, beta, m, C, v) per component, C the inverse scale, P = C^-1) on rows
 * whose entries are missing at random.  The factor is q(z_n, x_n,m) = q(z_n) q(x_n,m | z_n); for a row with observed entries o (D_o of
 * them) and missing entries m, Lbar_k = v_k P_k and d_o = x_o - m_k,o its optimum given q(pi, mu, Lambda) is
 *   R R^T = Lbar_mm,   t = Lbar_mo d_o,   y = R^-1 t,   q_o = d_o^T Lbar_oo d_o - |y|^2,
 *   xhat_m^(k) = m_k,m - R^-T y,   xhat_o^(k) = x_o,   Cov^(k) = Lbar_mm^-1 on the (m,m) block and 0 elsewhere (it depends on the
 *                                                       row's pattern and on k, not on the row's values),
 *   log rho_nk = E log pi_k + 1/2 E log|Lambda_k| - D / (2 beta_k) - 1/2 q_o - sum_i log R_ii   [ - D_o/2 log 2 pi ],
 *   r_nk = softmax_k log rho_nk,
 * with E log pi and E log|Lambda| as compute_log_pi / compute_expct_log_det_prec give them (models/gmm.py:117-138, the det <= 1e-20
 * guard included).  The bracketed term is the same for every k: the pass leaves it out (it matters for the lower bound only).  A row
 * with nothing missing is the E-step of vmp_mix_estep (Bishop 10.46 / 10.64); a row with nothing observed has q_o = 0.
 * The M-step is the NIW update of vmp_mix_finalize, unchanged, on the raw moments of the COMPLETED rows in the vmp_mix_stats layout:
 *   Nk = Wk = sum_n r_nk,   sx = sum_n r_nk xhat_n^(k),   sxx = sum_n r_nk ( xhat_n^(k) xhat_n^(k)^T + Cov_n^(k) ).
 * Fit pack: (K, vmp_mixture_fit_pack_words(D)) fp32 = [ m (D) | Lbar packed lower-triangular, row-major (D(D+1)/2) | c ],
 *   c = E log pi + 1/2 E log|Lambda| - D / (2 beta), built by vmp_mixture_fit_pack from (alpha (K), beta (K), m (K,D), C (K,D,D), v (K))
 *   with one thread per component, fp64 inside, rounded once.  A component whose C is not symmetric positive definite gets a NaN row.
 *
 * vmp_mixture_fit_pass: one streaming pass over x (N,D) (any alignment) and mask (N,D) uint8, nonzero = missing.  The value in a
 *   missing slot of x never enters arithmetic (NaN and +-Inf there are as good as 0).  Outputs: r_out (N,K), required; logr_out (N,K)
 *   = log r, optional; x_fill_out (N,D), optional - the observed entries of x copied bit for bit, the missing ones filled with
 *   sum_k r_nk xhat_m^(k); stats_out (K, vmp_mix_stats_words(D)) fp64, optional.  The moments are accumulated in fp32 on
 *   xhat - m_k (the shift is the component's own location, taken from the pack), flushed to fp64 every 128 rows of a wave into that
 *   wave's own words of `ws`, and added over the waves in a fixed order by a second launch that undoes the shift in fp64 - no
 *   atomics; every output is bit-identical from run to run and whichever optional outputs are requested.  ws
 *   (vmp_mixture_fit_workspace_bytes, 8-byte aligned) is always needed; without stats_out the second launch is skipped.
 * vmp_mixture_fit_iterate: `iterations` x (vmp_mix_finalize on stats -> vmp_mixture_fit_pack -> vmp_mixture_fit_pass with stats_out =
 *   stats) enqueued back to back, no host work in between; stats holds the moments of the current r on entry (seeded by
 *   vmp_mix_stats) and of the last r on return.  logr, x_fill, xbar, S, pi may be NULL.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1, x, mask, pack or
 *   r_out NULL - no output -, a NULL prior, posterior or stats of the iteration, iterations < 0), VMP_E_WS.                      */
int    vmp_mixture_fit_pack_words(int D);
int    vmp_mixture_fit_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* C, const float* v,
                            float* pack, void* stream);
size_t vmp_mixture_fit_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_fit_pass(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* r_out,
                            float* logr_out, float* x_fill_out, double* stats_out, void* ws, size_t ws_bytes, void* stream);
int    vmp_mixture_fit_iterate(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* alpha0,
                               const float* beta0, const float* m0, const float* C0, const float* v0, float* r, float* logr,
                               float* x_fill, float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S,
                               float* pi, float* pack, double* stats, void* ws, size_t ws_bytes, int iterations, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Variational lower bound (csrc/vmp_bound.hip): the free energy of the Gaussian-mixture fit, complete or partly observed rows
 * ------------------------------------------------------------------------------------------------
 * Gaussian mixture only.  theta = (alpha, beta, m, C, v) the NIW posterior, prior = (alpha0, beta0, m0, C0, v0), Lbar_k = v_k C_k^-1,
 * o(n) the observed entries of row n (D_o(n) of them; without a mask all D):
 *   bound   = data - kl_pi - sum_k kl_nw_k
 *   data    = sum_n [ logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi ]
 *   log rho_nk = c_k - 1/2 q_o - sum_i log R_ii       the cell of "Mixture fitting on partly observed rows", from the fit pack
 *                                                      [ m | Lbar packed lower | c_k ] of vmp_mixture_fit_pack; a complete row:
 *                                                      c_k - 1/2 (x_n - m_k)^T Lbar_k (x_n - m_k)
 *   kl_pi   = lgamma(sum alpha) - sum lgamma(alpha) - lgamma(sum alpha0) + sum lgamma(alpha0) + sum_k (alpha_k - alpha0_k) E log pi_k
 *   kl_nw_k = 1/2 D log(beta / beta0) - 1/2 D + 1/2 D beta0 / beta + 1/2 beta0 (m - m0)^T Lbar (m - m0)
 *             + logB(C, v) - logB(C0, v0) + 1/2 (v - v0) E log|Lambda| - 1/2 v D + 1/2 tr(C0 Lbar)
 *   logB(C, nu) = 1/2 nu log|C| - 1/2 nu D log 2 - 1/4 D (D - 1) log pi - sum_{i=1..D} lgamma((nu + 1 - i) / 2)
 * with E log pi and E log|Lambda| the expectations of the E-step, as vmp_mixture_fit_pack computes them (digamma arguments
 * (v + 1 + i) / 2, log det P replaced by 0 where det P <= 1e-20).  It is the free energy of the state after an iteration: theta from
 * the M-step, r from the E-step at that theta (the log-sum-exp is the optimum over q(z_n) q(x_n,m | z_n)).  With the reference's
 * v_k = v_0 + N_k + 1 the M-step is not the exact optimum, so the bound need not rise at every single iteration.
 *
 * vmp_mixture_bound_pass: one streaming pass over x (N,D) (any alignment) and, if mask != NULL, mask (N,D) uint8, nonzero = missing,
 *   then a one-wave launch that adds the per-block sums.  data_out (1) fp64, required; lse_out (N) fp32 = logsumexp_k log rho_nk
 *   (without the 2 pi term), optional.  Per row the log-sum-exp is fp32; the rows are added in fp64 in a fixed order - lanes, waves,
 *   blocks; no atomics, one geometry whichever outputs are requested: data_out is bit-identical from run to run and with or without
 *   lse_out.  mask == NULL: nothing is factored, log rho = c - 1/2 d^T Lbar d.  With a mask the pass does the part of the fit pass's
 *   cell that log rho needs: the factor and the forward substitution - no back-substitution, no inverse, no moments, no r.  The
 *   value in a missing slot of x never enters arithmetic.  A row whose every term is -inf contributes -inf; a NaN pack gives NaN.
 *   ws (vmp_mixture_bound_workspace_bytes: one fp64 word per block, 8-byte aligned) is always needed.
 * vmp_mixture_bound_terms: one launch, one thread per component, fp64 inside:  out (2 + K) fp64 = [ kl_pi | sum_k kl_nw_k |
 *   kl_nw_0 .. kl_nw_{K-1} ], the sums over k taken by one thread in k order.  A component whose C or C0 is not symmetric positive
 *   definite gives NaN.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x, fit_pack or
 *   data_out NULL; a NULL prior, posterior or out of the terms; ws not 8-byte aligned), VMP_E_WS (ws NULL or too small).
 *   vmp_mixture_bound_workspace_bytes is 0 outside the compiled range.                                                        */
size_t vmp_mixture_bound_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_bound_pass(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* fit_pack, float* lse_out,
                              double* data_out, void* ws, size_t ws_bytes, void* stream);
int    vmp_mixture_bound_terms(int D, int K, const float* alpha0, const float* beta0, const float* m0, const float* C0, const float* v0,
                               const float* alpha, const float* beta, const float* m, const float* C, const float* v, double* out,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture fitting on weighted rows (csrc/vmp_wfit.hip): counts, coresets, importance weights and 0/1 folds over resident rows
 * ------------------------------------------------------------------------------------------------
 * Gaussian mixture only.  Weights w (N) fp32, finite, >= 0: w_n makes row n count as w_n identical rows (integer weights reproduce
 * the fit on the replicated rows); they need not sum to N.  With log rho_nk, the completed rows xhat^(k) and Cov^(k) exactly as in
 * "Mixture fitting on partly observed rows" (a complete row: log rho_nk = c_k - 1/2 (x_n - m_k)^T Lbar_k (x_n - m_k), xhat = x_n,
 * Cov = 0) and D_o(n) the number of observed entries of row n:
 *   r_nk = softmax_k log rho_nk                     UNCHANGED: a weight does not enter a row's own responsibilities
 *   Nk   = Wk = sum_n w_n r_nk
 *   sx   = sum_n w_n r_nk xhat_n^(k)
 *   sxx  = sum_n w_n r_nk ( xhat_n^(k) xhat_n^(k)^T + Cov_n^(k) )
 *   data = sum_n w_n ( logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi )             the data term of "Variational lower bound"
 *   lower bound = data - kl_pi - sum_k kl_nw_k      the two KL terms from vmp_mixture_bound_terms, unchanged
 * A row with w_n = 0 is removed by a SELECT, not by a multiplication: whatever its x holds - NaN and +-Inf in observed slots
 * included - reaches neither the moments nor data.  Its r (log r, x_fill) is still written, as whatever the E-step gives: the
 * responsibilities of a held-out row.  Negative or non-finite weights are the caller's to refuse (models/_mix.py check_weights).
 *
 * vmp_mixture_wfit_pass: one streaming pass over x (N,D) (any alignment), w (N) and, if mask != NULL, mask (N,D) uint8, nonzero =
 *   missing, under a FIT pack (vmp_mixture_fit_pack).  mask == NULL: nothing is factored.  Outputs, all optional but at least one:
 *   r_out (N,K); logr_out (N,K) = log r (needs r_out); x_fill_out (N,D) as in vmp_mixture_fit_pass (needs a mask); stats_out
 *   (K, vmp_mix_stats_words(D)) fp64 = [Nk | Wk = Nk | sx | sxx] (needs r_out); bound_out (1) fp64 = data.  r_out == NULL (and so
 *   stats_out == NULL) is the bound-only form: no moments are formed.  The moments are accumulated as in vmp_mixture_fit_pass (fp32 on
 *   xhat - m_k, flushed to fp64 every 128 rows of a wave, the waves added in a fixed order by a second launch that undoes the shift);
 *   the rows' terms of data are added in fp64 in a fixed order - lanes, waves, blocks, the blocks by a one-wave launch.  No atomics,
 *   one geometry whichever outputs are requested: moments and data are bit-identical from run to run and for every set of optional
 *   outputs.  ws (vmp_mixture_wfit_workspace_bytes: the fp64 moments of every wave and one fp64 word per block, 8-byte aligned) is
 *   always needed.
 * vmp_mixture_wfit_iterate: `iterations` x (vmp_mix_finalize on stats -> vmp_mixture_fit_pack -> vmp_mixture_wfit_pass with stats_out =
 *   stats, bound_out = bound) enqueued back to back, no host work in between; stats holds the weighted moments of the current r on
 *   entry (vmp_mix_stats of r_nk w_n: the moments are linear in r) and of the last r on return.  logr, x_fill, xbar, S, pi and bound
 *   may be NULL; r and stats may not.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x, w or pack NULL; no
 *   output; stats_out or logr_out without r_out; x_fill_out without mask; ws not 8-byte aligned; a NULL prior, posterior, r or stats
 *   of the iteration; iterations < 0), VMP_E_WS (ws NULL or too small).  vmp_mixture_wfit_workspace_bytes is 0 outside the compiled
 *   range.                                                                                                                   */
size_t vmp_mixture_wfit_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_wfit_pass(const float* x, const float* w, const uint8_t* mask, int64_t N, int D, int K, const float* pack,
                             float* r_out, float* logr_out, float* x_fill_out, double* stats_out, double* bound_out, void* ws,
                             size_t ws_bytes, void* stream);
int    vmp_mixture_wfit_iterate(const float* x, const float* w, const uint8_t* mask, int64_t N, int D, int K, const float* alpha0,
                                const float* beta0, const float* m0, const float* C0, const float* v0, float* r, float* logr,
                                float* x_fill, float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S,
                                float* pi, float* pack, double* stats, double* bound, void* ws, size_t ws_bytes, int iterations,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diagonal-covariance mixture fitting on wide rows (csrc/vmp_diagfit.hip): D up to VMP_DIAG_MAX_D = 64, any D; K up to VMP_MAX_K
 * ------------------------------------------------------------------------------------------------
 * Gaussian mixture with one precision per component and coordinate.  pi ~ Dir(alpha0); lambda_kd ~ Gamma(shape a0_k, rate b0_kd);
 * mu_kd | lambda_kd ~ N(m0_kd, (beta0_k lambda_kd)^-1); given z_n = k, x_nd ~ N(mu_kd, 1 / lambda_kd).  The posterior has the same
 * form: theta = (alpha (K), beta (K), m (K,D), a (K), b (K,D)), the prior (alpha0, beta0, m0, a0, b0) likewise; all fp32.
 *   raw moments  Nk = sum_n r_nk,  sx_kd = sum_n r_nk x_nd,  sxx_kd = sum_n r_nk x_nd^2,  xbar = sx / Nk,  NS_kd = sxx_kd - sx_kd^2 / Nk
 *   M-step   alpha_k = alpha0_k + Nk,  beta_k = beta0_k + Nk,  a_k = a0_k + Nk / 2,  m_kd = (beta0_k m0_kd + sx_kd) / beta_k,
 *            b_kd = b0_kd + 1/2 [ NS_kd + (beta0_k Nk / beta_k) (xbar_kd - m0_kd)^2 ];  Nk = 0: the component's prior, no NaN
 *   E-step   lbar_kd = a_k / b_kd,  c_k = psi(alpha_k) - psi(sum alpha) + 1/2 sum_d (psi(a_k) - log b_kd) - D / (2 beta_k),
 *            log rho_nk = c_k - 1/2 sum_d lbar_kd (x_nd - m_kd)^2,   r_nk = softmax_k log rho_nk
 *   bound    = data - kl_pi - sum_kd kl_ng_kd,   data = sum_n logsumexp_k log rho_nk - 1/2 N D log 2 pi,   kl_pi as in "Variational
 *            lower bound",  kl_ng_kd = 1/2 log(beta / beta0) - 1/2 + 1/2 beta0 / beta + 1/2 beta0 lbar_kd (m_kd - m0_kd)^2
 *            + (a - a0) psi(a) - lgamma(a) + lgamma(a0) + a0 (log b_kd - log b0_kd) + a (b0_kd - b_kd) / b_kd
 * Both steps are exact coordinate ascent: the bound of the state after an iteration (theta from the M-step, r from the E-step at
 * that theta) never falls from one iteration to the next.
 * Layouts: pack (K, vmp_mixture_diag_pack_words(D) = 2 D + 1) fp32 = [ m (D) | lbar (D) | c ];  stats (K, 1 + 2 D) fp64 =
 * [ Nk | sx (D) | sxx (D) ].
 *
 * vmp_mixture_diag_pack: the pack from theta, one block per component, fp64 inside, rounded once.  A component with a non-positive
 *   (or NaN) b_kd, a_k or beta_k gets a NaN row.
 * vmp_mixture_diag_pass: one streaming pass over x (N,D) fp32, any alignment, under a pack.  Outputs, all optional but at least
 *   one: r_out (N,K); logr_out (N,K) = log r (needs r_out); stats_out (K, 1 + 2 D) fp64; bound_out (1) fp64 = data.  The moments are
 *   those of the responsibilities the pass itself computes; r_out == NULL is legal and is the fast form of an iteration: the pass
 *   then moves x alone.  r_in (N,K) != NULL replaces the E-part: stats_out are the moments of the caller's responsibilities (how a
 *   loop is started from r_init); r_out, logr_out and bound_out must then be NULL and the pack's values are not read.
 *   log rho is formed on x - m, never in the expanded form.  The moments are accumulated in fp32 on x - p with ONE pivot p near the
 *   data (the mean of up to 64 evenly strided rows, a function of x, N and D alone) in 16-row MFMA groups, added to the wave's own fp64 words every 128
 *   rows of a wave, and a second launch adds the waves in a fixed order and undoes the shift in fp64.  The rows' log-sum-exp (fp32
 *   per row) are added in fp64 in a fixed order - the rows of a lane, the lanes of a wave, the waves of a block, the blocks by block
 *   0 of the second launch.  No atomics, one geometry whichever outputs are requested: stats_out and bound_out are bit-identical
 *   from run to run and with or without r_out / logr_out.  ws (vmp_mixture_diag_workspace_bytes: the fp64 moments of every wave, one
 *   fp64 word per block and the pivot; 8-byte aligned) is always needed.
 * vmp_mixture_diag_finalize: stats + prior -> theta and, each optional, xbar (K,D), S (K,D) = NS / Nk (0 where Nk = 0) and pi (K) =
 *   exp E log pi.  One thread per (k, d), fp64 inside.
 * vmp_mixture_diag_bound_terms: out (2 + K) fp64 = [ kl_pi | sum_kd kl_ng_kd | sum_d kl_ng_0d .. sum_d kl_ng_{K-1}d ]; one thread per
 *   component adds its D terms in d order, one thread adds the components in k order; fp64.
 * vmp_mixture_diag_iterate: `iterations` x (vmp_mixture_diag_finalize on stats -> vmp_mixture_diag_pack -> vmp_mixture_diag_pass with
 *   stats_out = stats, bound_out = bound) enqueued back to back, no host work in between; stats holds the moments of the current r
 *   on entry and of the last r on return.  r and logr, if not NULL, are written by the last pass only.  xbar, S, pi, bound may be NULL.
 * Errors (decided before any launch): VMP_E_DIM (D outside 1..VMP_DIAG_MAX_D, K outside 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x or pack
 *   NULL; no output; logr_out without r_out; r_in together with r_out, logr_out or bound_out; ws not 8-byte aligned; a NULL prior,
 *   posterior or stats of the iteration, the finalize, the pack or the terms; iterations < 0), VMP_E_WS (ws NULL or too small).
 *   vmp_mixture_diag_workspace_bytes and vmp_mixture_diag_pack_words are 0 outside the compiled range.                          */
int    vmp_mixture_diag_pack_words(int D);
size_t vmp_mixture_diag_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_diag_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* a, const float* b,
                             float* pack, void* stream);
int    vmp_mixture_diag_pass(const float* x, int64_t N, int D, int K, const float* pack, const float* r_in, float* r_out,
                             float* logr_out, double* stats_out, double* bound_out, void* ws, size_t ws_bytes, void* stream);
int    vmp_mixture_diag_finalize(const double* stats, int D, int K, const float* alpha0, const float* beta0, const float* m0,
                                 const float* a0, const float* b0, float* alpha, float* beta, float* m, float* a, float* b,
                                 float* xbar, float* S, float* pi, void* stream);
int    vmp_mixture_diag_bound_terms(int D, int K, const float* alpha0, const float* beta0, const float* m0, const float* a0,
                                    const float* b0, const float* alpha, const float* beta, const float* m, const float* a,
                                    const float* b, double* out, void* stream);
int    vmp_mixture_diag_iterate(const float* x, int64_t N, int D, int K, const float* alpha0, const float* beta0, const float* m0,
                                const float* a0, const float* b0, float* r, float* logr, float* alpha, float* beta, float* m,
                                float* a, float* b, float* xbar, float* S, float* pi, float* pack, double* stats, double* bound,
                                void* ws, size_t ws_bytes, int iterations, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diagonal-covariance mixture: fitting partly observed and weighted rows (csrc/vmp_diagmfit.hip): D up to VMP_DIAG_MAX_D, K up to VMP_MAX_K
 * ------------------------------------------------------------------------------------------------
 * The fit of the section above on rows with missing entries (missing at random) and with row weights.  Notation and model are those
 * of that section; o(n) / m(n) are the observed / missing coordinates of row n, D_o(n) = |o(n)|, w_n >= 0 the weight of row n (1
 * without weights), lbar_kd = a_k / b_kd.  The missing entries are latent variables; for the diagonal model the optimum q(x_m | z) is
 * a product of one-dimensional Gaussians, so the posterior keeps its form theta = (alpha, beta, m, a, b) and both updates stay exact
 * coordinate ascent (the bound never falls):
 *   hl_kd      = -1/2 log lbar_kd
 *   log rho_nk = c_k - 1/2 sum_{d in o(n)} lbar_kd (x_nd - m_kd)^2 + sum_{d in m(n)} hl_kd      (c_k as above, over all D)
 *   r_nk       = softmax_k log rho_nk                  a weight does not enter a row's own responsibilities
 *   q(x_nd | z_n = k), d missing:  N(m_kd, 1 / lbar_kd)
 *   Nk     = sum_n w_n r_nk,    M_kd = sum_n w_n r_nk [d in m(n)]
 *   sx_kd  = sum_n w_n r_nk [d in o(n)] x_nd   + M_kd m_kd
 *   sxx_kd = sum_n w_n r_nk [d in o(n)] x_nd^2 + M_kd (m_kd^2 + 1 / lbar_kd)
 *   data   = sum_n w_n ( logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi )
 *   bound  = data - kl_pi - sum_kd kl_ng_kd            (vmp_mixture_diag_bound_terms, unchanged)
 * The M-step is vmp_mixture_diag_finalize, unchanged, on stats (K, 1 + 2 D) = [ Nk | sx | sxx ] of the completed rows.  A row that
 * observes nothing has log rho_nk = c_k + sum_d hl_kd; a column nobody observes stays finite.  A row with w = 0 is removed by a
 * select, not a product: whatever its slots hold (NaN and +-Inf included) reaches neither moments nor data; its r / log r / fill are
 * still written.  What a missing slot of x holds never enters arithmetic.
 * Layout: pack (K, vmp_mixture_diag_mfit_pack_words(D) = 3 D + 1) fp32 = [ m (D) | lbar (D) | hl (D) | c ].
 *
 * vmp_mixture_diag_mfit_pack: the pack from theta, one block per component, fp64 inside, rounded once.  A component with a
 *   non-positive (or NaN) b_kd, a_k or beta_k gets a NaN row.
 * vmp_mixture_diag_mfit_pass: one streaming pass over x (N,D) fp32, any alignment, with an optional mask (N,D) uint8, nonzero =
 *   missing, and optional weights w (N) fp32 (finite, >= 0; the caller's business), under a pack.  mask == NULL is a kernel of its own
 *   that reads and selects nothing of a mask; w == NULL is a wave-uniform test.  Outputs, all optional but at least one: r_out (N,K)
 *   and logr_out (N,K) (needs r_out), both of the unweighted r; x_fill_out (N,D) (needs mask): observed entries copied bit for bit,
 *   missing ones filled with sum_k r_nk m_kd; stats_out (K, 1 + 2 D) fp64; bound_out (1) fp64 = data.  r_out == NULL is the fast form
 *   of an iteration: the pass then moves x, mask and w alone.  The geometry is that of vmp_mixture_diag_pass: the moments of w r are
 *   accumulated in fp32 on x - p by 16-row MFMA groups with ONE pivot p (the mean of the observed entries of up to 64 evenly strided
 *   rows of positive weight: a function of x, mask, w, N and D alone), M_kd by a third MFMA chain on the 0/1 indicator of a missing
 *   entry; added to the wave's own fp64 words every 128 rows; a second launch adds the waves in a fixed order, undoes the shift on
 *   the observed part and completes the missing part in fp64 with the pack's own fp32 m and lbar:
 *     sx = s1 + (Nk - M) p + M m,    sxx = s2 + 2 p s1 + (Nk - M) p^2 + M (m^2 + 1 / lbar).
 *   A row's data term is formed in fp64 from its fp32 log-sum-exp, the integer D_o and the fp32 weight, and added in the fixed order
 *   of vmp_mixture_diag_pass.  No atomics, one geometry for (N, D, K): stats_out and bound_out are bit-identical from run to run and
 *   whichever other outputs are requested.  ws (vmp_mixture_diag_mfit_workspace_bytes: blocks x 4 waves x K (1 + 3 D) fp64 words, one
 *   fp64 word per block and the pivot, blocks = min(512 while K (1 + 3 D) <= 2048 else 256, ceil(N / 2048)); 8-byte aligned) is
 *   always needed.
 * vmp_mixture_diag_mfit_iterate: `iterations` x (vmp_mixture_diag_finalize on stats -> vmp_mixture_diag_mfit_pack ->
 *   vmp_mixture_diag_mfit_pass with stats_out = stats, bound_out = bound) enqueued back to back; stats holds the moments of the
 *   current r on entry.  r, logr and x_fill, if not NULL, are written by the last pass only.  xbar, S, pi, bound may be NULL.
 * Errors (decided before any launch): VMP_E_DIM (D outside 1..VMP_DIAG_MAX_D, K outside 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x or pack
 *   NULL; no output; logr_out without r_out; x_fill_out without mask; ws not 8-byte aligned; a NULL prior, posterior or stats of the
 *   iteration or the pack builder; iterations < 0), VMP_E_WS (ws NULL or too small).  vmp_mixture_diag_mfit_workspace_bytes and
 *   vmp_mixture_diag_mfit_pack_words are 0 outside the compiled range.                                                       */
int    vmp_mixture_diag_mfit_pack_words(int D);
int    vmp_mixture_diag_mfit_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* a, const float* b,
                                  float* pack, void* stream);
size_t vmp_mixture_diag_mfit_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_diag_mfit_pass(const float* x, const uint8_t* mask, const float* w, int64_t N, int D, int K, const float* pack,
                                  float* r_out, float* logr_out, float* x_fill_out, double* stats_out, double* bound_out, void* ws,
                                  size_t ws_bytes, void* stream);
int    vmp_mixture_diag_mfit_iterate(const float* x, const uint8_t* mask, const float* w, int64_t N, int D, int K, const float* alpha0,
                                     const float* beta0, const float* m0, const float* a0, const float* b0, float* r, float* logr,
                                     float* x_fill, float* alpha, float* beta, float* m, float* a, float* b, float* xbar, float* S,
                                     float* pi, float* pack, double* stats, double* bound, void* ws, size_t ws_bytes, int iterations,
                                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diagonal-covariance mixture: scoring and filling wide rows (csrc/vmp_diagscore.hip): D up to VMP_DIAG_MAX_D, K up to VMP_MAX_K
 * ------------------------------------------------------------------------------------------------
 * Log posterior predictive density, predictive responsibilities and conditional-mean fills of rows the posterior theta = (alpha,
 * beta, m, a, b) of the section above was not fitted on, complete or partly observed.  q(lambda_kd) = Gamma(a_k, rate b_kd) and
 * q(mu_kd | lambda_kd) = N(m_kd, (beta_k lambda_kd)^-1) are independent over d, so given z = k the predictive of a row is a product
 * of one-dimensional Student-t densities with 2 a_k degrees of freedom and location m_kd; marginalising a missing coordinate leaves
 * its factor out, and its conditional mean is the responsibility-weighted location.
 *   g_kd  = beta_k / (2 b_kd (1 + beta_k)),   G_k = lgamma(a_k + 1/2) - lgamma(a_k) - 1/2 log pi
 *   log St_kd(x) = G_k + 1/2 log g_kd - (a_k + 1/2) log1p(g_kd (x - m_kd)^2)
 *   log w_k = log(alpha_k / sum_j alpha_j)            (the weights of vmp_mix_score_pack_niw)
 *   l_nk  = log w_k + sum_{d in o(n)} log St_kd(x_nd)     o(n) = the observed coordinates of row n; without a mask all D
 *   logp_n = logsumexp_k l_nk,   resp_nk = exp(l_nk - logp_n)
 *   xhat_nd = sum_k resp_nk m_kd  for d missing       (the conditional mean when a_k > 1/2, the conditional location otherwise;
 *                                                      returned either way, as vmp_mixture_impute does)
 * a_k grows like N_k / 2 while g_kd (x - m)^2 shrinks like 1 / N_k: the kernel's log1p is accurate relative to its argument (four
 * cells are merged as (1 + T)(1 + t) - 1 = T + t + T t, then log1p(T) = log u + (T - (u - 1)) / u with u = fl(1 + T)), and x - m is
 * formed directly, never expanded.
 * Layout: pack (K, vmp_mixture_diag_score_pack_words(D) = 3 D + 3) fp32 = [ m (D) | g (D) | h (D) | log w | a + 1/2 | c ] with
 * h_kd = G_k + 1/2 log g_kd and c_k = log w_k + sum_d h_kd.
 *
 * vmp_mixture_diag_score_pack: the pack from theta, one block per component, fp64 inside, rounded once.  A component with a
 *   non-positive (or NaN) alpha_k, beta_k, a_k or b_kd gets a NaN row.
 * vmp_mixture_diag_score: one streaming pass over x (N,D) fp32, any alignment, with an optional mask (N,D) uint8, nonzero = missing;
 *   mask == NULL is a kernel of its own that reads and selects nothing.  Outputs, all optional but at least one: logp_out (N);
 *   resp_out (N,K); x_out (N,D) - needs a mask; observed entries copied bit for bit, missing ones filled with xhat; x_out == x fills
 *   in place; sum_out (1) fp64 = sum_n logp_n, the rows added in fp64 in a fixed order - the rows of a lane, the lanes of a wave, the
 *   waves of a block, then the blocks' partials (in ws) by a one-wave second launch.  No atomics; the geometry depends on N alone:
 *   every output has the same bits from run to run and whichever other outputs are requested.
 *   What a missing slot of x holds (NaN and +-Inf included) never enters arithmetic.  A row with nothing observed has l_nk = log w_k.
 *   log w_k = -inf (a hand-made pack) gives resp_k = 0; if every log w is -inf: logp = -inf, resp = 0, fills 0, no NaN.  A NaN pack
 *   row makes every row's logp NaN.
 * vmp_mixture_diag_score_workspace_bytes = 8 * blocks,  blocks = min(2048, max(1, ceil(N / 1024))): one fp64 partial per block; a
 *   multiple of 8, non-decreasing in N, 0 outside the compiled range.  ws is needed only with sum_out.
 * Errors (decided before any launch): VMP_E_DIM (D outside 1..VMP_DIAG_MAX_D, K outside 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x or pack
 *   NULL; no output; x_out without mask; ws not 8-byte aligned when sum_out is given; a NULL operand of the pack builder), VMP_E_WS
 *   (ws NULL or too small when sum_out is given).  vmp_mixture_diag_score_pack_words is 0 outside 1..VMP_DIAG_MAX_D.             */
int    vmp_mixture_diag_score_pack_words(int D);
int    vmp_mixture_diag_score_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* a,
                                   const float* b, float* pack, void* stream);
size_t vmp_mixture_diag_score_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_diag_score(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* logp_out,
                              float* resp_out, float* x_out, double* sum_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture initialisation (csrc/vmp_seed.hip): seeded k-means++ centres and the responsibilities of the nearest centre, on the device
 * ------------------------------------------------------------------------------------------------
 * D^2-seeding (Arthur & Vassilvitskii 2007) of K centres from the rows of x (N,D) fp32, any alignment, as a pure function of (seed,
 * row index, round); optional mask (N,D) uint8, nonzero = missing, with fill (D) fp32, the value a centre takes in a coordinate its
 * row does not have.  What a missing slot of x holds never enters arithmetic (NaN and +-Inf there are as good as 0).
 *   o(n) the observed coordinates of row n, D_o(n) their number (without a mask: all D);  x~_n = row n with fill in its missing slots;
 *   dist2(n, c) = (D / D_o(n)) sum_{i in o(n)} (x_ni - c_i)^2,  0 when D_o(n) = 0     (the partial-distance rule).
 * Rounds j = 0 .. K-1; before round 0 the weight is w_n = 1 if D_o(n) > 0, else 0:
 *   1. E_nj = -log u(seed, n, j);
 *   2. s_n = E_nj / w_n, +inf where w_n = 0;
 *   3. i_j = the row with the smallest s_n, ties to the lowest n (every s_n = +inf: row 0);
 *   4. c_j = x~_{i_j};
 *   5. w_n <- dist2(n, c_0) after round 0,  w_n <- min(w_n, dist2(n, c_j)) after every later round.
 * An exponential race: row n wins with probability w_n / sum w - exact D^2-sampling; round 0 is a uniform draw over the rows that
 * observe something.  The uniform is drawn as in "Mixture sampling": Philox4x32-7 (oracle/philox.py philox4x32), key = seed,
 * counter = (n low, n high, j, 0x6b6d2b00), word 0, u = (top 24 bits + 1/2) 2^-24 rounded once to fp32 and kept at most 1 - 2^-24.
 * The fourth counter word differs from every other one of csrc/: 0 (cell noise), 0x5bb5a3c1 (categorical draw), 0x6d78a500 + b (sampling).
 * Assignment: z_n = the k with the smallest dist2(n, c_k), ties to the lowest k;  r_nk = (1 - smooth) [k = z_n] + smooth / K in
 * fp32 (the one-hot entry is (1 - smooth) + smooth / K), 0 <= smooth < 1;  a row with D_o(n) = 0 gets z = -1 and r = 1 / K.
 * The pick is a lexicographic minimum of (s, n): it does not depend on grid, block or wave geometry; no atomics; every output is
 * bit-identical from run to run and whichever optional outputs are requested.
 *
 * vmp_mixture_seed_centers: centers_out (K,D) = c_j (the bits of x~ at the chosen rows); index_out (K) int64 = i_j or NULL;
 *   mind2_out (N) = w after the last round, or NULL.  N < K is legal: the centres then repeat.  ONE call enqueues K + 1 launches back
 *   to back, no host work in between: launch j = 0 .. K first reduces the per-block minima of launch j - 1 to i_{j-1} (every block
 *   the same reduction), reads c_{j-1} from x, and then streams the rows once - w is updated with c_{j-1} and, for j < K, the
 *   block's minimum of round j is left in ws; launch K without mind2_out is one block.  w lives in ws
 *   (vmp_mixture_seed_workspace_bytes, 8-byte aligned): per row a round reads x, the mask and w and writes w.
 * vmp_mixture_seed_assign: one launch; r_out (N,K), z_out (N) int32 or NULL; mask as above or NULL; no workspace.
 * Errors (decided before any launch): VMP_E_DIM (D, K outside 1..VMP_MAX_D / 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x, centers_out,
 *   centers or r_out NULL; exactly one of mask and fill NULL; smooth outside [0, 1) or NaN; ws not 8-byte aligned), VMP_E_WS (ws NULL
 *   or too small).                                                                                                          */
size_t vmp_mixture_seed_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_seed_centers(const float* x, const uint8_t* mask, const float* fill, int64_t N, int D, int K, uint64_t seed,
                                float* centers_out, int64_t* index_out, float* mind2_out, void* ws, size_t ws_bytes, void* stream);
int    vmp_mixture_seed_assign(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* centers, float smooth,
                               float* r_out, int32_t* z_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diagonal-covariance mixture: seeded start on wide rows (csrc/vmp_diagseed.hip): the k-means++ centres and the nearest-centre
 * responsibilities of "Mixture initialisation" for complete rows of D in 1..VMP_DIAG_MAX_D columns, K in 1..VMP_MAX_K
 * ------------------------------------------------------------------------------------------------
 * The mathematics of "Mixture initialisation" without a mask and without `fill`: dist2(n, c) = sum_d (x_nd - c_d)^2 in fp32 on the
 * difference x - c, in d order (never the expanded form); the same uniform (Philox4x32-7, key = seed, counter (n low, n high, j,
 * 0x6b6d2b00), word 0, the same u -> fp32 rule), the same exponential race, the same lexicographic (s, n) pick, round 0 uniform
 * over all rows, N < K legal (the centres then repeat).  For D <= VMP_MAX_D the arithmetic is that of vmp_mixture_seed_centers with
 * mask == NULL: both pick the same rows.
 * x (N,D) fp32, any alignment: a 64-row tile goes to the wave's LDS with coalesced dword loads, lane = row afterwards; the centre of
 * a round is read from x itself as a wave-uniform scalar operand.
 *
 * vmp_mixture_diag_seed_centers: centers_out (K,D) = the bits of x at the chosen rows; index_out (K) int64 = i_j or NULL; mind2_out
 *   (N) = w after the last round, or NULL.  ONE call enqueues K + 1 launches back to back, no host work and no host synchronisation
 *   in between: launch j = 0 .. K first reduces the per-block minima of launch j - 1 to i_{j-1} (every block the same reduction: no
 *   atomics), reads c_{j-1} from x and then streams the rows once - w <- min(w, dist2(., c_{j-1})) and, for j < K, the block's
 *   minimum of round j is left in ws; launch 0 reads no x, launch K without mind2_out is one block.  w lives in ws: per row a round
 *   reads x and w and writes w.  The geometry depends on (N, D) only: every output is bit-identical from run to run and whichever
 *   optional outputs are requested.
 * vmp_mixture_diag_seed_assign: one launch; z_out (N) int32 = the k with the smallest dist2(n, c_k), ties to the lowest k, or NULL;
 *   r_out (N,K) = (1 - smooth) [k = z_n] + smooth / K in fp32 (the one-hot entry is (1 - smooth) + smooth / K), or NULL; at least one
 *   of the two.  No workspace.
 * vmp_mixture_diag_seed_workspace_bytes = w (N) fp32 padded to 16 bytes + the double-buffered candidates (2, blocks) x (int64, fp32)
 *   padded to 16 bytes, blocks = min(D > 32 ? 512 : 1024, ceil(N / 1024)): a multiple of 8, non-decreasing in N, 0 outside the
 *   compiled range (and for N < 1).
 * Errors (decided before any launch): VMP_E_DIM (D outside 1..VMP_DIAG_MAX_D, K outside 1..VMP_MAX_K), VMP_E_BADARG (N < 1; x,
 *   centers_out or centers NULL; r_out and z_out both NULL; smooth outside [0, 1) or NaN; ws not 8-byte aligned), VMP_E_WS (ws NULL
 *   or too small).                                                                                                          */
size_t vmp_mixture_diag_seed_workspace_bytes(int64_t N, int D, int K);
int    vmp_mixture_diag_seed_centers(const float* x, int64_t N, int D, int K, uint64_t seed, float* centers_out, int64_t* index_out,
                                     float* mind2_out, void* ws, size_t ws_bytes, void* stream);
int    vmp_mixture_diag_seed_assign(const float* x, int64_t N, int D, int K, const float* centers, float smooth, float* r_out,
                                    int32_t* z_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T2: SVAE E-step fused with the ELBO regulariser (models/svae.py:14-119 and :229-252)
 * ------------------------------------------------------------------------------------------------
 * Per (n,k) cell:  Pt = diag(-2 eta2d_n) + P_k,  ht = eta1_n + h_k,  Lt = chol(Pt),
 *   log_z_nk  = normalise_k( bias_k + 1/2 |Lt^-1 ht|^2 - sum_i log Lt_ii )        compute_log_z_given_y, svae.py:50-92
 *   x_nks     = Lt^-T (Lt^-1 ht + eps_nks)                                         sample_x_per_comp,     svae.py:95-119
 *   T'_nk     = mean_s[ log N(x_s; phi~_nk) - log N(x_s; theta_k) - E log pi_k ]   the two per-sample densities of
 *               compute_elbo (svae.py:236-243; gaussian.py:74-105) in closed form, so that
 *               regulariser = sum_nk exp(log_z_nk) (T'_nk + log_z_nk)               (svae.py:245-252)
 * Inputs: eta1, eta2d (N,L) encoder outputs; hk (K,L), Pk (K,L,L) symmetric, bias (K) = B_k + log pi_k from
 * unpack_recognition_gmm (svae.py:342-358); noise (N,K,L,S) replaces tf.random_normal (svae.py:114);
 * theta side: log p(x, z=k | theta) = kappa_k - 1/2 |W_k (x - m_k)|^2 with W_k (K,L,L) LOWER triangular,
 * W^T W = E[Sigma_k]^-1, kappa_k = sum log W_ii - L/2 log 2pi + E log pi_k (GMM theta, svae.py:205-214, no gradient);
 * with nu != NULL the Student-t of compute_elbo_smm (svae.py:265-322, student_t.py:31-37):
 * kappa_k - 1/2 (nu_k + L) log1p(|W_k (x - m_k)|^2 / nu_k), W = chol(Sigma_k)^-1, kappa_k = lgamma terms - sum log L_ii
 * + E log pi_k (mu_k, L_k trainable: experiments.py:160-161).  Outputs: x (N,K,S,L), lz (N,K), Tp (N,K).     */
int    vmp_svae_estep_fwd(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                          const float* noise, const float* mk, const float* Wk, const float* kappa, const float* nu,
                          int64_t N, int K, int L, int S, float* x, float* lz, float* Tp, void* stream);
/* In-kernel noise (models/svae.py:113-114 draws eps inside the step: tf.random_normal, i.e. TensorFlow's Philox stream).
 * Same operation with eps generated where it is consumed: Philox4x32-7 (Random123's philox4x32 at 7 rounds) keyed by `seed`,
 * counter = (cell low, cell high, block, 0), cell = n K + k, block b = (s >> 1) ceil(L/4) + j -> four Box-Muller pairs, one per
 * 32-bit word (radius uniform from the word's top 20 bits, angle from its low 12): (eps[i,s], eps[i,s+1]) for i = 4j .. 4j+3 of
 * the cell's (L,S) noise block (csrc/vmp_svae.hip, oracle/philox.py).  No (N,K,L,S) tensor is read or written; the backward pass needs
 * none (it works from the saved samples x).  Shapes outside the in-kernel path (vmp_svae_rng_in_kernel == 0: L < 8 and L*S
 * not a multiple of 4 or a cell tile larger than the LDS; L = 8 is covered for every S) materialise the same stream in `noise_ws` (N,K,L,S) first.
 * vmp_svae_philox_noise writes that stream as a tensor (tests; callers that want to keep the draw).               */
int    vmp_svae_rng_in_kernel(int K, int L, int S);
int    vmp_svae_philox_noise(uint64_t seed, int64_t N, int K, int L, int S, float* noise, void* stream);
int    vmp_svae_philox_noise_dev(const uint64_t* seed_dev, int64_t N, int K, int L, int S, float* noise, void* stream);   /* key from a device word */
int    vmp_svae_estep_fwd_rng(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                              uint64_t seed, const float* mk, const float* Wk, const float* kappa, const float* nu,
                              int64_t N, int K, int L, int S, float* x, float* lz, float* Tp, float* noise_ws, void* stream);
/* Row offset (walking a large set in chunks): row n of the launch draws the stream of GLOBAL row row0 + n - the Philox cell id is
 * (row0 + n) K + k - so a chunk [row0, row0 + N) of a set gets exactly the noise it gets in one launch over the whole set.
 * vmp_svae_philox_noise_at == rows [row0, row0 + N) of vmp_svae_philox_noise, bit for bit.  vmp_svae_estep_fwd_rng_at is
 * vmp_svae_estep_fwd_rng (same shapes, noise_ws for those outside the in-kernel path) except that it always runs the streaming
 * kernels, never the one-block-per-tile minibatch form (whose T' sums in another order): x, lz and T' of a row are bit-identical
 * whatever the launch's N and row0 split.  row0 >= 0.                                                                  */
int    vmp_svae_philox_noise_at(uint64_t seed, int64_t row0, int64_t N, int K, int L, int S, float* noise, void* stream);
int    vmp_svae_estep_fwd_rng_at(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                                 uint64_t seed, int64_t row0, const float* mk, const float* Wk, const float* kappa,
                                 const float* nu, int64_t N, int K, int L, int S, float* x, float* lz, float* Tp,
                                 float* noise_ws, void* stream);
/* The same with the key read from a DEVICE word at execution time (in-kernel shapes only, vmp_svae_rng_in_kernel != 0): a
 * launch captured in a HIP graph draws fresh noise on every replay once the caller refreshes *seed_dev.            */
int    vmp_svae_estep_fwd_rng_dev(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                                  const uint64_t* seed_dev, const float* mk, const float* Wk, const float* kappa,
                                  const float* nu, int64_t N, int K, int L, int S, float* x, float* lz, float* Tp,
                                  void* stream);
/* The in-kernel-noise E-step with the step's next three operations done in its epilogue, while a cell's values are in
 * registers (in-kernel shapes only; key = `seed`, or *seed_dev when seed_dev != NULL):
 *   x_samples (N,L) = subsample_x(x, lz) with ONE draw per row (models/svae.py:122-151 as its caller uses it, svae.py:514:
 *                     z_n ~ Cat(exp lz_n), x_samples[n] = x[n, z_n, 0, :]) - bit-identical to vmp_svae_subsample_rng with the same
 *                     key and S_out = 1 (same uniforms, same inverse-CDF arithmetic);
 *   r (N,K)         = exp(lz) (svae.py:216; may be NULL);
 *   mom             = per-block fp64 partials of the M-step's raw moments sum_n r_nk [x_n | 1 | x_n x_n^T lower-packed | 0 0 0]
 *                     with x_n = x_samples[n] (svae.m_step -> gmm.update_Nk/xk/Sk, svae.py:154-176, gmm.py:25-46), laid out
 *                     (vmp_svae_fwd_mom_blocks(N,K,L,S), 16, 48); NULL = not wanted.  Exists for K = 16, L = 8
 *                     (vmp_svae_fwd_mom_blocks returns 0 otherwise: use vmp_mix_stats on x_samples and r).
 * vmp_svae_mom_cvi adds the partials in a fixed order into stats_out (K, 2+L+L*L) fp64 (vmp_mix_stats layout; may be NULL when
 * theta is given) and, when t_alpha != NULL, applies vmp_svae_cvi_update from them in the same launch.                    */
int    vmp_svae_fwd_mom_blocks(int64_t N, int K, int L, int S);
int    vmp_svae_estep_fwd_rng_epi(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                                  uint64_t seed, const uint64_t* seed_dev, const float* mk, const float* Wk, const float* kappa,
                                  const float* nu, int64_t N, int K, int L, int S, float* x, float* lz, float* Tp,
                                  float* x_samples, float* r, double* mom, size_t mom_bytes, void* stream);
int    vmp_svae_mom_cvi(const double* mom, int nblk, const float* p_alpha, const float* p_A, const float* p_b,
                        const float* p_beta, const float* p_vhat, float* t_alpha, float* t_A, float* t_b, float* t_beta,
                        float* t_vhat, float* s_alpha, float* s_A, float* s_b, float* s_beta, float* s_vhat,
                        const float* rho_dev, float rho, int K, int L, double* stats_out, void* stream);

/* Backward of the above: given dLoss/dx (N,K,S,L) (from the decoder), dLoss/dlog_z (N,K), dLoss/dT' (N,K), writes
 * dLoss/deta1, dLoss/deta2d (N,L) and per-block partial sums over n of dLoss/d{hk, Pk, bias}:
 * partials (vmp_svae_bwd_blocks(N,K), K, vmp_svae_bwd_partial_words(L)) = [ g_hk (L) | g_Pk lower triangle of the
 * symmetric gradient, row-major packed (L(L+1)/2) | g_bias | g_mk (L) | g_Wk lower packed | g_kappa ] (the last three
 * are zero except g_kappa unless nu != NULL); the caller sums them over the first axis.
 * Replaces TF autodiff through svae.py:50-119 and gaussian.py:74-105 (opt.compute_gradients, experiments.py:232). */
int    vmp_svae_bwd_partial_words(int L);
int    vmp_svae_bwd_blocks(int64_t N, int K);
size_t vmp_svae_workspace_bytes(int64_t N, int K, int L);
int    vmp_svae_estep_bwd(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                          const float* mk, const float* Wk, const float* nu, const float* x, const float* lz,
                          const float* Gx, const float* Glz, const float* GT, int64_t N, int K, int L, int S,
                          float* g_eta1, float* g_eta2d, float* partials, size_t partial_bytes, void* stream);
/* The same with the number of partial rows stated by the caller (round 6).  nblk = vmp_svae_bwd_blocks_for(N, K, L, S, nu != NULL)
 * selects the launch geometry of that query: at minibatch sizes (the reference's operating point, experiments.py:26) and a
 * Gaussian theta that is one block per tile of 64 / K rows with one wave per sample pair - one partial row per TILE instead of
 * per 4-wave block; nblk = vmp_svae_bwd_blocks(N, K) is vmp_svae_estep_bwd.  The caller reduces exactly nblk rows.     */
int    vmp_svae_bwd_blocks_for(int64_t N, int K, int L, int S, int student);
int    vmp_svae_estep_bwd_n(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                            const float* mk, const float* Wk, const float* nu, const float* x, const float* lz,
                            const float* Gx, const float* Glz, const float* GT, int64_t N, int K, int L, int S,
                            float* g_eta1, float* g_eta2d, float* partials, size_t partial_bytes, int nblk, void* stream);
/* Host query, no launch and no device: the launch plan of the E-step kernels (fwd_plan / bwd_plan, csrc/vmp_svae.hip) for N rows.
 * dir 0, forward: f0 = rng (in-kernel noise; 0: a noise tensor), f1 = the noise tensor is 16-byte aligned, f2 = in-kernel moments
 * wanted (vmp_svae_estep_fwd_rng_epi with mom != NULL), f3 = the minibatch form may be used (0: vmp_svae_estep_fwd_rng_at).
 *   out = [form: 0 none (no in-kernel-noise form / no in-kernel moments for the shape), 1 fwd1 (minibatch: one block per tile),
 *   2 tile, 3 pst (per-pair staging), 4 pst2 (two pairs per flush), 5 chunked, 6 fwd3 (register-staged) | waves per block | blocks |
 *   dynamic LDS bytes | cs: the LDS tile's cell stride (chunked: samples per chunk) | 0 | 0 | 0].
 * dir 1, backward: f0 = Student-t theta, f1 = x and dLoss/dx are 16-byte aligned, f2 = nblk, the rows of the caller's partial
 * buffer (0: what vmp_svae_bwd_blocks_for answers), f3 = 0.
 *   out = [form: 0 none (nblk is neither vmp_svae_bwd_blocks_for nor vmp_svae_bwd_blocks), 1 bwd1 (minibatch: one block per tile),
 *   2 ring, 3 generic, one tile per wave, 4 generic, streaming | partial rows | 1 when the form with the ELBO tail inside
 *   (vmp_svae_estep_bwd_tail, or _tail_t for f0 = 1) covers the shape | 0 ...].
 * Returns 0, or with out zeroed: VMP_E_BADARG (out NULL, no such dir, N < 1, S < 1, a flag outside 0 / 1, nblk < 0, f3 != 0 for
 * dir 1), VMP_E_DIM (K, L outside the compiled range, S > 65536) - the sizes the entry points refuse.                        */
int    vmp_svae_launch_plan(int dir, int64_t N, int K, int L, int S, int f0, int f1, int f2, int f3, int64_t* out);

/* subsample_x (models/svae.py:122-151): z_ns ~ Cat(exp lz_n) and x_samples[n,s,:] = x[n, z_ns, s, :] for s < S_out
 * (the reference draws all S and keeps s = 0, svae.py:514).  The draw is the inverse CDF of the supplied uniform
 * u (N,S_out) - replacing tf.multinomial - or the supplied index z (N,S_out) when z != NULL.  out (N,S_out,L).  */
int    vmp_svae_subsample(const float* x, const float* lz, const float* u, const int64_t* z, int64_t N, int K, int S,
                          int L, int S_out, float* out, int64_t* z_out, void* stream);
/* The same with the uniforms drawn in the kernel: u_ns = top 24 bits of word 0 of Philox4x32-7(key = seed, counter =
 * (n low, n high, s, 0x5bb5a3c1)) * 2^-24 - a stream apart from the E-step's normals (whose counter word 3 is 0).  The key
 * is `seed`, or *seed_dev when seed_dev != NULL (graph-captured steps).                                              */
int    vmp_svae_subsample_rng(const float* x, const float* lz, uint64_t seed, const uint64_t* seed_dev, int64_t N, int K,
                              int S, int L, int S_out, float* out, int64_t* z_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K-sized parameter maps of the training step, one launch each (one thread per component, fp64 inside)
 * ------------------------------------------------------------------------------------------------
 * vmp_svae_phi_prep_fwd : svae.unpack_recognition_gmm (svae.py:342-358) + the k-only part of compute_log_z_given_y
 *   (svae.py:70-92):  L_k = tril(L_raw), softplus on the diagonal;  P_k = L_k L_k^T (= -2 eta2);
 *   bias_k = -1/2 |L_k^-1 mu_k|^2 + sum_i log (L_k)_ii + log softmax(pi_raw)_k  - the inputs of vmp_svae_estep_fwd.
 * vmp_svae_phi_prep_bwd : its adjoint: (g_hk, g_P (w.r.t. the full matrix), g_bias) -> gradients w.r.t. the three
 *   'phi_gmm' variables (what TF's autodiff does through tril / softplus / matmul / matrix_solve / softmax).
 * vmp_svae_theta_pack   : theta side of compute_elbo (svae.py:205-214): niw.natural_to_standard + expected_values
 *   (niw.py:8-43), dirichlet.expected_log_pi (dirichlet.py:8-22) -> m_k, W_k = chol(E[Sigma_k])^-1 (lower),
 *   kappa_k = sum_i log W_ii - L/2 log 2pi + E log pi_k   (no gradient: stop_gradient in the reference).
 * vmp_svae_cvi_update   : svae.m_step in natural parameters (svae.py:154-176 = prior + raw moments, +1 on v_hat,
 *   SURVEY appendix A.6) and update_gmm_params (svae.py:376-403): theta <- (1-rho) theta + rho theta*, in place;
 *   theta* is also written when the s_* pointers are given.  stats = vmp_mix_stats layout (fp64).
 *   rho_dev != NULL reads the step size from device memory (graph-captured steps).                            */
int    vmp_svae_phi_prep_fwd(const float* mu_k, const float* L_raw, const float* pi_raw, int K, int L, float* Lk,
                             float* P, float* bias, void* stream);
int    vmp_svae_phi_prep_bwd(const float* mu_k, const float* L_raw, const float* pi_raw, const float* g_hk,
                             const float* g_P, const float* g_bias, int K, int L, float* g_mu, float* g_Lraw,
                             float* g_piraw, void* stream);
/* Fixed-order fp64 reduction of vmp_svae_estep_bwd's per-block partials into the K-sized gradients: g_hk (K,L),
 * g_P (K,L,L, symmetric), g_bias (K) and - Student-t theta only, else NULL - g_mk (K,L), g_W (K,L,L, lower), g_kappa (K). */
int    vmp_svae_bwd_reduce(const float* partials, int nblk, int K, int L, float* g_hk, float* g_P, float* g_bias,
                           float* g_mk, float* g_W, float* g_kappa, void* stream);
int    vmp_svae_theta_pack(const float* alpha, const float* A, const float* b, const float* beta, const float* v_hat,
                           int K, int L, float* m, float* W, float* kappa, void* stream);
/* vmp_svae_phi_prep_fwd and vmp_svae_theta_pack (independent K-sized maps, both run once per training step) in ONE launch. */
int    vmp_svae_prep_fwd(const float* mu_k, const float* L_raw, const float* pi_raw, const float* alpha, const float* A,
                         const float* b, const float* beta, const float* v_hat, int K, int L, float* Lk, float* P,
                         float* bias, float* m, float* W, float* kappa, void* stream);
/* Small batches (N <= 512 rows: the reference's minibatches), one process: the M-step moments of (x_samples (N,L), r (N,K))
 * - exactly vmp_mix_stats' small-batch sums, written to stats_out (K, 2+L+L*L) fp64 - and vmp_svae_cvi_update from them in
 * ONE launch.  Arguments as vmp_svae_cvi_update.                                                                      */
int    vmp_svae_stats_cvi(const float* x_samples, const float* r, int64_t N, const float* p_alpha, const float* p_A,
                          const float* p_b, const float* p_beta, const float* p_vhat, float* t_alpha, float* t_A,
                          float* t_b, float* t_beta, float* t_vhat, float* s_alpha, float* s_A, float* s_b, float* s_beta,
                          float* s_vhat, const float* rho_dev, float rho, int K, int L, double* stats_out, void* stream);
int    vmp_svae_cvi_update(const double* stats, const float* p_alpha, const float* p_A, const float* p_b,
                           const float* p_beta, const float* p_vhat, float* t_alpha, float* t_A, float* t_b,
                           float* t_beta, float* t_vhat, float* s_alpha, float* s_A, float* s_b, float* s_beta,
                           float* s_vhat, const float* rho_dev, float rho, int K, int L, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction term (models/vae.py:201-250, weights branch :233-248)
 * ------------------------------------------------------------------------------------------------
 * A_nk = sum_{s,d} [ (y_nd - mean_nksd)^2 / var_nksd + log(var_nksd + 1e-8) ]   -- the tensor the reference
 * contracts with the responsibilities in einsum('nksd,nk->') (vae.py:240).  y (N,Dy); mean, var (N,K,S,Dy).
 * Backward: gmean = gA_nk * d/dmean, gvar = gA_nk * d/dvar (same shapes as mean / var).                        */
/* eps: the reference adds 1e-8 inside the log in the weights branch (vae.py:240) and nothing in the plain-VAE branch
 * (weights=None, vae.py:225; call with K = 1, means (M,1,S,L)).                                                    */
int    vmp_diag_gauss_loglike_fwd(const float* y, const float* mean, const float* var, int64_t N, int K, int S,
                                  int Dy, float eps, float* A, void* stream);
int    vmp_diag_gauss_loglike_bwd(const float* y, const float* mean, const float* var, const float* gA,
                                  int64_t N, int K, int S, int Dy, float eps, float* gmean, float* gvar, void* stream);

/* Bernoulli decoder: rows_nks = sum_d m_nd * ( -log(1 + exp(-logit_nksd * y_nd)) ), y in {-1,+1},
 * m = 1 or the missing-data mask (N,D) - the per-sample-row part of vae.expected_bernoulli_loglike
 * (models/vae.py:175-198) and losses.bernoulli_logprob (losses.py:41-80).  logits (N,K,S,D); rows, g_rows (N,K,S).   */
int    vmp_bernoulli_rows_fwd(const float* y, const float* logits, const uint8_t* mask, int64_t N, int K, int S, int D,
                              float* rows, void* stream);
int    vmp_bernoulli_rows_bwd(const float* y, const float* logits, const uint8_t* mask, const float* g_rows, int64_t N,
                              int K, int S, int D, float* g_logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused decoder MLP + reconstruction term (models/vae.py:75-128 make_nnet, :138-151 make_decoder, :233-248)
 * ------------------------------------------------------------------------------------------------
 * The decoder the SVAE driver builds (experiments.py:140: [(U,tanh),(U,tanh),(Dy,'standard')]) applied to the
 * N*K*S sample rows x (N,K,S,L), fused with the per-row part of vae.expected_diagonal_gaussian_loglike:
 *   h0 = tanh(x W0 + b0), h1 = tanh(h0 W1 + b1), [raw1|raw2] = h1 W2 + b2            (vae.py:17-25, 86-93)
 *   mean = raw1 + x Ws + bs1,  var = softplus(raw2) + log1p(exp(bs2))                 (vae.py:28-49, 97-116)
 *   ll_nks = sum_d [ (y_nd - mean_d)^2 / var_d + log(var_d + 1e-8) ]                  (vae.py:236-240)
 * so that A_nk of vmp_diag_gauss_loglike_fwd = sum_s ll_nks, without the (rows x U) activations or the
 * (N,K,S,Dy) decoder outputs ever reaching HBM.  fp32 MFMA (v_mfma_f32_16x16x4_f32), L, Dy <= 8, U <= 64.
 * Parameters in the reference's variable layout: W0 (L,U) 'layer_0/kernel', b0 (U), W1 (U,U), b1 (U),
 * W2 (U,2Dy) 'gaussian_output/kernel', b2 (2Dy), Ws (L,Dy) 'shortcut/W', bs1 (Dy) 'shortcut/b1', bs2 (Dy).
 *   fwd: ll (N,K,S) and/or (mean, var) (N,K,S,Dy) - either may be NULL (K = S = 1 gives the plain decoder);
 *        y may be NULL when ll is.
 *   bwd: given gA (N,K) = dLoss/dA_nk writes dx (N,K,S,L) and the flat parameter gradient
 *        dparams [W0|b0|W1|b1|W2|b2|Ws|bs1|bs2] (vmp_decoder_param_words floats); deterministic.  With ll != NULL
 *        the same pass also writes ll (N,K,S) - value and gradient from one launch, for callers that know gA
 *        beforehand (the ELBO's dLoss/dA_nk = r_nk / 2S does not depend on the decoder).                     */
int    vmp_decoder_param_words(int L, int U, int Dy);
size_t vmp_decoder_workspace_bytes(int64_t N, int K, int S, int L, int U, int Dy);
int    vmp_decoder_loglike_fwd(const float* x, const float* y, const float* W0, const float* b0, const float* W1,
                               const float* b1, const float* W2, const float* b2, const float* Ws, const float* bs1,
                               const float* bs2, int64_t N, int K, int S, int L, int Dy, int U, float* ll, float* mean,
                               float* var, void* stream);
/* Backward pass of the same network as a stand-alone Gaussian-head MLP (the encoder, vae.make_encoder
 * models/vae.py:131-135; forward = vmp_decoder_loglike_fwd with ll == NULL, K = S = 1): the upstream gradients of the two
 * head outputs (mean, var) are inputs.  x (R,L); gmean, gvar (R,Dy); dx (R,L) may be NULL (x is data).        */
int    vmp_mlp_gauss_bwd(const float* x, const float* gmean, const float* gvar, const float* W0, const float* b0,
                         const float* W1, const float* b1, const float* W2, const float* b2, const float* Ws,
                         const float* bs1, const float* bs2, int64_t R, int L, int Dy, int U, float* dx, float* dparams,
                         void* ws, size_t ws_bytes, void* stream);
/* The same MLP with either Gaussian head of models/vae.py:28-50 (make_gaussian_layer): outputs (out1, out2) =
 * (mean, var_scale * var) - var_scale = 1: 'standard' (mean, softplus), var_scale = -1/2: the encoder's 'natparam' head
 * (eta1, -1/2 softplus) of experiments.py:139 - so that the head's scaling costs no launch of its own, forward or
 * backward (g_out2 is the upstream gradient of out2).  x (R,L); out1, out2, g_out1, g_out2 (R,Dy).              */
int    vmp_mlp_gauss_head_fwd(const float* x, const float* W0, const float* b0, const float* W1, const float* b1,
                              const float* W2, const float* b2, const float* Ws, const float* bs1, const float* bs2,
                              int64_t R, int L, int Dy, int U, float var_scale, float* out1, float* out2, void* stream);
int    vmp_mlp_gauss_head_bwd(const float* x, const float* g_out1, const float* g_out2, float var_scale, const float* W0,
                              const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                              const float* Ws, const float* bs1, const float* bs2, int64_t R, int L, int Dy, int U,
                              float* dx, float* dparams, void* ws, size_t ws_bytes, void* stream);
int    vmp_decoder_loglike_bwd(const float* x, const float* y, const float* gA, const float* W0, const float* b0,
                               const float* W1, const float* b1, const float* W2, const float* b2, const float* Ws,
                               const float* bs1, const float* bs2, int64_t N, int K, int S, int L, int Dy, int U,
                               float* dx, float* dparams, float* ll, void* ws, size_t ws_bytes, void* stream);
/* As vmp_decoder_loglike_bwd with the upstream gradient given through LOG weights: gA_nk = w_scale * exp(log_w_nk).  The
 * ELBO's weights are r_nk = exp(log z_nk) (models/svae.py:216-219, vae.py:240): with w_scale = -sigma / 2S the launch
 * returns sigma * d rec / d(x, parameters) without a separate exp / scaling pass over (N,K).  w_scale != 0.          */
int    vmp_decoder_loglike_bwd_logw(const float* x, const float* y, const float* log_w, float w_scale, const float* W0,
                                    const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                    const float* Ws, const float* bs1, const float* bs2, int64_t N, int K, int S, int L,
                                    int Dy, int U, float* dx, float* dparams, float* ll, void* ws, size_t ws_bytes,
                                    void* stream);

/* compute_elbo for the fused decoder in THREE launches: vmp_decoder_loglike_bwd_logw with w_scale = -sigma / 2S, then ONE
 * launch in which some blocks reduce the decoder's parameter partials and the others run the (N,K) pass of
 * vmp_svae_elbo_tail (below) - both wait for the decoder kernel only - then the one-wave sum of the tail's partials.  Arguments as those two calls; tail_ws as vmp_svae_elbo_tail's ws.  N >= 1.   */
int    vmp_decoder_elbo(const float* x, const float* y, const float* log_z, const float* T_prime, float sigma,
                        const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                        const float* b2, const float* Ws, const float* bs1, const float* bs2, int64_t N, int K, int S,
                        int L, int Dy, int U, float* dx, float* dparams, float* ll, float* scalars, float* g_log_z,
                        float* g_T_prime, float* r, void* ws, size_t ws_bytes, void* tail_ws, size_t tail_ws_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scalar tail of the SVAE ELBO (models/svae.py:216-254 compute_elbo; vae.py:232-250) - two launches
 * ------------------------------------------------------------------------------------------------
 * From log_z (N,K), T_prime (N,K) (the theta side of the regulariser, as the fused E-step returns it) and the
 * per-sample reconstruction sums ll (N,K,S) of the decoder kernel:
 *   r = exp(log_z);  rec = -1/(2S) sum_nk r_nk sum_s ll_nks - N Dy/2 log(2 pi);  reg = sum_nk r_nk (T'_nk + log_z_nk)
 *   scalars = [elbo = rec - reg, rec, reg]   (fp64 sums, fixed order: deterministic)
 *   g_log_z = sigma * d elbo / d log_z,  g_T_prime = sigma * d elbo / d T'   (sigma = -1 for loss = -elbo)
 * Two launches: the (N,K) pass with per-block partial sums, then a one-wave sum of the partials in a fixed order.
 * ws: vmp_svae_elbo_tail_workspace_bytes() bytes of scratch (no initialisation needed); one per concurrently running stream. */
size_t vmp_svae_elbo_tail_workspace_bytes(void);
int    vmp_svae_elbo_tail(const float* log_z, const float* T_prime, const float* ll, int64_t N, int K, int S, int Dy,
                          float sigma, float* scalars, float* g_log_z, float* g_T_prime, float* r, void* ws,
                          size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The minibatch training step in 6 launches (round 6; experiments.py:196-267 at its own operating point, minibatches
 * of 64-100 rows, where a step is bound by the NUMBER of launches - 13 + the input copy + an eager scalar launch before)
 * ------------------------------------------------------------------------------------------------
 *   vmp_mlp_gauss_head_fwd_prep  encoder (vae.make_encoder, vae.py:131-135) + recognition unpacking + theta packing
 *                                (svae.py:342-358, 205-214) + the replayed step's scalars from a table
 *   vmp_svae_estep_fwd_rng_epi   E-step, sub-sample, r                    (svae.py:14-151)
 *   vmp_decoder_elbo_lazy        decoder value + gradients; parameter partials stay in ws
 *   vmp_svae_estep_bwd_tail      ELBO tail + E-step backward              (svae.py:216-254 and the autodiff of :14-119)
 *   vmp_mlp_gauss_head_bwd_lazy  encoder backward; parameter partials stay in ws
 *   vmp_svae_step_final          partial rows -> gradients of phi_gmm (autodiff of svae.py:342-358), both MLP partial
 *                                reductions, Adam on all 21 tensors, M-step moments + CVI update, ELBO scalars
 * Every value equals what the stand-alone launches produce (same device functions, same summation orders); the ELBO
 * scalars are summed per tile instead of per tail block (fp64: equal to fp32 rounding).                              */

/* The step's first launch: vmp_mlp_gauss_head_fwd (the encoder: x (R,L) -> out1, out2 (R,Dy)) and vmp_svae_prep_fwd2 with latent
 * size Dy (recognition unpacking + theta packing, K components) as ONE grid - they depend on the parameters and the minibatch only.
 * scalar_table != NULL (a step replayed from a HIP graph): (table_rows, 2) 64-bit words [Philox key | CVI step size (f32), Adam step
 * size (f32)] filled by the host for the coming steps; the launch copies row *counter (u64, device) to dst16 - the 16 bytes the
 * later launches read, as vmp_svae_step_scalars writes them - and increments the counter: no eager launch per replay.         */
int    vmp_mlp_gauss_head_fwd_prep(const float* x, const float* W0, const float* b0, const float* W1, const float* b1,
                                   const float* W2, const float* b2, const float* Ws, const float* bs1, const float* bs2,
                                   int64_t R, int L, int Dy, int U, float var_scale, float* out1, float* out2,
                                   const float* mu_k, const float* L_raw, const float* pi_raw, const float* alpha,
                                   const float* A, const float* b, const float* beta, const float* v_hat, int K, float* Lk,
                                   float* P, float* bias, float* m, float* W, float* kappa, double* logpi,
                                   const void* scalar_table, int table_rows, void* counter, void* dst16, void* stream);
/* vmp_svae_step_scalars (below) and the copy of the minibatch (n_floats fp32 words, y_src -> y_dst) in one launch. */
int    vmp_svae_step_inputs(void* dst16, uint64_t philox_key, float cvi_step, float adam_step, const float* y_src,
                            float* y_dst, int64_t n_floats, void* stream);
/* Number of partial rows the fused MLP backward kernel writes for `rows` input rows (N*K*S for the decoder). */
int    vmp_decoder_bwd_blocks(int64_t rows);
/* Host query, no launch and no device: the launch plan of the fused MLP kernels (csrc/vmp_decoder.hip) for `rows` input rows
 * (N*K*S for the decoder).  kind: 0 forward (vmp_decoder_loglike_fwd, vmp_mlp_gauss_head_fwd), 1 evaluation forward
 * (vmp_decoder_eval_fwd), 2 encoder forward + prep (vmp_mlp_gauss_head_fwd_prep*; K components add 2 K blocks, K is ignored by the
 * other kinds), 3 backward of the decoder (vmp_decoder_loglike_bwd*, vmp_decoder_elbo*), 4 backward with the head outputs' gradients
 * as inputs (vmp_mlp_gauss_bwd, vmp_mlp_gauss_head_bwd*).  out = [UT: 16-unit tiles of the instance | FS: U is no multiple of 16 |
 * BT: bf16 terms of the backward data path's operands (2 or 3) | split: the older wave's % of a SIMD pair's tiles | red_one: the
 * block epilogue sums all 8 waves' slabs in one round | blocks (backward: the partial rows, vmp_decoder_bwd_blocks) | threads per
 * block | dynamic LDS bytes]; FS, BT, split and red_one are 0 for the forward kinds.  Returns 0, or with out zeroed: VMP_E_DIM for
 * the sizes the entry points refuse (L, Dy outside 1..8, U outside 1..64, rows < 0 or >= 2^31; kind 2: rows < 1, K outside
 * 1..VMP_MAX_K), VMP_E_BADARG (out NULL, no such kind).  rows = 0 is planned as a launch would be (one block), although the entry
 * points launch nothing then and vmp_decoder_bwd_blocks(0) is 0.                                                              */
int    vmp_decoder_launch_plan(int kind, int64_t rows, int L, int Dy, int U, int K, int64_t* out);
/* vmp_decoder_elbo without its second launch: dx, ll as there; the (vmp_decoder_bwd_blocks(N*K*S), param_words) fp32
 * parameter partials are left in ws for vmp_svae_step_final.  The scalar tail runs inside vmp_svae_estep_bwd_tail.  */
int    vmp_decoder_elbo_lazy(const float* x, const float* y, const float* log_z, float sigma, const float* W0,
                             const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* Ws, const float* bs1, const float* bs2, int64_t N, int K, int S, int L, int Dy,
                             int U, float* dx, float* ll, void* ws, size_t ws_bytes, void* stream);
/* vmp_mlp_gauss_head_bwd without the partial reduction ((vmp_decoder_bwd_blocks(R), param_words) partials stay in ws). */
int    vmp_mlp_gauss_head_bwd_lazy(const float* x, const float* g_out1, const float* g_out2, float var_scale,
                                   const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                   const float* b2, const float* Ws, const float* bs1, const float* bs2, int64_t R, int L,
                                   int Dy, int U, float* dx, void* ws, size_t ws_bytes, void* stream);
/* 1 when vmp_svae_estep_bwd_tail covers the shape (the minibatch form: <= 256 tiles of 64 / K rows, S <= 16). */
int    vmp_svae_bwd_tail_applies(int64_t N, int K, int L, int S);
/* vmp_svae_elbo_tail's (N,K) pass + vmp_svae_estep_bwd_n in ONE launch, Gaussian theta: dLoss/dlog_z and dLoss/dT' are
 * formed per cell inside the kernel (sigma * d elbo, as the tail) and never reach memory.  Gx = sigma * d elbo / dx from
 * the decoder.  Outputs: g_eta1, g_eta2d, partials (one row per tile: vmp_svae_bwd_blocks_for) as vmp_svae_estep_bwd_n;
 * r (N,K) = exp(log_z); tail_part (tiles, 2) fp64 = per-tile [sum r A / 2S, sum r (T' + log z)].                     */
int    vmp_svae_estep_bwd_tail(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                               const float* mk, const float* Wk, const float* x, const float* lz, const float* T_prime,
                               const float* ll, float sigma, const float* Gx, int64_t N, int K, int L, int S,
                               float* g_eta1, float* g_eta2d, float* partials, size_t partial_bytes, float* r,
                               double* tail_part, size_t tail_bytes, void* stream);
/* vmp_svae_prep_fwd that also leaves log softmax(pi_raw) (K) fp64 in logpi (may be NULL): the backward forms below read it
 * instead of the other components' pi_raw. */
int    vmp_svae_prep_fwd2(const float* mu_k, const float* L_raw, const float* pi_raw, const float* alpha, const float* A,
                          const float* b, const float* beta, const float* v_hat, int K, int L, float* Lk, float* P,
                          float* bias, float* m, float* W, float* kappa, double* logpi, void* stream);
/* vmp_svae_bwd_reduce (phi side) + vmp_svae_phi_prep_bwd in one launch (stand-alone form of what vmp_svae_step_final does for
 * phi_gmm): block k sums component k's rows of `partials` (nblk, K, vmp_svae_bwd_partial_words) in the order of
 * vmp_svae_bwd_reduce and differentiates the recognition unpacking on them. */
int    vmp_svae_bwd_reduce_prep(const float* partials, int nblk, const float* mu_k, const float* L_raw, const float* pi_raw,
                                const double* logpi, int K, int L, float* g_mu, float* g_Lraw, float* g_piraw, void* stream);
/* The closing launch.  dec_* / enc_*: parameter partials of the two MLPs (rows: *_blocks; sizes: in, units, out = (L,U,Dy)
 * for the decoder, (Dy,U,L) for the encoder), their 9 parameter / Adam-m / Adam-v tensors and 9 gradient outputs, in the
 * order [W0,b0,W1,b1,W2,b2,Ws,bs1,bs2]; partials (nblk rows) of vmp_svae_estep_bwd_tail and logpi of vmp_svae_prep_fwd2;
 * phi_*: the three phi_gmm tensors (mu_k (K,L), L_k (K,L,L), log_pi_k (K)), gradient outputs phi_g; x_samples (N,L), r (N,K): the M-step's inputs (N <= 512); prior, theta, theta_star: 5 natural
 * NIW / Dirichlet tensors each [alpha, A, b, beta, v_hat] (theta updated in place, theta_star may be NULL);
 * rho / rho_dev, lr_t / lr_t_dev as vmp_svae_cvi_update / vmp_adam_step; stats_out (K, 2+L+L*L) fp64;
 * tail_part (tail_n, 2) from vmp_svae_estep_bwd_tail -> scalars [elbo, rec, reg].                                   */
int    vmp_svae_step_final(const float* dec_part, int dec_blocks, int dec_in, int dec_units, int dec_out,
                           float* const* dec_p, float* const* dec_m, float* const* dec_v, float* const* dec_g,
                           const float* enc_part, int enc_blocks, int enc_in, int enc_units, int enc_out,
                           float* const* enc_p, float* const* enc_m, float* const* enc_v, float* const* enc_g,
                           const float* partials, int nblk, const double* logpi,
                           float* const* phi_p, float* const* phi_g, float* const* phi_m, float* const* phi_v,
                           const float* x_samples, const float* r, int64_t N, const float* const* prior,
                           float* const* theta, float* const* theta_star, const float* rho_dev, float rho, int K, int L,
                           double* stats_out, const double* tail_part, int tail_n, int Dy, float* scalars, double beta1,
                           double beta2, double eps, double lr_t, const float* lr_t_dev, void* stream);

/* The closing launch of a DATA-PARALLEL minibatch step (one process per GPU; experiments.py:247-260, tf_utils.py:52-87): the block
 * roles of vmp_svae_step_final, but nothing is updated - this rank's M-step moments, its 21 gradients and its three scalars go as
 * doubles into xbuf = [moments (K, 2+L+L*L) | phi_gmm mu_k, L_k, log_pi_k | encoder net (9) | decoder net (9) | elbo, rec, reg],
 * the packed buffer the step's ONE all-reduce sums; vmp_svae_cvi_update and vmp_adam_step_packed follow it.  The fp32
 * gradients are also left in dec_g / enc_g / phi_g.  xbuf_doubles >= the layout's length.                              */
int    vmp_svae_step_pack(double* xbuf, size_t xbuf_doubles, const float* dec_part, int dec_blocks, int dec_in, int dec_units,
                          int dec_out, float* const* dec_p, float* const* dec_g, const float* enc_part, int enc_blocks,
                          int enc_in, int enc_units, int enc_out, float* const* enc_p, float* const* enc_g,
                          const float* partials, int nblk, const double* logpi, float* const* phi_p, float* const* phi_g,
                          const float* x_samples, const float* r, int64_t N, int K, int L, const double* tail_part, int tail_n,
                          int Dy, float* scalars, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same six-launch minibatch step for the Student-t mixture SVAE (SVAETrainer(smm=True); experiments.py:154-176, 196-267;
 * models/svae.py:179-196, 265-322, 361-373).  Launches 2 (vmp_svae_estep_fwd_rng_epi, nu = DoF), 3 and 5 are the GMM step's;
 * launches 1, 4 and 6 are these.  They replace, for that model, the autograd step's theta packing in torch (tril / softplus,
 * solve_triangular, lgamma, digamma) and its autograd backward, the generic one-tile svae_estep_bwd_kernel + vmp_svae_bwd_reduce,
 * phi_prep_bwd, the torch N_k M-step + CVI update of alpha and the Adam launch.
 * ------------------------------------------------------------------------------------------------ */
/* Launch 1: vmp_mlp_gauss_head_fwd_prep with the Student-t theta packed from (alpha (natural Dirichlet), theta_L_raw, dof) as
 * svae._theta_pack does it: L_k = tril(raw) with softplus diagonal, W = L_k^-1 (K,L,L; lower, 0 above), kappa (K) =
 * lgamma((nu+L)/2) - lgamma(nu/2) - L/2 log(pi nu) - sum log diag L_k + E[log pi_k].  The location m of the E-step is theta/mu_k
 * itself (no output).  L = latent size Dy here, as in vmp_mlp_gauss_head_fwd_prep; scalar table as there. */
int    vmp_mlp_gauss_head_fwd_prep_smm(const float* x, const float* W0, const float* b0, const float* W1, const float* b1,
                                       const float* W2, const float* b2, const float* Ws, const float* bs1, const float* bs2,
                                       int64_t R, int L, int Dy, int U, float var_scale, float* out1, float* out2,
                                       const float* mu_k, const float* L_raw, const float* pi_raw, const float* alpha,
                                       const float* theta_L_raw, const float* dof, int K, float* Lk, float* P, float* bias,
                                       float* W, float* kappa, double* logpi, const void* scalar_table, int table_rows,
                                       void* counter, void* dst16, void* stream);
/* 1 when vmp_svae_estep_bwd_tail_t covers the shape: the envelope of vmp_svae_bwd_tail_applies (<= 256 tiles of 64 / K rows,
 * S <= 16), 0 otherwise (the SMM step then stays the autograd step). */
int    vmp_svae_bwd_tail_applies_t(int64_t N, int K, int L, int S);
/* Launch 4: vmp_svae_estep_bwd_tail with Student-t theta (nu (K) = DoF, mk = theta/mu_k, Wk from launch 1).  The partial rows
 * (vmp_svae_bwd_blocks_for(N, K, L, S, 0) = one per tile) also carry the theta half (words TH..2TH-1: d/dm, d/dW lower,
 * d/dkappa), the layout vmp_svae_bwd_reduce reads when nu != NULL.  vmp_svae_estep_bwd_n / vmp_svae_bwd_blocks_for(...,
 * student = 1) are unchanged (the autograd SMM step keeps the generic kernel). */
int    vmp_svae_estep_bwd_tail_t(const float* eta1, const float* eta2d, const float* hk, const float* Pk, const float* bias,
                                 const float* mk, const float* Wk, const float* nu, const float* x, const float* lz,
                                 const float* T_prime, const float* ll, float sigma, const float* Gx, int64_t N, int K, int L,
                                 int S, float* g_eta1, float* g_eta2d, float* partials, size_t partial_bytes, float* r,
                                 double* tail_part, size_t tail_bytes, void* stream);
/* Launch 6: vmp_svae_step_final's roles for the SMM model.  theta_p / _g / _m / _v: theta/mu_k (K,L), theta/L_k raw (K,L,L) with
 * their gradient outputs and Adam slots - their gradients are the theta half of the partial rows (reduced in
 * vmp_svae_bwd_reduce's order) through the theta packing: g_mu = g_m; g_Lk = -W^T g_W W^T (lower) - g_kappa / diag L_k;
 * softplus / tril to g_L_raw.  Adam on 23 tensors (trainables() order: phi (3), theta (2), encoder (9), decoder (9)).  M-step:
 * stats_out (K, 1) fp64 = N_k = sum_n r_nk, alpha* = prior_alpha + N_k -> alpha_star (may be NULL), alpha <- (1-rho) alpha +
 * rho alpha* (svae.py:179-196, experiments.py:252-256).  r (N,K) from launch 4, N <= 512. */
int    vmp_svae_step_final_smm(const float* dec_part, int dec_blocks, int dec_in, int dec_units, int dec_out,
                               float* const* dec_p, float* const* dec_m, float* const* dec_v, float* const* dec_g,
                               const float* enc_part, int enc_blocks, int enc_in, int enc_units, int enc_out,
                               float* const* enc_p, float* const* enc_m, float* const* enc_v, float* const* enc_g,
                               const float* partials, int nblk, const double* logpi,
                               float* const* phi_p, float* const* phi_g, float* const* phi_m, float* const* phi_v,
                               float* const* theta_p, float* const* theta_g, float* const* theta_m, float* const* theta_v,
                               const float* r, int64_t N, const float* prior_alpha, float* alpha, float* alpha_star,
                               const float* rho_dev, float rho, int K, int L, double* stats_out, const double* tail_part,
                               int tail_n, int Dy, float* scalars, double beta1, double beta2, double eps, double lr_t,
                               const float* lr_t_dev, void* stream);
/* Data-parallel form of vmp_svae_step_final_smm (as vmp_svae_step_pack for the GMM step): nothing is updated; xbuf = [N_k (K, 1) |
 * phi_gmm (3) | theta/mu_k, theta/L_k | encoder (9) | decoder (9) | elbo, rec, reg], the SMM step's exchange buffer. */
int    vmp_svae_step_pack_smm(double* xbuf, size_t xbuf_doubles, const float* dec_part, int dec_blocks, int dec_in,
                              int dec_units, int dec_out, float* const* dec_p, float* const* dec_g, const float* enc_part,
                              int enc_blocks, int enc_in, int enc_units, int enc_out, float* const* enc_p,
                              float* const* enc_g, const float* partials, int nblk, const double* logpi, float* const* phi_p,
                              float* const* phi_g, float* const* theta_p, float* const* theta_g, const float* r, int64_t N,
                              int K, int L, const double* tail_part, int tail_n, int Dy, float* scalars, void* stream);

/* Writes the 16 bytes [Philox key (u64) | CVI step size (f32) | Adam step size (f32)] that a graph-captured training step
 * reads at run time (vmp_svae_estep_fwd_rng_dev / vmp_svae_subsample_rng seed_dev, vmp_svae_cvi_update rho_dev,
 * vmp_adam_step lr_t_dev = dst16 + 0 / 8 / 12): one launch, values passed by value.                                  */
int    vmp_svae_step_scalars(void* dst16, uint64_t philox_key, float cvi_step, float adam_step, void* stream);

/* tf.train.AdamOptimizer's update (TF 1.3; experiments.py:264-265) of n_tensors fp32 tensors in one launch per 32
 * tensors:  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr_t m / (sqrt(v) + eps), where the caller supplies the
 * bias-corrected step size lr_t = lr sqrt(1-b2^t)/(1-b1^t) - by value, or through lr_t_dev (a device float that
 * overrides it: graph-captured steps refresh that word instead of re-capturing).  params/grads/m/v: HOST arrays of
 * n_tensors device pointers; sizes: element counts.  The scalars are doubles: 1 - b is formed in fp64, then rounded.                                                                */
int    vmp_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* m, float* const* v,
                     const int64_t* sizes, double beta1, double beta2, double eps, double lr_t, const float* lr_t_dev,
                     void* stream);

/* Data-parallel training step (experiments.py:247-265; helpers/tf_utils.py:52-87 average_gradients): the tower gather
 * becomes ONE packed fp64 buffer per rank, summed by one all-reduce (vmp_pack_allreduce / torch.distributed).
 * vmp_pack_f64: dst = [src_0 | src_1 | ...] converted to fp64, one launch per 32 tensors (src: HOST array of device
 *   pointers; src_is_f64[t] != 0: tensor t already holds doubles).
 * vmp_adam_step_packed: vmp_adam_step whose gradient of tensor t is gscale * gbuf[goffsets[t] ...] (gscale = 1 / ranks:
 *   the mean over the towers, formed in fp64 and rounded once); grads_out (nullable, or NULL entries): the averaged fp32
 *   gradient is also stored there (what the trainer reports).                                                              */
int    vmp_pack_f64(int n_tensors, const void* const* src, const int* src_is_f64, const int64_t* sizes, double* dst, void* stream);
int    vmp_adam_step_packed(int n_tensors, float* const* params, const double* gbuf, const int64_t* goffsets, double gscale,
                            float* const* grads_out, float* const* m, float* const* v, const int64_t* sizes, double beta1,
                            double beta2, double eps, double lr_t, const float* lr_t_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone per-cell log-densities (forward only; the training step uses the fused kernels above)
 * ------------------------------------------------------------------------------------------------
 * vmp_gauss_logprob_nat_per_samp : gaussian.log_probability_nat_per_samp (distributions/gaussian.py:74-105)
 *     x (N,K,S,D), eta1 (N,K,D), eta2 (N,K,D,D) -> out (N,K,S)
 * vmp_gauss_logprob_nat          : gaussian.log_probability_nat (gaussian.py:30-71), normalised over k
 *     x (N,D), eta1 (N,K,D), eta2 (N,K,D,D), log_weights (K) or NULL -> out (N,K)
 * vmp_student_t_logprob          : student_t.log_probability_per_samp (distributions/student_t.py:7-39,59-61)
 *     y (N,K,S,D), mu (K,D), W (K,D,D) lower with W^T W = sigma^-1, cst (K) = lgamma((v+D)/2) - lgamma(v/2)
 *     - D/2 log(pi v) - 1/2 logdet sigma, nu (K) -> out (N,K,S)   (the K distinct scale matrices are factorised
 *     once on the host side instead of N*K*S times, student_t.py:26-36)                                        */
int    vmp_gauss_logprob_nat_per_samp(const float* x, const float* eta1, const float* eta2, int64_t N, int K, int S,
                                      int D, float* out, void* stream);
int    vmp_gauss_logprob_nat(const float* x, const float* eta1, const float* eta2, const float* log_weights,
                             int64_t N, int K, int D, float* out, void* stream);
/* Stand-alone expected Mahalanobis distance (gmm.compute_expct_mahalanobis_dist models/gmm.py:84-94,
 * compute_dev_missing_data :97-114, smm.expct_mahalanobis_dist models/smm.py:88-96):
 * out (N,K) = v_k (x_n - m_k)^T P_k (x_n - m_k) + D / beta_k, entries with miss_mask (N,D) != 0 dropped.          */
int    vmp_mix_mahalanobis(const float* x, const float* m, const float* P, const float* v, const float* beta,
                           const uint8_t* miss_mask, int64_t N, int D, int K, float* out, void* stream);
int    vmp_student_t_logprob(const float* y, const float* mu, const float* W, const float* cst, const float* nu,
                             int64_t N, int K, int S, int D, float* out, void* stream);
/* Adjoints of the two per-sample densities above - what TF's autodiff does through gaussian.py:74-105 and student_t.py:7-39
 * when the reference differentiates compute_elbo (svae.py:236-243, 291-300; experiments.py:232):
 *   vmp_gauss_logprob_nat_per_samp_bwd: g (N,K,S) upstream -> gx (N,K,S,D), geta1 (N,K,D), geta2 (N,K,D,D) (symmetric:
 *       sum_s g_s (x_s x_s^T - E[x x^T]), the exponential-family identity; eta2 is read symmetrised as in the forward);
 *   vmp_student_t_logprob_bwd: gy (N,K,S,D) and per-block partial sums over (n,s) of the gradients w.r.t. the K-sized
 *       (mu_k (D) | W_k lower packed (D(D+1)/2) | cst_k): partials (vmp_student_t_bwd_blocks(N,S), K, D + D(D+1)/2 + 1),
 *       summed over the first axis by the caller; nu is treated as a constant (the reference's DoF is not trainable,
 *       experiments.py:163-165).                                                                                       */
int    vmp_gauss_logprob_nat_per_samp_bwd(const float* x, const float* eta1, const float* eta2, const float* g, int64_t N,
                                          int K, int S, int D, float* gx, float* geta1, float* geta2, void* stream);
int    vmp_student_t_bwd_blocks(int64_t N, int S);
int    vmp_student_t_logprob_bwd(const float* y, const float* mu, const float* W, const float* nu, const float* g, int64_t N,
                                 int K, int S, int D, float* gy, float* partials, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics: the (N,K,S,Dy)-sized part of losses.weighted_mse (losses.py:9-38) and
 * losses.diagonal_gaussian_logprob (losses.py:83-145)
 * ------------------------------------------------------------------------------------------------
 *   mse (N,K) = mean_s sum_d (y - mean)^2                                             (may be NULL)
 *   lse (N,K) = log 1/S sum_s exp( logw_nk(s) - 1/2 sum_d mask_nd [(y-mean)^2/var + log var + log 2pi] )   (may be NULL)
 * logw: (N,K), or (N,K,S) when logw_per_sample, or NULL; mask (N,Dy) uint8 or NULL (losses.py:118-124).
 * mask_mse != 0: the squared error also counts masked entries only,
 *   mse = mean_s sum_d mask_nd (y - mean)^2   = the per-cell part of losses.imputation_mse (losses.py:148-170).   */
int    vmp_eval_cell_metrics(const float* y, const float* mean, const float* var, const float* logw,
                             int logw_per_sample, const uint8_t* mask, int mask_mse, int64_t N, int K, int S, int Dy,
                             float* mse, float* lse, void* stream);

/* The same two per-cell metrics straight from the samples x (N,K,S,L): the fused decoder forward (vmp_decoder_loglike_fwd: same
 * parameters, same compiled range L, Dy <= 8, U <= 64, bit-identical mean / var per row) with the metrics as its epilogue, so that
 * no (N,K,S,Dy) tensor exists.  The kernel leaves two fp32 words per sample row in `ws` (N*K*S*8 bytes, 8-byte aligned, required);
 * a second small launch takes the mean / the online log-sum-exp over s.  Definitions and quirks as above (`log var`, not
 * log(var + 1e-8); mask_mse); logw is (N,K) or NULL; mask (N,Dy) uint8 or NULL; mse, lse (N,K): either may be NULL, not both.
 * The sum over d runs in another order than vmp_eval_cell_metrics' (last bits).                                          */
int    vmp_decoder_eval_fwd(const float* x, const float* y, const float* W0, const float* b0, const float* W1, const float* b1,
                            const float* W2, const float* b2, const float* Ws, const float* bs1, const float* bs2,
                            const uint8_t* mask, int mask_mse, const float* logw, int64_t N, int K, int S, int L, int Dy,
                            int U, float* mse, float* lse, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU exchange (replaces the in-graph tower gather + mean of experiments.py:247-260 and
 * helpers/tf_utils.py:52-87): ONE in-place all-reduce(sum) over RCCL / xGMI of the packed fp64 buffer
 *   T1: raw moments (K, 2+D+D*D);   T3: [ raw moments | flat gradients | elbo, neg_rec_err, regulariser ]
 * after which every rank applies the identical K-sized update.  `comm` is an RCCL communicator (ncclComm_t); a host
 * that has none (the torch host uses torch.distributed's) builds one with the three helpers: rank 0 calls
 * vmp_comm_unique_id and ships the 128-byte id to the other ranks out of band, every rank calls vmp_comm_init_rank
 * with its device current.  RCCL is resolved at run time (the copy the process has already loaded, else librccl.so.1):
 * the library has no link-time dependency on it and single-GPU hosts never load it.                              */
#define VMP_COMM_ID_BYTES 128
int    vmp_comm_unique_id(void* id_out /* VMP_COMM_ID_BYTES */);
int    vmp_comm_init_rank(void** comm_out, int nranks, const void* id, int rank);
int    vmp_comm_destroy(void* comm);
int    vmp_pack_allreduce(void* comm, double* buf, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T1 data-parallel iteration in ONE launch per rank (round 3).  The RCCL form above costs three dependent launches
 * plus the collective (local reduction -> all-reduce -> posterior); here the finalize kernel of every rank
 *   (1) reduces its own per-block partials (as vmp_mix_finalize_ws),
 *   (2) PUSHES its un-shifted fp64 moments of component k into slot [parity][rank][k] of EVERY rank's exchange buffer
 *       (plain stores, system-scope release, then a sequence word = iteration + 1),
 *   (3) waits until the sequence words of all ranks for component k have arrived in its OWN buffer (bounded spin on
 *       local memory), and sums the slots in rank order 0..G-1 - the same order on every rank, so all ranks obtain
 *       bit-identical moments -, then
 *   (4) continues with the posterior update and the E-step pack (as vmp_mix_finalize).
 * Replaces the tower gather + M-step on the parameter device of experiments.py:247-260 for the pure mixture loop
 * (gmm.py:258-263 over sharded rows).  Exchange buffers: one per rank, vmp_exch_bytes(G, K, D) bytes of uncached
 * device memory (vmp_exch_alloc), exported with vmp_exch_export (VMP_EXCH_HANDLE_BYTES, shipped to the peers out of band)
 * and mapped by every peer with vmp_exch_open; peers[g] = rank g's buffer as mapped in THIS process (peers[rank] = the
 * local allocation).  `iteration` must increase by one per call on every rank (slots are double-buffered by parity).
 * `status` (device int, may be NULL) is set to 1 if a wait timed out (~4 s): the results of that call are invalid.   */
#define VMP_EXCH_MAX_RANKS 16
#define VMP_EXCH_HANDLE_BYTES 64
size_t vmp_exch_bytes(int nranks, int K, int D);
int    vmp_exch_alloc(void** buf_out, size_t bytes);
int    vmp_exch_free(void* buf);
int    vmp_exch_export(void* buf, void* handle_out /* VMP_EXCH_HANDLE_BYTES */);
int    vmp_exch_open(const void* handle, void** peer_out);
int    vmp_exch_close(void* peer);
int    vmp_mix_finalize_exchange(const void* workspace, const float* pivot, int64_t N, int D, int K, int flavour,
                                 const float* alpha0, const float* beta0, const float* m0, const float* C0,
                                 const float* v0, const float* kappa, float* alpha, float* beta, float* m, float* C,
                                 float* v, float* xbar, float* S, float* pi, float* pack, double* stats_out,
                                 void* const* peers, int nranks, int rank, unsigned long long iteration, int* status,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VMP_HIP_H */
