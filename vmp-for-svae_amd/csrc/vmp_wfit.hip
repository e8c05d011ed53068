// Fitting the variational Gaussian mixture on WEIGHTED rows (include/vmp_hip.h "Mixture fitting on weighted rows"): a weight w_n >= 0
// makes row n count as w_n identical rows - counts of binned or de-duplicated data, coresets, importance weights, and 0/1 folds over
// rows that stay where they are.  One streaming pass over (x, w[, mask]) under the fit pack of vmp_missfit.hip
// [ m_k (D) | Lbar_k = v_k C_k^-1 lower, row-major packed | c_k ]:
//   log rho_nk, xhat^(k), Cov^(k)   the cell of vmp_missfit.hip (its header); a complete row: log rho = c - 1/2 d^T Lbar d, d = x - m_k,
//                                   xhat = x, no Cov,
//   r_nk = softmax_k log rho_nk     UNCHANGED: a weight does not enter a row's own responsibilities,
//   Nk  = sum_n w_n r_nk,   sx = sum_n w_n r_nk xhat^(k),   sxx = sum_n w_n r_nk (xhat^(k) xhat^(k)^T + Cov^(k)),
//   data = sum_n w_n (logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi)          the data term of the lower bound (vmp_bound.hip).
// The weight enters in two places only: the r handed to the moment accumulation is w r, and the fp64 row sum adds w times the row's
// term.  A row with w = 0 is REMOVED, not multiplied: its lanes skip the moment accumulation (a lane predicate - 0 * NaN would be NaN)
// and add a selected 0.0 to the row sum, so whatever its x holds - NaN and Inf in observed slots included - reaches neither.  Its r,
// log r and x_fill are still written, as whatever the E-step gives: the responsibilities of a held-out row.
//
// Geometry: that of fit_kernel (vmp_missfit.hip) - 4 waves per block, wave g owns rows [g rpw, (g+1) rpw), lane l = (i16 = l & 15,
// kk = l >> 4) owns component i16 + 16 t of every tile and row n4 + kk; the moments are formed in fp32 on xhat - m_k, the four lanes of a
// component are added every FIT_CHUNK rows (rows4_sum) and flushed to the wave's own fp64 words by a plain read-modify-write, and a
// second launch adds the waves in a fixed order and un-shifts in fp64.  K > 16: a chunk is walked twice, r written in the first walk
// and read back from the lane's own store in the second.  The row sum is the one of vmp_mix_stream.h.  Neither depends on which
// outputs are requested: no atomics, the same bits from run to run and for every set of optional outputs.
// MASKED = false: nothing is factored and the moments come from d alone (fit_cell_full / fit_moments_full) - the form that matters
// for speed.  MASKED = true: fit_cell / fit_moments, the cell and the moments of fit_kernel.  All four, the flush, the row load, the
// body of the reduction, the block geometry (FIT_*) and the host's iteration are in vmp_fit_cell.h, shared with vmp_missfit.hip.
#include "vmp_fit_cell.h"

using namespace vmp;

namespace {

struct WFitArgs {
    const float* x;
    const float* w;       // (N) weights, >= 0
    const uint8_t* mask;  // (N,D) or NULL
    const float* pack;
    float* r;             // (N,K), or NULL: no moments either (the bound-only form)
    float* logr;          // (N,K) or NULL
    float* x_fill;        // (N,D) or NULL (needs a mask)
    double* slab;         // (waves, K, MW) fp64: the moments of a wave's rows
    double* partials;     // (blocks) fp64: the row sums of the blocks
    long long N;
    long long rpw;        // rows per wave (multiple of 4): wave g owns rows [g rpw, min(N, (g+1) rpw))
    int K;
    int vec_in, vec_out;  // x / x_fill 16-byte aligned
};

// what a cell leaves for the moments: d = xhat - m_k and, under a mask, the factor
template <int D, bool MASKED>
struct WCell {
    float dh[D];
    float A[MASKED ? FitGeo<D>::TRI : 1], rd[MASKED ? D : 1];
    __device__ __forceinline__ float eval(const FitParams<D>& p, const float (&x)[D], const bool (&miss)[D]) {
        if constexpr (MASKED) return fit_cell<D>(p, x, miss, dh, A, rd);
        else                  return fit_cell_full<D>(p, x, dh);
    }
    // wr = w r of a kept cell, 0 of a cell that does not count (w = 0, a row or a component past the end): such a lane adds nothing -
    // a predicate, not a product, because its dh may be NaN
    __device__ __forceinline__ void moments(const bool (&miss)[D], float wr, float (&acc)[FitGeo<D>::MW]) {
        if (wr != 0.f) {
            if constexpr (MASKED) fit_moments<D>(dh, miss, A, rd, wr, acc);
            else                  fit_moments_full<D>(dh, wr, acc);
        }
    }
};

template <int D, int KTMAX, bool MASKED>
__global__ __launch_bounds__(FIT_NW * WAVE) void wfit_pass_kernel(WFitArgs a) {
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
    const bool mom = a.r != nullptr;                                         // the bound-only form: no r, no moments
    double* slab = a.slab + g * a.K * G::MW;
    const double HALF_LOG_2PI = 0.91893853320467274178;
    double dsum = 0.0;                                                       // lanes i16 = 0: the weighted row terms, in row order
    float acc[G::MW];
#pragma unroll
    for (int i = 0; i < G::MW; ++i) acc[i] = 0.f;

    if (r0 >= r1 && mom)                                                     // a wave without rows: its moments are zero
        for (int i = lane; i < a.K * G::MW; i += WAVE) slab[i] = 0.0;

    for (long long c0 = r0; c0 < r1; c0 += FIT_CHUNK) {
        const long long c1 = c0 + FIT_CHUNK < r1 ? c0 + FIT_CHUNK : r1;
        for (long long n4 = c0; n4 < c1; n4 += 4) {
            const long long n = n4 + kk;
            const bool valid = n < c1;
            const long long nr = valid ? n : c1 - 1;                         // rows past the range: a row of the range, discarded
            float x[D];
            bool miss[D];
            const int n_obs = fit_load_row<D, MASKED>(a, nr, x, miss);
            const float w = a.w[nr];

            // lane-local online log-sum-exp over the lane's tiles: ml = running maximum, s = sum e, ax = sum e xhat
            float ml = -INFINITY, s = 0.f, ax[MASKED ? D : 1], lt[KTMAX];
            WCell<D, MASKED> cell;
            if constexpr (MASKED) {
#pragma unroll
                for (int d = 0; d < D; ++d) ax[d] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) lt[j] = -INFINITY;
#pragma unroll 1
            for (int t = 0; t < KT; ++t) {
                const int k = t * 16 + i16;
                if constexpr (KTMAX > 1) p.load(lds + (k < a.K ? k : 0) * G::STRIDE);
                float l = cell.eval(p, x, miss);
                l = k < a.K ? l : -INFINITY;
#pragma unroll
                for (int j = 0; j < KTMAX; ++j) lt[j] = t == j ? l : lt[j];
                const float mn = fmaxf(ml, l);
                const float sh = mn == -INFINITY ? 0.f : mn;                 // every term so far -inf: -inf - (-inf) would be NaN
                const float c = __expf(ml - sh), e = __expf(l - sh);
                s = fmaf(s, c, e);
                if constexpr (MASKED) {
#pragma unroll
                    for (int d = 0; d < D; ++d) ax[d] = fmaf(ax[d], c, e == 0.f ? 0.f : e * (p.mu[d] + cell.dh[d]));
                }
                ml = mn;
            }
            const float mx = row16_max(ml);
            const float shift = mx == -INFINITY ? 0.f : mx;
            const float f = __expf(ml - shift);
            const float S = row16_sum(s * f);
            const float inv = S == 0.f ? 0.f : 1.0f / S;                     // a row without mass: r = 0, filled entries 0
            const float lp = shift + logf(S);
            const double term = (double)lp - HALF_LOG_2PI * (double)n_obs;
            if (valid) dsum += w == 0.f ? 0.0 : (double)w * term;            // lanes i16 = 0 are the ones the row sum reads
            if constexpr (MASKED) {
                if (a.x_fill) {
                    float o[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const float xs = row16_sum(ax[d] * f) * inv;
                        o[d] = miss[d] ? xs : x[d];
                    }
                    if (valid && i16 == 0) store_row<D>(a.x_fill + n * D, o, a.vec_out != 0);
                }
            }
            float rk = 0.f;
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) {
                const int k = j * 16 + i16;
                rk = __expf(lt[j] - shift) * inv;
                if (mom && valid && k < a.K) {
                    a.r[n * a.K + k] = rk;
                    if (a.logr) a.logr[n * a.K + k] = lt[j] - lp;
                }
            }
            if constexpr (KTMAX == 1) {
                if (mom) cell.moments(miss, (valid && i16 < a.K && w != 0.f) ? w * rk : 0.f, acc);
            }
        }
        if (!mom) continue;
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
                    float x[D];
                    bool miss[D];
                    fit_load_row<D, MASKED>(a, nr, x, miss);
                    const float w = a.w[nr];
                    WCell<D, MASKED> cell;
                    cell.eval(p, x, miss);
                    const float rk = (valid && k < a.K) ? a.r[n * a.K + k] : 0.f;      // the lane's own store of the first walk
                    cell.moments(miss, w != 0.f ? w * rk : 0.f, acc);
                }
                fit_flush<D>(acc, slab + (k < a.K ? k : 0) * G::MW, c0 == r0, kk == 0 && k < a.K);
            }
        }
    }
    wave_block_sum<FIT_NW>(dsum, lane, wave, a.partials);
}

__global__ __launch_bounds__(WAVE) void wfit_sum_kernel(const double* partials, int nblk, double* out) { block_sum(partials, nblk, out); }

struct WFitReduceArgs {
    const double* slab;
    const float* pack;
    double* stats;        // (K, SW)
    int nwaves, K;
};

// the waves of the slab added in a fixed order and un-shifted by m_k: fit_unshift_reduce (vmp_fit_cell.h); word 1 (Wk) = word 0 (Nk)
template <int D>
__global__ __launch_bounds__(FIT_RED_GROUPS * WAVE) void wfit_unshift_kernel(WFitReduceArgs a) {
    fit_unshift_reduce<D>(a);
}

template <int D, bool MASKED>
int launch_wfit(const WFitArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(FIT_NW * WAVE);
    if (a.K <= 16) hipLaunchKernelGGL((wfit_pass_kernel<D, 1, MASKED>), grid, block, 0, s, a);
    else           hipLaunchKernelGGL((wfit_pass_kernel<D, 4, MASKED>), grid, block, 0, s, a);
    return check_launch("wfit_pass_kernel");
}

// every refusal of the pass, decided on the host
int wfit_pass_check(const char* who, const float* x, const float* w, const uint8_t* mask, int64_t N, int D, int K, const float* pack,
                    const float* r_out, const float* logr_out, const float* x_fill_out, const double* stats_out, const double* bound_out,
                    const void* ws, size_t ws_bytes) {
    int rc = stream_dims(who, D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !w || !pack) { set_error("%s: null pointer (%s)", who, !x ? "x" : !w ? "w" : "pack"); return VMP_E_BADARG; }
    if (!r_out && !logr_out && !x_fill_out && !stats_out && !bound_out) {
        set_error("%s: no output requested (r_out, logr_out, x_fill_out, stats_out and bound_out are all NULL)", who);
        return VMP_E_BADARG;
    }
    if (!r_out && stats_out) { set_error("%s: stats_out needs r_out (the moments are those of the r the pass writes)", who); return VMP_E_BADARG; }
    if (!r_out && logr_out) { set_error("%s: logr_out needs r_out", who); return VMP_E_BADARG; }
    if (x_fill_out && !mask) { set_error("%s: x_fill_out needs a mask (a complete row has nothing to fill)", who); return VMP_E_BADARG; }
    return workspace_check(who, ws, ws_bytes, vmp_mixture_wfit_workspace_bytes(N, D, K));
}

}  // namespace

extern "C" {

size_t vmp_mixture_wfit_workspace_bytes(int64_t N, int D, int K) {
    if (D < 1 || D > VMP_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    return fit_slab_bytes(N, D, K) + (size_t)fit_blocks(N) * sizeof(double);         // the fp64 moments of every wave | one partial per block
}

int vmp_mixture_wfit_pass(const float* x, const float* w, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* r_out,
                          float* logr_out, float* x_fill_out, double* stats_out, double* bound_out, void* ws, size_t ws_bytes,
                          void* stream) {
    int rc = wfit_pass_check("vmp_mixture_wfit_pass", x, w, mask, N, D, K, pack, r_out, logr_out, x_fill_out, stats_out, bound_out, ws,
                             ws_bytes);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = fit_blocks(N);
    const long long waves = (long long)blocks * FIT_NW;
    WFitArgs a{};
    a.x = x; a.w = w; a.mask = mask; a.pack = pack; a.r = r_out; a.logr = logr_out; a.x_fill = x_fill_out;
    a.slab = static_cast<double*>(ws);
    a.partials = reinterpret_cast<double*>(static_cast<char*>(ws) + fit_slab_bytes(N, D, K));
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, waves, 4);
    a.vec_in = aligned16(x); a.vec_out = aligned16(x_fill_out);
    rc = -1;
    if (mask) { VMP_SWITCH_DIM(D, DD, rc = (launch_wfit<DD, true>(a, blocks, s))); }
    else      { VMP_SWITCH_DIM(D, DD, rc = (launch_wfit<DD, false>(a, blocks, s))); }
    if (rc) return rc;
    if (stats_out) {
        WFitReduceArgs ra{a.slab, pack, stats_out, (int)waves, K};
        rc = -1;
        VMP_SWITCH_DIM(D, DD, {
            hipLaunchKernelGGL((wfit_unshift_kernel<DD>), dim3(K), dim3(FIT_RED_GROUPS * WAVE), 0, s, ra);
            rc = check_launch("wfit_unshift_kernel");
        });
        if (rc) return rc;
    }
    if (bound_out) {
        hipLaunchKernelGGL(wfit_sum_kernel, dim3(1), dim3(WAVE), 0, s, a.partials, blocks, bound_out);
        rc = check_launch("wfit_sum_kernel");
    }
    return rc;
}

int vmp_mixture_wfit_iterate(const float* x, const float* w, const uint8_t* mask, int64_t N, int D, int K, const float* alpha0,
                             const float* beta0, const float* m0, const float* C0, const float* v0, float* r, float* logr, float* x_fill,
                             float* alpha, float* beta, float* m, float* C, float* v, float* xbar, float* S, float* pi, float* pack,
                             double* stats, double* bound, void* ws, size_t ws_bytes, int iterations, void* stream) {
    if (!r || !stats) {      // the pass alone has a bound-only form; the iteration has not
        int rc = stream_dims("vmp_mixture_wfit_iterate", D, K);
        if (rc) return rc;
        set_error("vmp_mixture_wfit_iterate: null pointer (%s)", !r ? "r" : "stats");
        return VMP_E_BADARG;
    }
    int rc = wfit_pass_check("vmp_mixture_wfit_iterate", x, w, mask, N, D, K, pack, r, logr, x_fill, stats, bound, ws, ws_bytes);
    if (rc) return rc;
    return fit_iterate("vmp_mixture_wfit_iterate", "prior or posterior", D, K, alpha0, beta0, m0, C0, v0, alpha, beta, m, C, v, xbar, S, pi,
                       pack, stats, iterations, stream, [&] {
                           return vmp_mixture_wfit_pass(x, w, mask, N, D, K, pack, r, logr, x_fill, stats, bound, ws, ws_bytes, stream);
                       });
}

}  // extern "C"
