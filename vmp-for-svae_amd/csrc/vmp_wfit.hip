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
// component are added every WF_CHUNK rows (rows4_sum) and flushed to the wave's own fp64 words by a plain read-modify-write, and a
// second launch adds the waves in a fixed order and un-shifts in fp64.  K > 16: a chunk is walked twice, r written in the first walk
// and read back from the lane's own store in the second.  The row sum is the one of vmp_mix_stream.h.  Neither depends on which
// outputs are requested: no atomics, the same bits from run to run and for every set of optional outputs.
// MASKED = false: nothing is factored and the moments come from d alone - the form that matters for speed.  MASKED = true: the cell
// and the moments of fit_cell / fit_moments, written out here so that vmp_missfit.hip stays as it is.
#include "vmp_mix_stream.h"

using namespace vmp;

namespace {

constexpr int WF_NW = 4;                  // waves per block
constexpr int WF_MAX_BLOCKS = 512;
constexpr int WF_CHUNK = 128;             // rows of a wave between two fp32 -> fp64 flushes, as FIT_CHUNK
constexpr int WF_RED_GROUPS = 16;         // wave groups of the reduction block

inline int wfit_blocks(int64_t N) { return stream_blocks(N, (int64_t)WF_NW * WF_CHUNK, WF_MAX_BLOCKS); }

template <int D>
struct WGeo {
    static constexpr int TRI  = D * (D + 1) / 2;
    static constexpr int C    = D + TRI;
    static constexpr int PACK = C + 1;
    static constexpr int STRIDE = PACK | 1;        // LDS stride: odd, so that the 16 components of a tile fall into 16 banks
    static constexpr int MW   = 1 + D + TRI;       // moment words per component: Nk | s1 (D) | s2 lower packed
    static constexpr int SW   = 2 + D + D * D;     // public stats words
};

inline int wfit_moment_words(int D) { return 1 + D + D * (D + 1) / 2; }
inline size_t wfit_slab_bytes(int64_t N, int D, int K) { return (size_t)wfit_blocks(N) * WF_NW * K * wfit_moment_words(D) * sizeof(double); }

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

template <int D>
struct WParams {
    float mu[D], lam[WGeo<D>::TRI], c;
    __device__ __forceinline__ void load(const float* src) {
        using G = WGeo<D>;
#pragma unroll
        for (int d = 0; d < D; ++d) mu[d] = src[d];
#pragma unroll
        for (int i = 0; i < G::TRI; ++i) lam[i] = src[D + i];
        c = src[G::C];
    }
    __device__ __forceinline__ float L(int i, int j) const { return lam[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i]; }
};

// complete row: d = x - m_k and log rho = c - 1/2 d^T Lbar d over the lower triangle (bound_cell_full of vmp_bound.hip)
template <int D>
__device__ __forceinline__ float wfit_cell_full(const WParams<D>& p, const float (&x)[D], float (&d)[D]) {
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
__device__ __forceinline__ void wfit_moments_full(const float (&d)[D], float r, float (&acc)[WGeo<D>::MW]) {
    acc[0] += r;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float rd = r * d[i];
        acc[1 + i] += rd;
#pragma unroll
        for (int j = 0; j <= i; ++j) acc[1 + D + i * (i + 1) / 2 + j] = fmaf(rd, d[j], acc[1 + D + i * (i + 1) / 2 + j]);
    }
}

// partly observed row: fit_cell of vmp_missfit.hip in the same operations - log rho; dh[] = xhat - m_k; A[] the off-diagonal entries
// of the Cholesky factor of A~ = M Lbar M + (I - M) and rd[] its reciprocal diagonal, for wfit_moments_masked
template <int D>
__device__ __forceinline__ float wfit_cell_masked(const WParams<D>& p, const float (&x)[D], const bool (&miss)[D], float (&dh)[D],
                                                  float (&A)[WGeo<D>::TRI], float (&rd)[D]) {
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

// acc += r [ 1 | dh | dh dh^T + Cov ]: fit_moments of vmp_missfit.hip - W = R^-1 in place of the factor, Cov = W^T W with the
// observed diagonal (exactly 1) dropped
template <int D>
__device__ __forceinline__ void wfit_moments_masked(const float (&dh)[D], const bool (&miss)[D], float (&A)[WGeo<D>::TRI],
                                                    const float (&rd)[D], float r, float (&acc)[WGeo<D>::MW]) {
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

// what a cell leaves for the moments: d = xhat - m_k and, under a mask, the factor
template <int D, bool MASKED>
struct WCell {
    float dh[D];
    float A[MASKED ? WGeo<D>::TRI : 1], rd[MASKED ? D : 1];
    __device__ __forceinline__ float eval(const WParams<D>& p, const float (&x)[D], const bool (&miss)[D]) {
        if constexpr (MASKED) return wfit_cell_masked<D>(p, x, miss, dh, A, rd);
        else                  return wfit_cell_full<D>(p, x, dh);
    }
    // wr = w r of a kept cell, 0 of a cell that does not count (w = 0, a row or a component past the end): such a lane adds nothing -
    // a predicate, not a product, because its dh may be NaN
    __device__ __forceinline__ void moments(const bool (&miss)[D], float wr, float (&acc)[WGeo<D>::MW]) {
        if (wr != 0.f) {
            if constexpr (MASKED) wfit_moments_masked<D>(dh, miss, A, rd, wr, acc);
            else                  wfit_moments_full<D>(dh, wr, acc);
        }
    }
};

// the four lanes that own component k add their sums; lane kk = 0 adds the result to the wave's fp64 words (first: replaces them)
template <int D>
__device__ __forceinline__ void wfit_flush(float (&acc)[WGeo<D>::MW], double* __restrict__ dst, bool first, bool owner) {
#pragma unroll
    for (int i = 0; i < WGeo<D>::MW; ++i) {
        const float s = rows4_sum(acc[i]);
        if (owner) dst[i] = (first ? 0.0 : dst[i]) + (double)s;
        acc[i] = 0.f;
    }
}

template <int D, bool MASKED>
__device__ __forceinline__ int wfit_load_row(const WFitArgs& a, long long nr, float (&x)[D], bool (&miss)[D]) {
    load_row<D>(a.x + nr * D, x, a.vec_in != 0);
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

template <int D, int KTMAX, bool MASKED>
__global__ __launch_bounds__(WF_NW * WAVE) void wfit_pass_kernel(WFitArgs a) {
    using G = WGeo<D>;
    __shared__ float lds[KTMAX * 16 * G::STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, kk = lane >> 4;
    const int KT = KTMAX == 1 ? 1 : (a.K + 15) / 16;

    for (int i = threadIdx.x; i < a.K * G::PACK; i += WF_NW * WAVE) lds[(i / G::PACK) * G::STRIDE + i % G::PACK] = a.pack[i];
    __syncthreads();
    WParams<D> p;
    if constexpr (KTMAX == 1) p.load(lds + (i16 < a.K ? i16 : 0) * G::STRIDE);   // lanes beyond K: a readable component, its term forced to -inf

    const long long g = (long long)blockIdx.x * WF_NW + wave;
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

    for (long long c0 = r0; c0 < r1; c0 += WF_CHUNK) {
        const long long c1 = c0 + WF_CHUNK < r1 ? c0 + WF_CHUNK : r1;
        for (long long n4 = c0; n4 < c1; n4 += 4) {
            const long long n = n4 + kk;
            const bool valid = n < c1;
            const long long nr = valid ? n : c1 - 1;                         // rows past the range: a row of the range, discarded
            float x[D];
            bool miss[D];
            const int n_obs = wfit_load_row<D, MASKED>(a, nr, x, miss);
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
            wfit_flush<D>(acc, slab + i16 * G::MW, c0 == r0, kk == 0 && i16 < a.K);
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
                    wfit_load_row<D, MASKED>(a, nr, x, miss);
                    const float w = a.w[nr];
                    WCell<D, MASKED> cell;
                    cell.eval(p, x, miss);
                    const float rk = (valid && k < a.K) ? a.r[n * a.K + k] : 0.f;      // the lane's own store of the first walk
                    cell.moments(miss, w != 0.f ? w * rk : 0.f, acc);
                }
                wfit_flush<D>(acc, slab + (k < a.K ? k : 0) * G::MW, c0 == r0, kk == 0 && k < a.K);
            }
        }
    }
    wave_block_sum<WF_NW>(dsum, lane, wave, a.partials);
}

__global__ __launch_bounds__(WAVE) void wfit_sum_kernel(const double* partials, int nblk, double* out) { block_sum(partials, nblk, out); }

struct WFitReduceArgs {
    const double* slab;
    const float* pack;
    double* stats;        // (K, SW)
    int nwaves, K;
};

// One block per component: wave group j adds waves j, j + 16, ... in that order, the 16 group sums are added in group order, then
// the shift by m_k (the fp32 words of the pack, exact in fp64) is undone:
//   sx = s1 + Nk m,   sxx = s2 + s1 m^T + m s1^T + Nk m m^T;   word 1 (Wk) = word 0 (Nk).
template <int D>
__global__ __launch_bounds__(WF_RED_GROUPS * WAVE) void wfit_unshift_kernel(WFitReduceArgs a) {
    using G = WGeo<D>;
    __shared__ double part[WF_RED_GROUPS][WAVE];
    __shared__ double red[WAVE];
    const int k = blockIdx.x, grp = threadIdx.x >> 6, i = threadIdx.x & 63;
    double s = 0.0;
    if (i < G::MW)
        for (int w = grp; w < a.nwaves; w += WF_RED_GROUPS) s += a.slab[((long long)w * a.K + k) * G::MW + i];
    part[grp][i] = s;
    __syncthreads();
    if (grp == 0) {
        double t = part[0][i];
#pragma unroll
        for (int j = 1; j < WF_RED_GROUPS; ++j) t += part[j][i];
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

template <int D, bool MASKED>
int launch_wfit(const WFitArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(WF_NW * WAVE);
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
    return wfit_slab_bytes(N, D, K) + (size_t)wfit_blocks(N) * sizeof(double);         // the fp64 moments of every wave | one partial per block
}

int vmp_mixture_wfit_pass(const float* x, const float* w, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* r_out,
                          float* logr_out, float* x_fill_out, double* stats_out, double* bound_out, void* ws, size_t ws_bytes,
                          void* stream) {
    int rc = wfit_pass_check("vmp_mixture_wfit_pass", x, w, mask, N, D, K, pack, r_out, logr_out, x_fill_out, stats_out, bound_out, ws,
                             ws_bytes);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = wfit_blocks(N);
    const long long waves = (long long)blocks * WF_NW;
    WFitArgs a{};
    a.x = x; a.w = w; a.mask = mask; a.pack = pack; a.r = r_out; a.logr = logr_out; a.x_fill = x_fill_out;
    a.slab = static_cast<double*>(ws);
    a.partials = reinterpret_cast<double*>(static_cast<char*>(ws) + wfit_slab_bytes(N, D, K));
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
            hipLaunchKernelGGL((wfit_unshift_kernel<DD>), dim3(K), dim3(WF_RED_GROUPS * WAVE), 0, s, ra);
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
    if (iterations < 0) { set_error("vmp_mixture_wfit_iterate: iterations must not be negative (got %d)", iterations); return VMP_E_BADARG; }
    if (!alpha0 || !beta0 || !m0 || !C0 || !v0 || !alpha || !beta || !m || !C || !v) {
        set_error("vmp_mixture_wfit_iterate: null pointer (prior or posterior)");
        return VMP_E_BADARG;
    }
    for (int it = 0; it < iterations; ++it) {
        rc = vmp_mix_finalize(stats, D, K, VMP_GMM, alpha0, beta0, m0, C0, v0, nullptr, alpha, beta, m, C, v, xbar, S, pi, nullptr, stream);
        if (rc) return rc;
        if ((rc = vmp_mixture_fit_pack(D, K, alpha, beta, m, C, v, pack, stream)) != 0) return rc;
        if ((rc = vmp_mixture_wfit_pass(x, w, mask, N, D, K, pack, r, logr, x_fill, stats, bound, ws, ws_bytes, stream)) != 0) return rc;
    }
    return 0;
}

}  // extern "C"
