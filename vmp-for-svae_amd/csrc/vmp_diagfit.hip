// Diagonal-covariance Gaussian mixture fit for rows of up to VMP_DIAG_MAX_D = 64 columns (include/vmp_hip.h "Diagonal-covariance
// mixture fitting on wide rows").  Posterior theta = (alpha (K), beta (K), m (K,D), a (K), b (K,D)): pi ~ Dir(alpha),
// lambda_kd ~ Gamma(a_k, rate b_kd), mu_kd | lambda_kd ~ N(m_kd, (beta_k lambda_kd)^-1).  With lbar_kd = a_k / b_kd:
//   c_k      = psi(alpha_k) - psi(sum alpha) + 1/2 sum_d (psi(a_k) - log b_kd) - D / (2 beta_k)
//   log rho_nk = c_k - 1/2 sum_d lbar_kd (x_nd - m_kd)^2,      r_nk = softmax_k log rho_nk
//   Nk = sum_n r_nk,  sx_kd = sum_n r_nk x_nd,  sxx_kd = sum_n r_nk x_nd^2,     data = sum_n logsumexp_k log rho_nk - 1/2 N D log 2 pi
// The pack is [ m (D) | lbar (D) | c ] per component, fp32.
//
// The pass kernel: 4 waves per block, wave g owns the rows [g rpw, (g+1) rpw) (rpw a multiple of 64) and walks them in tiles of 64
// rows.  A tile of x is copied to the wave's own LDS with coalesced dword loads (any alignment of x).  What this kernel shares with
// the scoring pass (vmp_diagscore.hip) - tile movement, launch and dispatch - is in vmp_diag_stream.h.  Then two lane maps:
//   E-part   lane = row.  The row's D values sit in registers; component k's m, lbar and c are wave-uniform and come through scalar
//            loads (the pack is read through the constant address space); log rho is formed on x - m, never in the expanded form.
//            log rho, then r, go to the wave's LDS tile rs (64, K); r_out is written from there with coalesced stores.
//   M-part   r^T [y | y^2] with y = x - pivot as v_mfma_f32_16x16x4_f32: A = r (lane = (component, row of a 4-row step)), B = y or
//            y^2 (lane = (column, row)), one 16 x 16 accumulator tile per (component tile, column tile).  The MFMA is the cross-lane
//            reduction: an accumulator word belongs to one (k, d) and one lane.  Nk is the sum of the A operands a lane has loaded.
//            A chain of MFMAs covers 16 rows from zero; the 16-row sums are added to the fp32 accumulators on the VALU.
// The pivot is ONE point near the data, the mean of up to 64 evenly strided rows, a function of (x, N, D) alone; every block forms the
// same bits and block 0 leaves them in the workspace for the reducing launch.  The fp32 accumulators are added to the wave's own fp64
// words every 128 rows (a plain read-modify-write), and the reducing launch adds the waves in a fixed order and undoes the shift in
// fp64.  The rows' log-sum-exp are added in fp64 in a fixed order: a lane's rows, the lanes of a wave (a fixed butterfly), the waves
// of a block, the blocks (by block 0 of the reducing launch).  No atomics; the geometry depends on (N, D, K) only: stats and data are
// bit-identical from run to run and for every set of optional outputs.
#include "vmp_diag_stream.h"

using namespace vmp;

namespace {

constexpr int DG_FLUSH_TILES = 2;             // tiles between two fp32 -> fp64 flushes: 128 rows of a wave
constexpr int DG_ROWS_PER_BLOCK = 2048;       // below that a block is not worth its launch slot
constexpr int DG_RED_GROUPS = 16;             // wave groups of the reduction block
constexpr int DG_PIVOT_ROWS = 64;

// the slab of a wave is K (1 + 2 D) fp64 words: at most 512 blocks while that stays within 16 KB, 256 beyond
inline int diag_max_blocks(int D, int K) { return K * (1 + 2 * D) <= 2048 ? 512 : 256; }
inline int diag_blocks(int64_t N, int D, int K) { return stream_blocks(N, DG_ROWS_PER_BLOCK, diag_max_blocks(D, K)); }
inline size_t diag_slab_bytes(int64_t N, int D, int K) { return (size_t)diag_blocks(N, D, K) * DIAG_NW * K * (1 + 2 * D) * sizeof(double); }
inline size_t diag_lds_bytes(int D, int K) { return (size_t)(64 + DIAG_NW * DIAG_TILE * ((D | 1) + (K | 1))) * sizeof(float); }

struct DiagArgs {
    const float* x;
    const float* r_in;    // (N,K) or NULL: responsibilities of the caller in place of the E-part
    float* r;             // (N,K) or NULL
    float* logr;          // (N,K) or NULL
    double* slab;         // (waves, K, 1 + 2 D) fp64
    double* partials;     // (blocks) fp64
    float* pivot;         // (64) fp32, written by block 0
    long long N;
    long long rpw;        // rows per wave, a multiple of 64
    int K;
};

template <int D, int KTMAX>
__global__ __launch_bounds__(DIAG_NW * WAVE) void diag_pass_kernel(DiagArgs a, const float* __restrict__ pack) {
    extern __shared__ float dg_lds[];
    __shared__ double wsum[DIAG_NW];
    constexpr int XS = D | 1, FT = (D + 15) / 16, PW = 2 * D + 1, SW = 1 + 2 * D;
    const int K = a.K, RS = K | 1, KT = (K + 15) / 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, j4 = lane >> 4;
    float* pv = dg_lds;
    float* xs = dg_lds + 64 + wave * DIAG_TILE * (XS + RS);
    float* rs = xs + DIAG_TILE * XS;

    // the pivot: column means of up to 64 evenly strided rows, added in row order
    if (threadIdx.x < D) {
        const long long cnt = a.N < DG_PIVOT_ROWS ? a.N : DG_PIVOT_ROWS, stride = a.N / cnt;
        float s = 0.f;
        for (long long j = 0; j < cnt; ++j) s += a.x[j * stride * D + threadIdx.x];
        s = s / (float)cnt;
        pv[threadIdx.x] = s;
        if (blockIdx.x == 0) a.pivot[threadIdx.x] = s;
    }
    __syncthreads();
    float pvr[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) pvr[ft] = 16 * ft + i16 < D ? pv[16 * ft + i16] : 0.f;

    const long long g = (long long)blockIdx.x * DIAG_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    double* slab = a.slab + g * K * SW;
    cfloat* cpack = (cfloat*)pack;
    double dsum = 0.0;                                                       // the lane's rows' log-sum-exp, in row order

    f32x4 acc1[KTMAX][FT], acc2[KTMAX][FT];
    float nk[KTMAX];
#pragma unroll
    for (int kt = 0; kt < KTMAX; ++kt) {
        nk[kt] = 0.f;
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) { acc1[kt][ft] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[kt][ft] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }

    if (r0 >= r1)                                                            // a wave without rows: its moments are zero
        for (int i = lane; i < K * SW; i += WAVE) slab[i] = 0.0;

    int tile = 0;
    for (long long t0 = r0; t0 < r1; t0 += DIAG_TILE, ++tile) {
        const int rows = r1 - t0 < DIAG_TILE ? (int)(r1 - t0) : DIAG_TILE;
        tile_stage(a.x + t0 * D, xs, rows * D, D, XS, lane);
        if (a.r_in) {
            tile_stage(a.r_in + t0 * K, rs, rows * K, K, RS, lane);
        } else {
            __builtin_amdgcn_wave_barrier();
            float x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = xs[lane * XS + d];
            const bool valid = lane < rows;
            float ml = -INFINITY;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                cfloat* p = cpack + k * PW;
                float q = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float t = x[d] - p[d];
                    q = fmaf(t * p[D + d], t, q);
                }
                const float l = fmaf(-0.5f, q, p[2 * D]);
                rs[lane * RS + k] = l;
                ml = fmaxf(ml, l);
            }
            const float shift = ml == -INFINITY ? 0.f : ml;                  // every term -inf: -inf - (-inf) would be NaN
            float s = 0.f;
#pragma unroll 1
            for (int k = 0; k < K; ++k) s += __expf(rs[lane * RS + k] - shift);
            const float inv = s == 0.f ? 0.f : 1.0f / s;                     // a row without mass: r = 0
            const float lse = shift + logf(s);
            if (valid) dsum += (double)lse;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float l = rs[lane * RS + k];
                if (a.logr && valid) a.logr[(t0 + lane) * K + k] = l - lse;
                rs[lane * RS + k] = valid ? __expf(l - shift) * inv : 0.f;   // rows past the range add nothing to the moments
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (a.r) tile_store(a.r + t0 * K, rs, rows * K, K, RS, lane);        // the tile of r is contiguous in r_out
        // M-part: four rows per step, lane = (i16, j4): A = r[row j4][component 16 kt + i16], B = y[row j4][column 16 ft + i16]
        // The MFMA chain of a (kt, ft) tile runs over the 4 steps of a 16-row group from zero; the group's sums are then added to the
        // accumulators on the VALU (round to nearest).  A chain over all 32 steps between two flushes rounds at the size of the running
        // sum at every step; this way only 8 additions per flush interval do.
#pragma unroll 1
        for (int sg = 0; sg < DIAG_TILE / 16; ++sg) {
            float av[4][KTMAX];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int row = 16 * sg + 4 * st + j4;
#pragma unroll
                for (int kt = 0; kt < KTMAX; ++kt) {
                    av[st][kt] = 16 * kt + i16 < K ? rs[row * RS + 16 * kt + i16] : 0.f;
                    nk[kt] += av[st][kt];
                }
            }
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                f32x4 g1[KTMAX], g2[KTMAX];
#pragma unroll
                for (int kt = 0; kt < KTMAX; ++kt) { g1[kt] = f32x4{0.f, 0.f, 0.f, 0.f}; g2[kt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int row = 16 * sg + 4 * st + j4;
                    const float y = 16 * ft + i16 < D ? xs[row * XS + 16 * ft + i16] - pvr[ft] : 0.f;
                    const float y2 = y * y;
#pragma unroll
                    for (int kt = 0; kt < KTMAX; ++kt) {
                        if (kt < KT) {
                            g1[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st][kt], y, g1[kt], 0, 0, 0);
                            g2[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st][kt], y2, g2[kt], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int kt = 0; kt < KTMAX; ++kt) {
                    if (kt < KT) { acc1[kt][ft] += g1[kt]; acc2[kt][ft] += g2[kt]; }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (tile % DG_FLUSH_TILES == DG_FLUSH_TILES - 1 || t0 + DIAG_TILE >= r1) {
            // accumulator word v of tile (kt, ft) in lane (i16, j4): component 16 kt + 4 j4 + v, column 16 ft + i16
            const bool first = tile < DG_FLUSH_TILES;
#pragma unroll
            for (int kt = 0; kt < KTMAX; ++kt) {
                if (kt < KT) {
#pragma unroll
                    for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int k = 16 * kt + 4 * j4 + v, f = 16 * ft + i16;
                            if (k < K && f < D) {
                                double* w = slab + k * SW;
                                w[1 + f] = (first ? 0.0 : w[1 + f]) + (double)acc1[kt][ft][v];
                                w[1 + D + f] = (first ? 0.0 : w[1 + D + f]) + (double)acc2[kt][ft][v];
                            }
                        }
                        acc1[kt][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
                        acc2[kt][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    const float sn = rows4_sum(nk[kt]);
                    const int k = 16 * kt + i16;
                    if (j4 == 0 && k < K) slab[k * SW] = (first ? 0.0 : slab[k * SW]) + (double)sn;
                    nk[kt] = 0.f;
                }
            }
        }
    }
    // lanes (a fixed butterfly), waves, then one word per block
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) dsum += __shfl_xor(dsum, off);
    if (lane == 0) wsum[wave] = dsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int j = 1; j < DIAG_NW; ++j) s += wsum[j];
        a.partials[blockIdx.x] = s;
    }
}

struct DiagReduceArgs {
    const double* slab;
    const double* partials;
    const float* pivot;
    double* stats;        // (K, 1 + 2 D) or NULL
    double* bound;        // (1) or NULL
    long long N;
    int nwaves, nblk, K, D;
};

// One block per component: lane d of wave group j adds Nk, s1_d and s2_d of the waves j, j + 16, ... in that order, the 16 group sums
// are added in group order, then the shift by the pivot p (fp32 words, exact in fp64) is undone:
//   sx = s1 + Nk p,   sxx = s2 + 2 p s1 + Nk p^2.
// Block 0 also adds the blocks' row sums (vmp_mix_stream.h block_sum) and subtracts 1/2 N D log 2 pi.
__global__ __launch_bounds__(DG_RED_GROUPS * WAVE) void diag_reduce_kernel(DiagReduceArgs a) {
    __shared__ double part[3][DG_RED_GROUPS][WAVE];
    __shared__ double bsum[WAVE];
    const int k = blockIdx.x, grp = threadIdx.x >> 6, d = threadIdx.x & 63;
    const int D = a.D, SW = 1 + 2 * D;
    if (a.stats) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (d < D)
            for (int w = grp; w < a.nwaves; w += DG_RED_GROUPS) {
                const double* p = a.slab + ((long long)w * a.K + k) * SW;
                s0 += p[0]; s1 += p[1 + d]; s2 += p[1 + D + d];
            }
        part[0][grp][d] = s0; part[1][grp][d] = s1; part[2][grp][d] = s2;
        __syncthreads();
        if (grp == 0 && d < D) {
            double t0 = part[0][0][d], t1 = part[1][0][d], t2 = part[2][0][d];
#pragma unroll
            for (int j = 1; j < DG_RED_GROUPS; ++j) { t0 += part[0][j][d]; t1 += part[1][j][d]; t2 += part[2][j][d]; }
            const double p = (double)a.pivot[d];
            double* out = a.stats + (long long)k * SW;
            if (d == 0) out[0] = t0;
            out[1 + d] = t1 + t0 * p;
            out[1 + D + d] = t2 + 2.0 * p * t1 + t0 * p * p;
        }
    }
    if (a.bound && blockIdx.x == 0 && grp == 0) {                            // one wave; its own LDS words, nobody else's
        double s = 0.0;
        for (int j = d; j < a.nblk; j += WAVE) s += a.partials[j];
        bsum[d] = s;
        __builtin_amdgcn_wave_barrier();
        if (d == 0) {
            double t = bsum[0];
            for (int j = 1; j < WAVE; ++j) t += bsum[j];
            *a.bound = t - 0.5 * (double)a.N * (double)D * 1.83787706640934548356;
        }
    }
}

// psi(x) for x > 0 and finite, NaN otherwise (digamma_d's recurrence does not end at -inf)
__device__ __forceinline__ double diag_psi(double x) { return (x > 0.0 && x < 1e300) ? digamma_d(x) : __builtin_nan(""); }
__device__ __forceinline__ double diag_lgamma(double x) { return (x > 0.0 && x < 1e300) ? lgamma(x) : __builtin_nan(""); }

// (a - a0) psi(a) - lgamma(a) - a for a > 0 and finite, NaN otherwise.  Each of the three is of the size of a log a, the sum of the size
// of log a: formed from them at a = 5e7 it keeps 1e-7 of absolute error.  From a = 10 on (where digamma_d is its asymptotic series
// too) the series of psi and of lgamma are combined term by term, and nothing of the size of a is ever formed:
//   (1/2 - a0) log a - (a - a0) / (2 a) - (a - a0) P(a) - 1/2 log 2 pi - Q(a),    P, Q: the Bernoulli tails of psi and lgamma
__device__ __forceinline__ double diag_gamma_rest(double a, double a0) {
    if (!(a > 0.0 && a < 1e300)) return __builtin_nan("");
    if (a < 10.0) return (a - a0) * digamma_d(a) - lgamma(a) - a;
    const double f = 1.0 / (a * a);
    const double P = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760))))));
    const double Q = (1.0 / a) * (1.0 / 12 - f * (1.0 / 360 - f * (1.0 / 1260 - f * (1.0 / 1680 - f * (1.0 / 1188 - f * (691.0 / 360360))))));
    return (0.5 - a0) * log(a) - 0.5 * (a - a0) / a - (a - a0) * P - 0.91893853320467274178 - Q;
}

struct DiagFinArgs {
    const double* stats;
    const float *alpha0, *beta0, *m0, *a0, *b0;
    float *alpha, *beta, *m, *a, *b, *xbar, *S, *pi;
    int D, K;
};

// thread (k, d); fp64 inside.  Nk = 0: the posterior of the component is its prior.
__global__ __launch_bounds__(256) void diag_mstep_kernel(DiagFinArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int D = a.D, SW = 1 + 2 * D;
    if (idx >= a.K * D) return;
    const int k = idx / D, d = idx % D;
    const double* st = a.stats + (long long)k * SW;
    const double Nk = st[0], sx = st[1 + d], sxx = st[1 + D + d];
    const double be0 = a.beta0[k], m0 = a.m0[idx], be = be0 + Nk;
    const bool some = Nk > 0.0;
    const double xbar = some ? sx / Nk : 0.0;
    double NS = some ? sxx - sx * sx / Nk : 0.0;
    NS = NS < 0.0 ? 0.0 : NS;                                                // rounding of the difference; a NaN stays a NaN
    const double dx = xbar - m0;
    a.m[idx] = (float)((be0 * m0 + sx) / be);
    a.b[idx] = (float)((double)a.b0[idx] + 0.5 * (NS + (be0 * Nk / be) * dx * dx));
    if (a.xbar) a.xbar[idx] = (float)xbar;
    if (a.S) a.S[idx] = (float)(some ? NS / Nk : 0.0);
    if (d == 0) {
        const double al = (double)a.alpha0[k] + Nk;
        a.alpha[k] = (float)al;
        a.beta[k] = (float)be;
        a.a[k] = (float)((double)a.a0[k] + 0.5 * Nk);
        if (a.pi) {
            double asum = 0.0;
            for (int j = 0; j < a.K; ++j) asum += (double)a.alpha0[j] + a.stats[(long long)j * SW];
            a.pi[k] = (float)exp(diag_psi(al) - diag_psi(asum));
        }
    }
}

struct DiagPackArgs {
    const float *alpha, *beta, *m, *a, *b;
    float* pack;
    int D, K;
};

// one block per component, lane d; the sum over d by lane 0 in d order.  b, a or beta not positive: a NaN row.
__global__ __launch_bounds__(WAVE) void diag_pack_kernel(DiagPackArgs a) {
    __shared__ double logb[WAVE];
    __shared__ int bad[WAVE];
    const int k = blockIdx.x, d = threadIdx.x, D = a.D, PW = 2 * D + 1;
    const double ak = a.a[k], bk = a.beta[k];
    double lam = 0.0;
    logb[d] = 0.0;
    bad[d] = 0;
    if (d < D) {
        const double b = a.b[k * D + d];
        bad[d] = !(b > 0.0);
        logb[d] = b > 0.0 ? log(b) : 0.0;
        lam = ak / b;
    }
    __syncthreads();
    double s = 0.0;
    int nbad = !(ak > 0.0) || !(bk > 0.0);
    for (int j = 0; j < D; ++j) { s += logb[j]; nbad += bad[j]; }
    const float qnan = __builtin_nanf("");
    float* out = a.pack + (long long)k * PW;
    if (d < D) {
        out[d] = nbad ? qnan : a.m[k * D + d];
        out[D + d] = nbad ? qnan : (float)lam;
    }
    if (d == 0) {
        double asum = 0.0;
        for (int j = 0; j < a.K; ++j) asum += a.alpha[j];
        const double c = diag_psi((double)a.alpha[k]) - diag_psi(asum) + 0.5 * (D * diag_psi(ak) - s) - 0.5 * D / bk;
        out[2 * D] = nbad ? qnan : (float)c;
    }
}

struct DiagTermsArgs {
    const float *alpha0, *beta0, *m0, *a0, *b0;
    const float *alpha, *beta, *m, *a, *b;
    double* out;          // [kl_pi | sum_kd kl_ng_kd | sum_d kl_ng_0d .. sum_d kl_ng_{K-1}d]
    int D, K;
};

// thread k owns component k and adds its D terms in d order; thread 0 adds in k order.  The -a of a (b0 - b) / b is taken into
// diag_gamma_rest, where it cancels in the series: a term is of the size of log a, not of a.
__global__ __launch_bounds__(WAVE) void diag_terms_kernel(DiagTermsArgs a) {
    __shared__ double ng[WAVE], dir[WAVE];
    const int k = threadIdx.x, D = a.D;
    double asum = 0.0, a0sum = 0.0;
    for (int j = 0; j < a.K; ++j) { asum += a.alpha[j]; a0sum += a.alpha0[j]; }
    if (k < a.K) {
        const double al = a.alpha[k], al0 = a.alpha0[k], be = a.beta[k], be0 = a.beta0[k], ak = a.a[k], ak0 = a.a0[k];
        const double common = 0.5 * log(be / be0) - 0.5 + 0.5 * be0 / be + diag_gamma_rest(ak, ak0) + diag_lgamma(ak0);
        double s = 0.0;
        for (int d = 0; d < D; ++d) {
            const double b = a.b[k * D + d], b0 = a.b0[k * D + d], dm = (double)a.m[k * D + d] - (double)a.m0[k * D + d];
            s += common + 0.5 * be0 * (ak / b) * dm * dm + ak0 * (log(b) - log(b0)) + ak * b0 / b;
        }
        ng[k] = s;
        dir[k] = diag_lgamma(al0) - diag_lgamma(al) + (al - al0) * (diag_psi(al) - diag_psi(asum));
        a.out[2 + k] = s;
    }
    __syncthreads();
    if (k == 0) {
        double sng = 0.0, sdir = diag_lgamma(asum) - diag_lgamma(a0sum);
        for (int j = 0; j < a.K; ++j) { sng += ng[j]; sdir += dir[j]; }
        a.out[0] = sdir;
        a.out[1] = sng;
    }
}

int launch_diag_dim(int D, const DiagArgs& a, const float* pack, int blocks, size_t lds, hipStream_t s) {
    return dispatch_dim<VMP_DIAG_MAX_D>(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        return a.K <= 16 ? launch_dyn_lds(diag_pass_kernel<DD, 1>, "diag_pass_kernel", blocks, DIAG_NW * WAVE, lds, s, a, pack)
                         : launch_dyn_lds(diag_pass_kernel<DD, 4>, "diag_pass_kernel", blocks, DIAG_NW * WAVE, lds, s, a, pack);
    });
}

// every refusal of the pass, decided on the host
int diag_pass_check(const char* who, const float* x, int64_t N, int D, int K, const float* pack, const float* r_in, const float* r_out,
                    const float* logr_out, const double* stats_out, const double* bound_out, const void* ws, size_t ws_bytes) {
    int rc = stream_dims(who, D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !pack) { set_error("%s: null pointer (%s)", who, !x ? "x" : "pack"); return VMP_E_BADARG; }
    if (!r_out && !logr_out && !stats_out && !bound_out) {
        set_error("%s: no output requested (r_out, logr_out, stats_out and bound_out are all NULL)", who);
        return VMP_E_BADARG;
    }
    if (!r_out && logr_out) { set_error("%s: logr_out needs r_out", who); return VMP_E_BADARG; }
    if (r_in && (r_out || logr_out || bound_out)) {
        set_error("%s: r_in gives the moments of the caller's responsibilities only (r_out, logr_out and bound_out must be NULL)", who);
        return VMP_E_BADARG;
    }
    return workspace_check(who, ws, ws_bytes, vmp_mixture_diag_workspace_bytes(N, D, K));
}

}  // namespace

extern "C" {

int vmp_mixture_diag_pack_words(int D) { return (D < 1 || D > VMP_DIAG_MAX_D) ? 0 : 2 * D + 1; }

size_t vmp_mixture_diag_workspace_bytes(int64_t N, int D, int K) {
    if (D < 1 || D > VMP_DIAG_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    // the fp64 moments of every wave | one fp64 partial per block | the pivot (64 fp32 words)
    return diag_slab_bytes(N, D, K) + (size_t)diag_blocks(N, D, K) * sizeof(double) + 64 * sizeof(float);
}

int vmp_mixture_diag_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* a, const float* b, float* pack,
                          void* stream) {
    int rc = stream_dims("vmp_mixture_diag_pack", D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (!alpha || !beta || !m || !a || !b || !pack) { set_error("vmp_mixture_diag_pack: null pointer (posterior or pack)"); return VMP_E_BADARG; }
    DiagPackArgs pa{alpha, beta, m, a, b, pack, D, K};
    hipLaunchKernelGGL(diag_pack_kernel, dim3(K), dim3(WAVE), 0, static_cast<hipStream_t>(stream), pa);
    return check_launch("diag_pack_kernel");
}

int vmp_mixture_diag_pass(const float* x, int64_t N, int D, int K, const float* pack, const float* r_in, float* r_out, float* logr_out,
                          double* stats_out, double* bound_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = diag_pass_check("vmp_mixture_diag_pass", x, N, D, K, pack, r_in, r_out, logr_out, stats_out, bound_out, ws, ws_bytes);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = diag_blocks(N, D, K);
    const long long waves = (long long)blocks * DIAG_NW;
    DiagArgs a{};
    a.x = x; a.r_in = r_in; a.r = r_out; a.logr = logr_out;
    a.slab = static_cast<double*>(ws);
    a.partials = reinterpret_cast<double*>(static_cast<char*>(ws) + diag_slab_bytes(N, D, K));
    a.pivot = reinterpret_cast<float*>(a.partials + blocks);
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, waves, DIAG_TILE);
    if ((rc = launch_diag_dim(D, a, pack, blocks, diag_lds_bytes(D, K), s)) != 0) return rc;
    if (stats_out || bound_out) {
        DiagReduceArgs ra{a.slab, a.partials, a.pivot, stats_out, bound_out, N, (int)waves, blocks, K, D};
        hipLaunchKernelGGL(diag_reduce_kernel, dim3(stats_out ? K : 1), dim3(DG_RED_GROUPS * WAVE), 0, s, ra);
        rc = check_launch("diag_reduce_kernel");
    }
    return rc;
}

int vmp_mixture_diag_finalize(const double* stats, int D, int K, const float* alpha0, const float* beta0, const float* m0, const float* a0,
                              const float* b0, float* alpha, float* beta, float* m, float* a, float* b, float* xbar, float* S, float* pi,
                              void* stream) {
    int rc = stream_dims("vmp_mixture_diag_finalize", D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (!stats || !alpha0 || !beta0 || !m0 || !a0 || !b0 || !alpha || !beta || !m || !a || !b) {
        set_error("vmp_mixture_diag_finalize: null pointer (stats, prior or posterior)");
        return VMP_E_BADARG;
    }
    DiagFinArgs fa{stats, alpha0, beta0, m0, a0, b0, alpha, beta, m, a, b, xbar, S, pi, D, K};
    hipLaunchKernelGGL(diag_mstep_kernel, dim3((K * D + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), fa);
    return check_launch("diag_mstep_kernel");
}

int vmp_mixture_diag_bound_terms(int D, int K, const float* alpha0, const float* beta0, const float* m0, const float* a0, const float* b0,
                                 const float* alpha, const float* beta, const float* m, const float* a, const float* b, double* out,
                                 void* stream) {
    int rc = stream_dims("vmp_mixture_diag_bound_terms", D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (!alpha0 || !beta0 || !m0 || !a0 || !b0 || !alpha || !beta || !m || !a || !b || !out) {
        set_error("vmp_mixture_diag_bound_terms: null pointer (prior, posterior or out)");
        return VMP_E_BADARG;
    }
    DiagTermsArgs ta{alpha0, beta0, m0, a0, b0, alpha, beta, m, a, b, out, D, K};
    hipLaunchKernelGGL(diag_terms_kernel, dim3(1), dim3(WAVE), 0, static_cast<hipStream_t>(stream), ta);
    return check_launch("diag_terms_kernel");
}

int vmp_mixture_diag_iterate(const float* x, int64_t N, int D, int K, const float* alpha0, const float* beta0, const float* m0,
                             const float* a0, const float* b0, float* r, float* logr, float* alpha, float* beta, float* m, float* a,
                             float* b, float* xbar, float* S, float* pi, float* pack, double* stats, double* bound, void* ws,
                             size_t ws_bytes, int iterations, void* stream) {
    if (!stats) {
        int rc = stream_dims("vmp_mixture_diag_iterate", D, K, VMP_DIAG_MAX_D);
        if (rc) return rc;
        set_error("vmp_mixture_diag_iterate: null pointer (stats)");
        return VMP_E_BADARG;
    }
    int rc = diag_pass_check("vmp_mixture_diag_iterate", x, N, D, K, pack, nullptr, r, logr, stats, bound, ws, ws_bytes);
    if (rc) return rc;
    if (iterations < 0) { set_error("vmp_mixture_diag_iterate: iterations must not be negative (got %d)", iterations); return VMP_E_BADARG; }
    if (!alpha0 || !beta0 || !m0 || !a0 || !b0 || !alpha || !beta || !m || !a || !b) {
        set_error("vmp_mixture_diag_iterate: null pointer (prior or posterior)");
        return VMP_E_BADARG;
    }
    for (int it = 0; it < iterations; ++it) {
        const bool last = it + 1 == iterations;
        if ((rc = vmp_mixture_diag_finalize(stats, D, K, alpha0, beta0, m0, a0, b0, alpha, beta, m, a, b, xbar, S, pi, stream)) != 0) return rc;
        if ((rc = vmp_mixture_diag_pack(D, K, alpha, beta, m, a, b, pack, stream)) != 0) return rc;
        if ((rc = vmp_mixture_diag_pass(x, N, D, K, pack, nullptr, last ? r : nullptr, last ? logr : nullptr, stats, bound, ws, ws_bytes,
                                        stream)) != 0) return rc;
    }
    return 0;
}

}  // extern "C"
