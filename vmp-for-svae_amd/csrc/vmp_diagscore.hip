// Diagonal-covariance Gaussian mixture: log posterior predictive density, predictive responsibilities and conditional-mean fills of
// rows of up to VMP_DIAG_MAX_D = 64 columns, complete or partly observed, in one streaming pass (include/vmp_hip.h "Diagonal-covariance
// mixture: scoring and filling wide rows").  Given z = k the predictive factorises over the coordinates into one-dimensional
// Student-t densities with 2 a_k degrees of freedom:
//   g_kd = beta_k / (2 b_kd (1 + beta_k)),   G_k = lgamma(a_k + 1/2) - lgamma(a_k) - 1/2 log pi,   h_kd = G_k + 1/2 log g_kd
//   l_nk = log w_k + sum_{d in o(n)} [ h_kd - (a_k + 1/2) log1p(g_kd (x_nd - m_kd)^2) ],   logp_n = logsumexp_k l_nk
// The pack is [ m (D) | g (D) | h (D) | log w | a + 1/2 | c = log w + sum_d h_d ] per component, fp32.
//
// The pass kernel is the E-part of diag_pass_kernel (vmp_diagfit.hip; what the two files share is in vmp_diag_stream.h): 4 waves per
// block, wave g owns the rows [g rpw, (g+1) rpw), walks them in tiles of 64, lane = row.  A tile of x (and of the mask bytes) is copied to the wave's own LDS with coalesced loads, so the
// alignment of x changes no bit; the row's D values sit in registers and the pack words are wave-uniform scalar operands.
//
// sum_d log1p(t_d), t_d = g_d (x_d - m_d)^2 >= 0.  a_k grows like N_k / 2 while t shrinks like 1 / N_k, so log1p has to be accurate
// RELATIVE TO t: rounding 1 + t first costs 6e-8 absolute, times a_k.  Two steps, both exact in that sense:
//   - DS_GROUP = 4 cells are merged in "t-space": (1 + T)(1 + t) - 1 = T + t + T t, all terms non-negative, so the merged T keeps
//     its relative accuracy (one rounding of the size of T per operation, what a running sum of four log1p would lose as well);
//   - log1p(T) = log(u) + e / u with u = fl(1 + T) and e = T - (u - 1) the exact rounding error of that sum (u - 1 is exact for
//     u < 2^24, e is then representable); the neglected term is e^2 / (2 u^2) < 2e-15.  v_log_f32 is accurate relative to its result.
// One v_log_f32 and one v_rcp_f32 per four cells instead of per cell.  T is clamped at 3e38 (a NaN stays a NaN): an overflow gives a
// finite, very negative term, never inf - inf.  Four cells overflow together only past an average t of 4e9 per cell.
//
// Masked rows: the lane holds o_d = 1 / 0 (observed / missing) and x_d with 0 in the missing slots, selected when the tile is read, so
// what a missing slot holds never enters arithmetic; the deviation is fma(-m_d, o_d, x_d), exactly x_d - m_d or 0, and the h_d of the
// observed coordinates are added in d order.  mask == NULL is its own instantiation without any of this.
// The rows' logp are added in fp64 in a fixed order: a lane's rows, the lanes of a wave (a fixed butterfly), the waves of a block,
// the blocks (dscore_rowsum_kernel, one wave).  No atomics; the geometry depends on N only.
#include "vmp_diag_stream.h"

using namespace vmp;

namespace {

constexpr int DS_GROUP = 4;                   // cells merged before one logarithm
constexpr int DS_ROWS_PER_BLOCK = 1024;
constexpr int DS_MAX_BLOCKS = 2048;
constexpr int DS_FENCE = 16;                  // cells between two scheduling fences of a component's chain
constexpr float DS_TMAX = 3e38f;
constexpr float DS_LN2 = 0.693147180559945309f;

inline int dscore_blocks(int64_t N) { return stream_blocks(N, DS_ROWS_PER_BLOCK, DS_MAX_BLOCKS); }
// bytes of a row of the mask tile: a multiple of 4 with an odd word count, so the 64 lanes read 64 different banks
constexpr int dscore_mask_stride(int D) { return 4 * (((D + 3) / 4) | 1); }
inline size_t dscore_lds_bytes(int D, int K, bool masked) {
    return (size_t)DIAG_NW * DIAG_TILE * (((D | 1) + (K | 1)) * sizeof(float) + (masked ? dscore_mask_stride(D) : 0));
}

struct DScoreArgs {
    const float* x;
    const uint8_t* mask;  // (N,D) or NULL (then the kernel is the unmasked instantiation)
    float* logp;          // (N) or NULL
    float* resp;          // (N,K) or NULL
    float* x_out;         // (N,D) or NULL; may be x
    double* partials;     // (blocks) fp64 or NULL
    long long N;
    long long rpw;        // rows per wave, a multiple of 64
    int K;
};

template <int D, bool MASKED>
__global__ __launch_bounds__(DIAG_NW * WAVE) void dscore_pass_kernel(DScoreArgs a, const float* __restrict__ pack) {
    extern __shared__ float ds_lds[];
    __shared__ double wsum[DIAG_NW];
    constexpr int XS = D | 1, PW = 3 * D + 3, MS = dscore_mask_stride(D);
    const int K = a.K, RS = K | 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xs = ds_lds + wave * DIAG_TILE * (XS + RS);
    float* rs = xs + DIAG_TILE * XS;
    uint8_t* mb = reinterpret_cast<uint8_t*>(ds_lds + DIAG_NW * DIAG_TILE * (XS + RS)) + wave * DIAG_TILE * MS;

    const long long g = (long long)blockIdx.x * DIAG_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    cfloat* cpack = (cfloat*)pack;
    double dsum = 0.0;                                                       // the lane's rows' logp, in row order

    for (long long t0 = r0; t0 < r1; t0 += DIAG_TILE) {
        const int rows = r1 - t0 < DIAG_TILE ? (int)(r1 - t0) : DIAG_TILE;
        const bool valid = lane < rows;
        tile_stage(a.x + t0 * D, xs, rows * D, D, XS, lane);
        if (MASKED) tile_stage(a.mask + t0 * D, mb, rows * D, D, MS, lane);
        __builtin_amdgcn_wave_barrier();
        float x[D], o[MASKED ? D : 1];
        unsigned mlo = 0u, mhi = 0u;                                         // bit d of (mhi, mlo): coordinate d is missing
        if constexpr (MASKED) {
#pragma unroll 1
            for (int d = 0; d < D; ++d) {
                const unsigned gone = mb[lane * MS + d] != 0;
                if (d < 32) mlo |= gone << d; else mhi |= gone << (d - 32);
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = xs[lane * XS + d];
            if constexpr (MASKED) {
                const unsigned gone = ((d < 32 ? mlo : mhi) >> (d & 31)) & 1u;
                o[d] = 1.0f - (float)gone;
                x[d] = __uint_as_float(__float_as_uint(x[d]) & (gone - 1u));   // what a missing slot holds ends here: +0 (bit
                                                                             // arithmetic: a compare per coordinate costs an SGPR pair)
            }
        }
        float ml = -INFINITY;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            cfloat* p = cpack + k * PW;
            float l2[4] = {0.f, 0.f, 0.f, 0.f}, corr[4] = {0.f, 0.f, 0.f, 0.f}, hs[4] = {0.f, 0.f, 0.f, 0.f};   // four partial sums each,
                                                                             // added pairwise at the end: shorter rounding chains
#pragma unroll
            for (int g0 = 0; g0 < D; g0 += DS_GROUP) {
                // the scheduler would otherwise start every scalar load of the component at once and run out of SGPRs
                if (g0 && g0 % DS_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
                float T = 0.f;
#pragma unroll
                for (int j = 0; j < DS_GROUP; ++j) {
                    const int d = g0 + j;
                    if (d < D) {
                        float dev;
                        if constexpr (MASKED) {
                            dev = fmaf(-p[d], o[d], x[d]);
                        } else {
                            dev = x[d] - p[d];
                        }
                        const float t = (dev * p[D + d]) * dev;
                        T = j == 0 ? t : fmaf(T, t, T + t);
                    }
                }
                T = T > DS_TMAX ? DS_TMAX : T;
                const float u = 1.0f + T;
                const float e = T - (u - 1.0f);
                l2[(g0 / DS_GROUP) & 3] += __log2f(u);
                corr[(g0 / DS_GROUP) & 3] = fmaf(e, __builtin_amdgcn_rcpf(u), corr[(g0 / DS_GROUP) & 3]);
            }
            if constexpr (MASKED) {                                          // the h_d of the observed coordinates, d order; a loop
#pragma unroll                                                               // of its own: m, g and h in one chain are too many SGPRs
                for (int d = 0; d < D; ++d) {
                    if (d % DS_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
                    hs[d & 3] = fmaf(o[d], p[2 * D + d], hs[d & 3]);
                }
            }
            const float hsum = (hs[0] + hs[1]) + (hs[2] + hs[3]);
            const float s = fmaf((l2[0] + l2[1]) + (l2[2] + l2[3]), DS_LN2, (corr[0] + corr[1]) + (corr[2] + corr[3]));
            const float l = MASKED ? fmaf(-p[3 * D + 1], s, p[3 * D] + hsum) : fmaf(-p[3 * D + 1], s, p[3 * D + 2]);
            rs[lane * RS + k] = l;
            ml = fmaxf(ml, l);
        }
        const float shift = ml == -INFINITY ? 0.f : ml;                      // every term -inf: -inf - (-inf) would be NaN
        float se = 0.f;
#pragma unroll 1
        for (int k = 0; k < K; ++k) se += __expf(rs[lane * RS + k] - shift);
        const float inv = se == 0.f ? 0.f : 1.0f / se;                       // a row without mass: resp = 0
        const float lse = shift + logf(se);
        if (valid) {
            dsum += (double)lse;
            if (a.logp) a.logp[t0 + lane] = lse;
        }
        const bool fill = MASKED && a.x_out;
        if (a.resp || fill) {
#pragma unroll 1
            for (int k = 0; k < K; ++k) rs[lane * RS + k] = __expf(rs[lane * RS + k] - shift) * inv;
        }
        if (fill) {                                                          // sum_k resp_k m_kd into the missing slots, k order
            float xh[D];
#pragma unroll
            for (int d = 0; d < D; ++d) xh[d] = 0.f;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                cfloat* p = cpack + k * PW;
                const float r = rs[lane * RS + k];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (d && d % DS_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
                    xh[d] = fmaf(r, p[d], xh[d]);
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const unsigned gone = ((d < 32 ? mlo : mhi) >> (d & 31)) & 1u;   // x[d] is +0 where gone: OR the fill in
                xs[lane * XS + d] = __uint_as_float(__float_as_uint(x[d]) | (__float_as_uint(xh[d]) & (0u - gone)));
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (a.resp) tile_store(a.resp + t0 * K, rs, rows * K, K, RS, lane);  // the tile of resp is contiguous in resp_out
        if (fill) {                                                          // and so is the tile of x_out (D is a constant here: in
            float* dst = a.x_out + t0 * D;                                   // tile_store the column walk gets another closed form)
            const int total = rows * D;
            int row = lane / D, col = lane % D;
            for (int i = lane; i < total; i += WAVE) {
                dst[i] = xs[row * XS + col];
                col += WAVE;
                while (col >= D) { col -= D; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // lanes (a fixed butterfly), waves, then one word per block
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) dsum += __shfl_xor(dsum, off);
    if (lane == 0) wsum[wave] = dsum;
    __syncthreads();
    if (threadIdx.x == 0 && a.partials) {
        double s = wsum[0];
#pragma unroll
        for (int j = 1; j < DIAG_NW; ++j) s += wsum[j];
        a.partials[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(WAVE) void dscore_rowsum_kernel(const double* partials, int nblk, double* out) { block_sum(partials, nblk, out); }

// lgamma(a + 1/2) - lgamma(a) for a > 0 and finite, NaN otherwise.  Each lgamma is of the size of a log a: their difference at
// a = 5e7 keeps 1e-7 of absolute error in fp64.  From a = 16 on the Stirling series of the difference is used instead, and nothing
// of the size of a is ever formed:  1/2 log a - 1/(8 a) + 1/(192 a^3) - 1/(640 a^5) + 17/(14336 a^7)   (next term 31/(18432 a^9) < 3e-14)
__device__ __forceinline__ double dscore_lgamma_half(double a) {
    if (!(a > 0.0 && a < 1e300)) return __builtin_nan("");
    if (a < 16.0) return lgamma(a + 0.5) - lgamma(a);
    const double f = 1.0 / (a * a);
    return 0.5 * log(a) - (1.0 / a) * (1.0 / 8 - f * (1.0 / 192 - f * (1.0 / 640 - f * (17.0 / 14336))));
}

struct DScorePackArgs {
    const float *alpha, *beta, *m, *a, *b;
    float* pack;
    int D, K;
};

// one block per component, lane d; the sum over d by every lane in d order.  alpha, beta, a or a b not positive: a NaN row.
__global__ __launch_bounds__(WAVE) void dscore_pack_kernel(DScorePackArgs a) {
    __shared__ double hs[WAVE];
    __shared__ int bad[WAVE];
    const int k = blockIdx.x, d = threadIdx.x, D = a.D, PW = 3 * D + 3;
    const double ak = a.a[k], bk = a.beta[k], al = a.alpha[k];
    const double G = dscore_lgamma_half(ak) - 0.57236494292470008707;        // 1/2 log pi
    double gd = 0.0, hd = 0.0;
    hs[d] = 0.0;
    bad[d] = 0;
    if (d < D) {
        const double b = a.b[k * D + d];
        bad[d] = !(b > 0.0);
        gd = bk / (2.0 * b * (1.0 + bk));
        hd = G + 0.5 * log(gd);
        hs[d] = b > 0.0 ? hd : 0.0;
    }
    __syncthreads();
    double s = 0.0;
    int nbad = !(ak > 0.0) || !(bk > 0.0) || !(al > 0.0);
    for (int j = 0; j < D; ++j) { s += hs[j]; nbad += bad[j]; }
    const float qnan = __builtin_nanf("");
    float* out = a.pack + (long long)k * PW;
    if (d < D) {
        out[d] = nbad ? qnan : a.m[k * D + d];
        out[D + d] = nbad ? qnan : (float)gd;
        out[2 * D + d] = nbad ? qnan : (float)hd;
    }
    if (d == 0) {
        double asum = 0.0;
        for (int j = 0; j < a.K; ++j) asum += a.alpha[j];
        const double lw = log(al / asum);
        out[3 * D] = nbad ? qnan : (float)lw;
        out[3 * D + 1] = nbad ? qnan : (float)(ak + 0.5);
        out[3 * D + 2] = nbad ? qnan : (float)(lw + s);
    }
}

int launch_dscore_dim(int D, const DScoreArgs& a, const float* pack, int blocks, size_t lds, hipStream_t s) {
    return dispatch_dim<VMP_DIAG_MAX_D>(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        return a.mask ? launch_dyn_lds(dscore_pass_kernel<DD, true>, "dscore_pass_kernel", blocks, DIAG_NW * WAVE, lds, s, a, pack)
                      : launch_dyn_lds(dscore_pass_kernel<DD, false>, "dscore_pass_kernel", blocks, DIAG_NW * WAVE, lds, s, a, pack);
    });
}

}  // namespace

extern "C" {

int vmp_mixture_diag_score_pack_words(int D) { return (D < 1 || D > VMP_DIAG_MAX_D) ? 0 : 3 * D + 3; }

size_t vmp_mixture_diag_score_workspace_bytes(int64_t N, int D, int K) {
    if (D < 1 || D > VMP_DIAG_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    return (size_t)dscore_blocks(N) * sizeof(double);                        // one fp64 partial per block
}

int vmp_mixture_diag_score_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* a, const float* b,
                                float* pack, void* stream) {
    int rc = stream_dims("vmp_mixture_diag_score_pack", D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (!alpha || !beta || !m || !a || !b || !pack) {
        set_error("vmp_mixture_diag_score_pack: null pointer (posterior or pack)");
        return VMP_E_BADARG;
    }
    DScorePackArgs pa{alpha, beta, m, a, b, pack, D, K};
    hipLaunchKernelGGL(dscore_pack_kernel, dim3(K), dim3(WAVE), 0, static_cast<hipStream_t>(stream), pa);
    return check_launch("dscore_pack_kernel");
}

int vmp_mixture_diag_score(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, float* logp_out,
                           float* resp_out, float* x_out, double* sum_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "vmp_mixture_diag_score";
    int rc = stream_dims(who, D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !pack) { set_error("%s: null pointer (%s)", who, !x ? "x" : "pack"); return VMP_E_BADARG; }
    if (!logp_out && !resp_out && !x_out && !sum_out) {
        set_error("%s: no output requested (logp_out, resp_out, x_out and sum_out are all NULL)", who);
        return VMP_E_BADARG;
    }
    if (x_out && !mask) { set_error("%s: x_out needs a mask (without one there is nothing to fill)", who); return VMP_E_BADARG; }
    if ((rc = sum_workspace_check(who, sum_out, ws, ws_bytes, vmp_mixture_diag_score_workspace_bytes(N, D, K))) != 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = dscore_blocks(N);
    DScoreArgs a{};
    a.x = x; a.mask = mask; a.logp = logp_out; a.resp = resp_out; a.x_out = x_out;
    a.partials = sum_out ? static_cast<double*>(ws) : nullptr;
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, (long long)blocks * DIAG_NW, DIAG_TILE);
    if ((rc = launch_dscore_dim(D, a, pack, blocks, dscore_lds_bytes(D, K, mask != nullptr), s)) != 0) return rc;
    if (sum_out) {
        hipLaunchKernelGGL(dscore_rowsum_kernel, dim3(1), dim3(WAVE), 0, s, a.partials, blocks, sum_out);
        rc = check_launch("dscore_rowsum_kernel");
    }
    return rc;
}

}  // extern "C"
