// Mixture sampling: seeded draws from a mixture of Student-t densities, unconditional or conditional on the observed part of each
// row (multiple imputation), in one streaming pass over (x, mask) with no workspace, no atomics and no second launch.
//
// A draw from the mixture is a conditional draw on a row with nothing observed (l_k = log w_k, conditional location mu,
// Lambda_mm = Lambda), so both are one kernel.  Per row, with the notation of vmp_impute.hip (o / m the observed / missing entries,
// D_o observed, R R^T = Lambda_mm, y = R^-1 Lambda_mo d_o, q = d_o^T Sigma_oo^-1 d_o, l_k, xhat_m^(k)), draw s is
//   component  resp_k = exp(l_k - logsumexp l) (the numbers of vmp_mixture_impute, same operations);  cdf_k = sum_{j <= k} resp_j;
//              z = first k with cdf_k > u_z;  none (rounding left the total below u_z): the last k with resp_k > 0;
//   scale      g ~ Gamma(a = (nu_z + D_o) / 2, rate 1/2), Marsaglia-Tsang (2000) on a' = a (a >= 1) or a + 1 (a < 1):
//              d = a' - 1/3, c = 1 / sqrt(9 d);  attempt t: w = 1 + c n_t, v = w^3, accepted if w > 0 and
//              log u_t < n_t^2 / 2 + d - d v + d log v;  gamma = d v of the first accepted attempt, d if all SMP_ATTEMPTS are rejected;
//              g = 2 gamma (a >= 1),  2 gamma u_b^(1/a) (a < 1), kept >= FLT_MIN;
//   entries    x_m = xhat_m^(z) + sqrt((nu_z + q_z) / g) R_z^-T eps;  observed entries are copied bit for bit.
// That is the conditional Student-t t_{nu + D_o}(xhat, (nu + q) / (nu + D_o) Lambda_mm^-1) of each component, mixed by resp.
// SMP_ATTEMPTS = 8: an attempt is rejected with probability 1 - e^d Gamma(a') d^-a' / (3 c sqrt(2 pi)) <= 0.0484 (its value at
// a' = 1, decreasing in a'), so all eight with probability <= 0.0484^8 < 3.1e-11.
// As in vmp_impute.hip the factorisation is that of A~ = M Lambda M + (I - M): its observed rows and columns are those of the
// identity, so R~^-T applied to eps with eps_o = 0 is R^-T eps_m in the missing slots and 0 in the observed ones.  What a missing
// slot of x holds never enters arithmetic.  Every log w = -inf: the missing entries are 0 and z = -1; a NaN in l_k (a NaN pack row, as
// the pack builders write it: log w included) makes every resp NaN: the missing entries are NaN and z = -1.  With nothing observed
// l_k = log w_k alone: a row whose log w is finite but whose mu, Lambda or nu is NaN is chosen with its weight and gives NaN entries
// with z = that k, the other components draw normally.
//
// Random stream: Philox4x32 at VMP_PHILOX_ROUNDS rounds (the generator of vmp_svae.hip, restated in vmp_philox.h because that file
// is not a header), key = seed, counter = (row low, row high, s, SAMPLE_TAG + b) with row = row0 + n the ABSOLUTE row index, s the draw and b
// the block; nothing else enters (not the grid, the wave, N or the outputs requested), so rows [a, b) drawn with row0 = a are rows
// a .. b of the whole call.  SAMPLE_TAG + b differs from the fourth counter word of the cell noise (0) and of the categorical draw of
// subsample_kernel (SUBSAMPLE_TAG).  A uniform is (top 24 bits of a word + 1/2) 2^-24; in fp32 that is rounded once (ties to even),
// so the values above 1/2 are multiples of 2^-24, and the one that would round to 1.0 (top 24 bits all set) is kept at 1 - 2^-24, the
// largest fp32 below 1: no uniform is 0 or 1.  A normal pair comes from one word as oracle/philox.py box_muller8: radius
// sqrt(-2 log((a + 1/2) 2^-20)) from the top 20 bits, angle b 2^-12 revolutions from the low 12, (cos, sin).
//   b = 0        word 0 -> u_z,  word 1 -> u_b  (words 2, 3 unused)
//   b = 1        word t -> (eps_2t, eps_2t+1) = r (cos, sin), t = 0 .. 3: eps_i belongs to coordinate i; observed coordinates discard theirs
//   b = 16 + t   attempt t of the gamma draw: word 0 -> n_t = r cos (the sine is unused),  word 1 -> u_t  (words 2, 3 unused)
//
// Lane map (vmp_impute.hip): lane l = (i16 = l & 15, kk = l >> 4); a wave advances 4 rows per iteration over a contiguous range that
// depends on (N, blocks) only, and in the K-loop lane i16 owns component k = i16 + 16 t of the row n4 + kk.  l_k of a row is computed
// once and serves every draw; the cdf is an in-row prefix sum (four DPP row shifts per tile).  In the draw loop lane i16 owns draw
// s = s0 + i16 of its row: z is found for the 16 draws in turn (the draw's u_z is broadcast, the first k with cdf_k > u_z is a
// row16 reduction), then each lane evaluates the cell of ITS z again for R, y, q and xhat - only cdf_k is kept per component - and
// does the gamma draw and the R^-T solve on its own.  x == NULL (plain draws): the K-loop evaluates no cell, l_k = log w_k.
#include "vmp_impute_pack.h"
#include "vmp_philox.h"

using namespace vmp;

namespace {

constexpr int SMP_NW = 4;                 // waves per block
constexpr int SMP_MAX_BLOCKS = 2048;
constexpr int SMP_ROWS_PER_BLOCK = 64 * SMP_NW;
constexpr int SMP_ATTEMPTS = 8;           // T of the header comment
constexpr unsigned SAMPLE_TAG = 0x6d78a500u;
constexpr unsigned SMP_B_Z = 0u, SMP_B_EPS = 1u, SMP_B_GAMMA = 16u;

inline int sample_blocks(int64_t N) { return stream_blocks(N, SMP_ROWS_PER_BLOCK, SMP_MAX_BLOCKS); }

__device__ __forceinline__ void sample_philox(unsigned (&c)[4], unsigned long long row, unsigned s, unsigned b, unsigned long long seed) {
    c[0] = (unsigned)row; c[1] = (unsigned)(row >> 32); c[2] = s; c[3] = SAMPLE_TAG + b;
    philox_rounds(c, seed);
}
__device__ __forceinline__ float sample_uniform(unsigned w) { return philox_uniform24(w); }     // in (0, 1): never 1.0
__device__ __forceinline__ float sample_radius(unsigned w) {
    const float u1 = fmaf((float)(w >> 12), 9.5367431640625e-07f, 4.76837158203125e-07f);       // (a + 1/2) 2^-20, exact
    return sqrtf(-2.0f * logf(u1));
}
__device__ __forceinline__ float sample_angle(unsigned w) { return (float)(w & 0xFFFu) * 4.8828125e-04f; }   // in units of pi: b 2^-11, exact

struct SampleArgs {
    const float* x;           // (N,D) or NULL: every entry missing
    const uint8_t* mask;
    const float* pack;
    float* x_out;             // (draws, N, D)
    int* z_out;               // (draws, N) or NULL
    long long N;
    long long rpw;            // rows per wave (multiple of 4): wave g owns rows [g rpw, min(N, (g+1) rpw))
    long long row0;
    unsigned long long seed;
    int K, draws;
    int vec_in, vec_out;      // x / x_out 16-byte aligned
};

// One (row, component) cell, the operations of impute_cell (vmp_impute.hip) in its order: returns l_k; q, the conditional location
// xh[] (meaningful in the missing slots), the off-diagonal entries A[] of the Cholesky factor of A~ and its reciprocal diagonal rd[]
// are what a draw needs of the chosen component (the K-loop uses l_k alone; the rest is dead code there).
template <int D>
__device__ __forceinline__ float sample_cell(const ImputeParams<D>& p, const float (&x)[D], const bool (&miss)[D], int n_obs, float g,
                                             float& q_out, float (&xh)[D], float (&A)[ImputeGeo<D>::TRI], float (&rd)[D]) {
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
    float yy = 0.f;                              // y = R^-1 t (in v), |y|^2, R^-T y (in v)
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
    q_out = q;
    const float h = 0.5f * (p.nu + (float)n_obs);
    const float l = (p.lw + g) + (0.5f * p.ldet - slog) - h * log1p_f(q * p.inu);
    return n_obs == 0 ? p.lw : l;                // nothing observed: the weight alone
}

// inclusive prefix sum over the 16 lanes of a DPP row: v_i + v_{i-1}, then strides 2, 4, 8 (a lane without a source adds 0)
__device__ __forceinline__ float row16_prefix(float v) {
#define VMP_SHR_(n) __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x110 + (n), 0xf, 0xf, false))
    v += VMP_SHR_(1);
    v += VMP_SHR_(2);
    v += VMP_SHR_(4);
    v += VMP_SHR_(8);
#undef VMP_SHR_
    return v;
}

// g of the header comment for a = (nu + D_o) / 2 from the blocks b = 16 + t of (row, s); u_b is used when a < 1 only
__device__ __forceinline__ float sample_gamma(float a, float u_b, unsigned long long row, unsigned s, unsigned long long seed) {
    const bool small = a < 1.0f;
    const float ap = small ? a + 1.0f : a;
    const float d = ap - 0.333333343f;
    const float c = 1.0f / sqrtf(9.0f * d);
    float gam = d;
    bool done = false;
#pragma unroll 1
    for (int t = 0; t < SMP_ATTEMPTS; ++t) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        unsigned cw[4];
        sample_philox(cw, row, s, SMP_B_GAMMA + (unsigned)t, seed);
        const float n = sample_radius(cw[0]) * cospif(sample_angle(cw[0]));
        const float lu = logf(sample_uniform(cw[1]));
        const float w = fmaf(c, n, 1.0f);
        const float v = w * w * w;
        const float rhs = fmaf(d, logf(v), fmaf(-d, v, fmaf(0.5f * n, n, d)));
        const bool ok = w > 0.f && lu < rhs;
        gam = (!done && ok) ? d * v : gam;
        done = done || ok;
    }
    float g = 2.0f * gam;
    if (small) g *= expf(logf(u_b) / a);
    return g < 1.17549435e-38f ? 1.17549435e-38f : g;        // a NaN stays a NaN
}

// The packs are staged in LDS once per block.  KTMAX = 1: K <= 16;  KTMAX = 4: the lane walks ceil(K / 16) tiles.
template <int D, int KTMAX>
__global__ __launch_bounds__(SMP_NW * WAVE) void sample_kernel(SampleArgs a) {
    using G = ImputeGeo<D>;
    __shared__ float lds[KTMAX * 16 * G::STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, kk = lane >> 4;
    const int KT = KTMAX == 1 ? 1 : (a.K + 15) / 16;
    const bool cond = a.x != nullptr;                                       // the same in every lane

    for (int i = threadIdx.x; i < a.K * G::PACK; i += SMP_NW * WAVE) lds[(i / G::PACK) * G::STRIDE + i % G::PACK] = a.pack[i];
    __syncthreads();

    const long long gw = (long long)blockIdx.x * SMP_NW + wave;
    const long long r0 = gw * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    for (long long n4 = r0; n4 < r1; n4 += 4) {
        const long long n = n4 + kk;
        const bool valid = n < r1;
        const long long nr = valid ? n : r1 - 1;                         // rows past the range: a row of the range, discarded
        float x[D];
        bool miss[D];
        int n_obs = 0;
        if (cond) {
            load_row<D>(a.x + nr * D, x, a.vec_in != 0);
#pragma unroll
            for (int d = 0; d < D; ++d) { miss[d] = a.mask[nr * D + d] != 0; n_obs += miss[d] ? 0 : 1; }
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) { x[d] = 0.f; miss[d] = true; }
        }

        // l_k of the lane's components, the row's maximum and sum: the operations of impute_kernel, so that resp has its bits
        float ml = -INFINITY, sm = 0.f, lt[KTMAX];
#pragma unroll
        for (int j = 0; j < KTMAX; ++j) lt[j] = -INFINITY;
#pragma unroll 1
        for (int t = 0; t < KT; ++t) {
            const int k = t * 16 + i16;
            const float* row = lds + (k < a.K ? k : 0) * G::STRIDE;
            float l = row[G::LW];
            if (cond) {
                ImputeParams<D> p;
                p.load(row);
                float q, xh[D], A[G::TRI], rd[D];
                l = sample_cell<D>(p, x, miss, n_obs, row[G::G + n_obs], q, xh, A, rd);
            }
            l = k < a.K ? l : -INFINITY;
#pragma unroll
            for (int j = 0; j < KTMAX; ++j) lt[j] = t == j ? l : lt[j];
            const float mn = fmaxf(ml, l);
            const float sh = mn == -INFINITY ? 0.f : mn;                 // every term so far -inf: -inf - (-inf) would be NaN
            sm = fmaf(sm, __expf(ml - sh), __expf(l - sh));
            ml = mn;
        }
        const float mx = row16_max(ml);
        const float shift = mx == -INFINITY ? 0.f : mx;
        const float S = row16_sum(sm * __expf(ml - shift));
        const float inv = S == 0.f ? 0.f : 1.0f / S;                     // a row without mass: resp = 0
        const bool bad = inv != inv;                                     // a NaN term: every resp is NaN

        // cdf_k of the lane's components (lt[] becomes cdf[]) and the last k with resp_k > 0
        float base = 0.f, klast = -1.f;
#pragma unroll
        for (int j = 0; j < KTMAX; ++j) {
            const float r = __expf(lt[j] - shift) * inv;                 // components beyond K: exp(-inf) = 0
            klast = r > 0.f ? (float)(j * 16 + i16) : klast;
            lt[j] = base + row16_prefix(r);
            if constexpr (KTMAX > 1) base += row16_sum(r);
        }
        const int zlast = (int)row16_max(klast);

        const unsigned long long rowid = (unsigned long long)(a.row0 + nr);
#pragma unroll 1
        for (int s0 = 0; s0 < a.draws; s0 += 16) {
            const int s = s0 + i16;
            unsigned cw[4];
            sample_philox(cw, rowid, (unsigned)s, SMP_B_Z, a.seed);
            const float u_z = sample_uniform(cw[0]), u_b = sample_uniform(cw[1]);
            int z = zlast;
            const int ns = a.draws - s0 < 16 ? a.draws - s0 : 16;
#pragma unroll 1
            for (int sl = 0; sl < ns; ++sl) {
                const float u = __shfl(u_z, (lane & 48) | sl);
                float first = -128.f;                                    // minus the first k of the lane with cdf_k > u
#pragma unroll
                for (int j = KTMAX - 1; j >= 0; --j) first = (lt[j] > u && j * 16 + i16 < a.K) ? -(float)(j * 16 + i16) : first;
                first = row16_max(first);
                if (sl == i16 && first > -100.f) z = (int)(-first);
            }
            if (valid && s < a.draws) {
                float o[D];
                if (z < 0) {
#pragma unroll
                    for (int d = 0; d < D; ++d) o[d] = miss[d] ? (bad ? __builtin_nanf("") : 0.f) : x[d];
                } else {
                    const float* row = lds + z * G::STRIDE;
                    ImputeParams<D> p;
                    p.load(row);
                    float q, xh[D], A[G::TRI], rd[D], w[D];
                    sample_cell<D>(p, x, miss, n_obs, 0.f, q, xh, A, rd);
                    const float g = sample_gamma(0.5f * (p.nu + (float)n_obs), u_b, rowid, (unsigned)s, a.seed);
                    const float scale = sqrtf((p.nu + q) / g);
                    sample_philox(cw, rowid, (unsigned)s, SMP_B_EPS, a.seed);
#pragma unroll
                    for (int t = 0; t < (D + 1) / 2; ++t) {
                        const float rad = sample_radius(cw[t]), ang = sample_angle(cw[t]);
                        w[2 * t] = miss[2 * t] ? rad * cospif(ang) : 0.f;
                        if (2 * t + 1 < D) w[2 * t + 1] = miss[2 * t + 1] ? rad * sinpif(ang) : 0.f;
                    }
#pragma unroll
                    for (int i = D - 1; i >= 0; --i) {                       // R~^-T eps
                        float sacc = w[i];
#pragma unroll
                        for (int jq = i + 1; jq < D; ++jq) sacc = fmaf(-A[jq * (jq + 1) / 2 + i], w[jq], sacc);
                        w[i] = sacc * rd[i];
                    }
#pragma unroll
                    for (int d = 0; d < D; ++d) o[d] = miss[d] ? fmaf(scale, w[d], xh[d]) : x[d];
                }
                const long long at = (long long)s * a.N + n;
                store_row<D>(a.x_out + at * D, o, a.vec_out != 0);
                if (a.z_out) a.z_out[at] = z;
            }
        }
    }
}

template <int D>
int launch_sample(const SampleArgs& a, int blocks, hipStream_t s) {
    const dim3 grid(blocks), block(SMP_NW * WAVE);
    if (a.K <= 16) hipLaunchKernelGGL((sample_kernel<D, 1>), grid, block, 0, s, a);
    else           hipLaunchKernelGGL((sample_kernel<D, 4>), grid, block, 0, s, a);
    return check_launch("sample_kernel");
}

}  // namespace

extern "C" {

int vmp_mixture_sample(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* impute_pack, uint64_t seed,
                       int64_t row0, int draws, float* x_out, int32_t* z_out, void* stream) {
    int rc = stream_dims("vmp_mixture_sample", D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("vmp_mixture_sample: N must be positive (got %lld)", (long long)N); return VMP_E_BADARG; }
    if (draws <= 0) { set_error("vmp_mixture_sample: draws must be positive (got %d)", draws); return VMP_E_BADARG; }
    if (row0 < 0) { set_error("vmp_mixture_sample: row0 must not be negative (got %lld)", (long long)row0); return VMP_E_BADARG; }
    if ((x == nullptr) != (mask == nullptr)) {
        set_error("vmp_mixture_sample: x and mask are given together or both NULL (%s is NULL)", !x ? "x" : "mask");
        return VMP_E_BADARG;
    }
    if (!impute_pack || !x_out) { set_error("vmp_mixture_sample: null pointer (%s)", !impute_pack ? "pack" : "x_out"); return VMP_E_BADARG; }
    const int blocks = sample_blocks(N);
    SampleArgs a{};
    a.x = x; a.mask = mask; a.pack = impute_pack; a.x_out = x_out; a.z_out = z_out;
    a.N = N; a.row0 = row0; a.seed = seed; a.K = K; a.draws = draws;
    a.rpw = rows_per_wave(N, (long long)blocks * SMP_NW, 4);
    a.vec_in = aligned16(x); a.vec_out = aligned16(x_out);
    rc = -1;
    VMP_SWITCH_DIM(D, DD, rc = launch_sample<DD>(a, blocks, static_cast<hipStream_t>(stream)));
    return rc;
}

}  // extern "C"
