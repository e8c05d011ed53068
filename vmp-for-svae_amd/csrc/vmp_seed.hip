// Mixture initialisation: seeded k-means++ centres (D^2-seeding, Arthur & Vassilvitskii 2007) and the responsibilities of the nearest
// centre, on fully or partly observed rows, with no atomics and no host work between launches (include/vmp_hip.h "Mixture
// initialisation").
//
// Per row n: o(n) its observed coordinates, D_o(n) their number, x~_n the row with `fill` in its missing slots,
//   dist2(n, c) = (D / D_o(n)) sum_{i in o(n)} (x_ni - c_i)^2   (0 when D_o(n) = 0: the partial-distance rule).
// Rounds j = 0 .. K-1, with w_n = [D_o(n) > 0] before round 0:
//   E_nj = -log u(seed, n, j);  s_n = E_nj / w_n (+inf where w_n = 0);  i_j = the row with the smallest (s_n, n), lexicographically;
//   c_j = x~_{i_j};  w_n <- dist2(n, c_0) after round 0,  min(w_n, dist2(n, c_j)) after a later round.
// The smallest of independent exponentials of rates w_n falls on row n with probability w_n / sum w: exact D^2-sampling, and a
// minimum of (s, n) does not depend on how the rows are spread over lanes, waves and blocks.  u is word 0 of the Philox block
// (vmp_philox.h) with counter (n low, n high, j, SEED_TAG), as a 24-bit uniform in (0, 1).
//
// Launches: K + 1 of seed_round_kernel for the centres, 1 of seed_assign_kernel for the responsibilities.  Launch j = 0 .. K
//   prologue (j > 0): every block reduces the per-block candidates (s, n) that launch j - 1 left in the workspace to i_{j-1} - the
//                     same fixed-order reduction in every block - and reads c_{j-1} = x~ of that row; block 0 writes it out;
//   body (j < K, or j = K with mind2_out): one row per lane: w of the row is updated with c_{j-1} (kept in the workspace; launch K
//                     writes it to mind2_out) and, for j < K, s_n enters the lane's, then the wave's, then the block's minimum, which
//                     goes to the candidate slot of the block.  The slots are double-buffered by the parity of j.
// Launch K without mind2_out is one block that runs the prologue alone.  Per row a round reads x, the mask and w and writes w.
#include "vmp_mix_stream.h"
#include "vmp_philox.h"

using namespace vmp;

namespace {

constexpr int SEED_NW = 4;                       // waves per block
constexpr int SEED_ROWS_PER_BLOCK = 1024;        // a wave walks at least four 64-row groups before a block is added
constexpr int SEED_MAX_BLOCKS = 1024;
constexpr unsigned SEED_TAG = 0x6b6d2b00u;       // no other fourth counter word of csrc/ equals it (vmp_philox.h lists them)
constexpr long long NO_ROW = 0x7fffffffffffffffLL;

inline int seed_blocks(int64_t N) { return stream_blocks(N, SEED_ROWS_PER_BLOCK, SEED_MAX_BLOCKS); }

// workspace: [ w (N) fp32, padded to 16 bytes | candidate rows (2, blocks) int64 | candidate values (2, blocks) fp32 ]
inline size_t seed_w_bytes(int64_t N) { return ((size_t)N * sizeof(float) + 15) / 16 * 16; }
inline size_t seed_ws_bytes(int64_t N) {
    return seed_w_bytes(N) + ((size_t)2 * seed_blocks(N) * (sizeof(long long) + sizeof(float)) + 15) / 16 * 16;
}

struct SeedArgs {
    const float* x;
    const uint8_t* mask;      // or NULL: every entry observed
    const float* fill;
    float* w;                 // (N) in the workspace
    float* w_dst;             // where this launch writes w: the workspace, or mind2_out in launch K
    long long* cand_n;        // (2, nblk)
    float* cand_s;            // (2, nblk)
    float* centers;           // (K,D)
    long long* index;         // (K) or NULL
    long long N;
    long long rpw;            // rows per wave (multiple of 64): wave g owns rows [g rpw, min(N, (g+1) rpw))
    unsigned long long seed;
    int round, K, nblk;
    int rows;                 // 0: prologue only
    int vec, mvec;            // x 16-byte aligned / the mask 4-byte aligned
};

// (bs, bn) <- the lexicographic minimum of (bs, bn) and (s, n)
__device__ __forceinline__ void take_min(float& bs, long long& bn, float s, long long n) {
    const bool lt = s < bs || (s == bs && n < bn);
    bs = lt ? s : bs;
    bn = lt ? n : bn;
}

// the minimum over the block in every thread; called by every thread of the block
__device__ __forceinline__ void block_min(float& bs, long long& bn, int lane, int wave) {
    __shared__ float ls[SEED_NW];
    __shared__ long long ln[SEED_NW];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) take_min(bs, bn, __shfl_xor(bs, m), __shfl_xor(bn, m));
    __syncthreads();                             // the previous call's readers are done with ls / ln
    if (lane == 0) { ls[wave] = bs; ln[wave] = bn; }
    __syncthreads();
    bs = ls[0]; bn = ln[0];
#pragma unroll
    for (int j = 1; j < SEED_NW; ++j) take_min(bs, bn, ls[j], ln[j]);
}

// the row's missing flags and D_o; mvec (the mask is 4-byte aligned and D a multiple of 4): whole words instead of bytes
template <int D>
__device__ __forceinline__ int load_mask(const uint8_t* mask, long long n, bool mvec, bool (&miss)[D]) {
    int n_obs = D;
#pragma unroll
    for (int d = 0; d < D; ++d) miss[d] = false;
    if (mask) {
        n_obs = 0;
        if (D % 4 == 0 && mvec) {
#pragma unroll
            for (int q = 0; q < D / 4; ++q) {
                const unsigned m4 = reinterpret_cast<const unsigned*>(mask + n * D)[q];
#pragma unroll
                for (int b = 0; b < 4; ++b) miss[4 * q + b] = ((m4 >> (8 * b)) & 0xffu) != 0;
            }
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) miss[d] = mask[n * D + d] != 0;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) n_obs += miss[d] ? 0 : 1;
    }
    return n_obs;
}

// dist2 of the header comment; what a missing slot of x holds is selected away, never computed with
template <int D>
__device__ __forceinline__ float dist2(const float (&x)[D], const bool (&miss)[D], int n_obs, const float* c) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float t = miss[d] ? 0.f : x[d] - c[d];
        s = fmaf(t, t, s);
    }
    return n_obs == 0 ? 0.f : s * ((float)D / (float)n_obs);
}

template <int D>
__global__ __launch_bounds__(SEED_NW * WAVE) void seed_round_kernel(SeedArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = a.round;
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = 0.f;

    if (j > 0) {                                 // the pick of round j - 1
        const float* cs = a.cand_s + (size_t)((j - 1) & 1) * a.nblk;
        const long long* cn = a.cand_n + (size_t)((j - 1) & 1) * a.nblk;
        float bs = INFINITY;
        long long bn = NO_ROW;
        for (int i = threadIdx.x; i < a.nblk; i += SEED_NW * WAVE) take_min(bs, bn, cs[i], cn[i]);
        block_min(bs, bn, lane, wave);
        const long long pick = (bn >= 0 && bn < a.N) ? bn : 0;           // block 0 always holds a row: never taken
#pragma unroll
        for (int d = 0; d < D; ++d) c[d] = (a.mask && a.mask[pick * D + d] != 0) ? a.fill[d] : a.x[pick * D + d];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) a.centers[(size_t)(j - 1) * D + d] = c[d];
            if (a.index) a.index[j - 1] = pick;
        }
    }
    if (!a.rows) return;

    const long long gw = (long long)blockIdx.x * SEED_NW + wave;
    const long long r0 = gw * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    float bs = INFINITY;
    long long bn = NO_ROW;
    for (long long n0 = r0; n0 < r1; n0 += WAVE) {
        const long long n = n0 + lane;
        const bool valid = n < r1;
        const long long nr = valid ? n : r1 - 1;                          // lanes past the range: a row of the range, discarded
        float x[D];
        bool miss[D];
        load_row<D>(a.x + nr * D, x, a.vec != 0);
        const int n_obs = load_mask<D>(a.mask, nr, a.mvec != 0, miss);
        float w;
        if (j == 0) {
            w = n_obs > 0 ? 1.f : 0.f;
        } else {
            const float d2 = dist2<D>(x, miss, n_obs, c);
            w = j == 1 ? d2 : fminf(a.w[nr], d2);
        }
        if (valid) a.w_dst[n] = w;
        if (j < a.K && valid) {
            unsigned cw[4] = {(unsigned)n, (unsigned)((unsigned long long)n >> 32), (unsigned)j, SEED_TAG};
            philox_rounds(cw, a.seed);
            const float e = -logf(philox_uniform24(cw[0]));
            take_min(bs, bn, w > 0.f ? e / w : INFINITY, n);
        }
    }
    if (j < a.K) {
        block_min(bs, bn, lane, wave);
        if (threadIdx.x == 0) {
            a.cand_s[(size_t)(j & 1) * a.nblk + blockIdx.x] = bs;
            a.cand_n[(size_t)(j & 1) * a.nblk + blockIdx.x] = bn;
        }
    }
}

struct AssignArgs {
    const float* x;
    const uint8_t* mask;
    const float* centers;     // (K,D)
    float* r;                 // (N,K)
    int* z;                   // (N) or NULL
    long long N;
    long long rpw;
    float smooth;
    int K;
    int vec, mvec;            // x 16-byte aligned / the mask 4-byte aligned
};

// One row per lane for the distances; the (64, K) block of r that a wave's 64 rows own is contiguous and is written by the wave
// together, lane l the elements l, l + 64, ...: whole 256-byte stores whatever K is.
template <int D>
__global__ __launch_bounds__(SEED_NW * WAVE) void seed_assign_kernel(AssignArgs a) {
    __shared__ float cen[VMP_MAX_K * D];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = a.K;
    for (int i = threadIdx.x; i < K * D; i += SEED_NW * WAVE) cen[i] = a.centers[i];
    __syncthreads();
    const float lo = a.smooth / (float)K;
    const float hi = (1.0f - a.smooth) + lo;
    const float uni = 1.0f / (float)K;

    const long long gw = (long long)blockIdx.x * SEED_NW + wave;
    const long long r0 = gw * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    for (long long n0 = r0; n0 < r1; n0 += WAVE) {
        const long long n = n0 + lane;
        const bool valid = n < r1;
        const long long nr = valid ? n : r1 - 1;
        float x[D];
        bool miss[D];
        load_row<D>(a.x + nr * D, x, a.vec != 0);
        const int n_obs = load_mask<D>(a.mask, nr, a.mvec != 0, miss);
        float best = INFINITY;
        int z = 0;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float d2 = dist2<D>(x, miss, n_obs, cen + k * D);
            z = d2 < best ? k : z;                                       // ties: the lowest k
            best = d2 < best ? d2 : best;
        }
        z = n_obs == 0 ? -1 : z;
        if (valid && a.z) a.z[n] = z;
        const int cnt = (int)(r1 - n0 < WAVE ? r1 - n0 : WAVE) * K;      // elements of r the group owns
        float* rg = a.r + n0 * K;
#pragma unroll 1
        for (int t = 0; t < K; ++t) {
            const int e = t * WAVE + lane;
            const int row = e / K, k = e - row * K;                      // row < 64
            const int zr = __shfl(z, row);
            if (e < cnt) rg[e] = zr < 0 ? uni : (k == zr ? hi : lo);
        }
    }
}

template <int D>
int launch_rounds(SeedArgs a, float* mind2_out, int blocks, hipStream_t s) {
    for (int j = 0; j <= a.K; ++j) {
        a.round = j;
        a.rows = j < a.K || mind2_out != nullptr;
        a.w_dst = j == a.K ? mind2_out : a.w;
        hipLaunchKernelGGL((seed_round_kernel<D>), dim3(a.rows ? blocks : 1), dim3(SEED_NW * WAVE), 0, s, a);
        if (const int rc = check_launch("seed_round_kernel")) return rc;
    }
    return 0;
}

template <int D>
int launch_assign(const AssignArgs& a, int blocks, hipStream_t s) {
    hipLaunchKernelGGL((seed_assign_kernel<D>), dim3(blocks), dim3(SEED_NW * WAVE), 0, s, a);
    return check_launch("seed_assign_kernel");
}

}  // namespace

extern "C" {

size_t vmp_mixture_seed_workspace_bytes(int64_t N, int D, int K) {
    (void)D; (void)K;
    return N < 1 ? 0 : seed_ws_bytes(N);
}

int vmp_mixture_seed_centers(const float* x, const uint8_t* mask, const float* fill, int64_t N, int D, int K, uint64_t seed,
                             float* centers_out, int64_t* index_out, float* mind2_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "vmp_mixture_seed_centers";
    int rc = stream_dims(who, D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !centers_out) { set_error("%s: null pointer (%s)", who, !x ? "x" : "centers_out"); return VMP_E_BADARG; }
    if ((mask == nullptr) != (fill == nullptr)) {
        set_error("%s: mask and fill are given together or both NULL (%s is NULL)", who, !mask ? "mask" : "fill");
        return VMP_E_BADARG;
    }
    if ((rc = workspace_check(who, ws, ws_bytes, seed_ws_bytes(N)))) return rc;
    const int blocks = seed_blocks(N);
    SeedArgs a{};
    a.x = x; a.mask = mask; a.fill = fill;
    a.w = static_cast<float*>(ws);
    a.cand_n = reinterpret_cast<long long*>(static_cast<char*>(ws) + seed_w_bytes(N));
    a.cand_s = reinterpret_cast<float*>(a.cand_n + (size_t)2 * blocks);
    a.centers = centers_out;
    a.index = reinterpret_cast<long long*>(index_out);
    a.N = N; a.seed = seed; a.K = K; a.nblk = blocks;
    a.rpw = rows_per_wave(N, (long long)blocks * SEED_NW, WAVE);
    a.vec = aligned16(x); a.mvec = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    rc = -1;
    VMP_SWITCH_DIM(D, DD, rc = launch_rounds<DD>(a, mind2_out, blocks, static_cast<hipStream_t>(stream)));
    return rc;
}

int vmp_mixture_seed_assign(const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* centers, float smooth,
                            float* r_out, int32_t* z_out, void* stream) {
    const char* who = "vmp_mixture_seed_assign";
    int rc = stream_dims(who, D, K);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !centers || !r_out) {
        set_error("%s: null pointer (%s)", who, !x ? "x" : (!centers ? "centers" : "r_out"));
        return VMP_E_BADARG;
    }
    if (!(smooth >= 0.f && smooth < 1.f)) { set_error("%s: smooth must be in [0, 1) (got %g)", who, (double)smooth); return VMP_E_BADARG; }
    const int blocks = seed_blocks(N);
    AssignArgs a{};
    a.x = x; a.mask = mask; a.centers = centers; a.r = r_out; a.z = z_out;
    a.N = N; a.smooth = smooth; a.K = K;
    a.rpw = rows_per_wave(N, (long long)blocks * SEED_NW, WAVE);
    a.vec = aligned16(x); a.mvec = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    rc = -1;
    VMP_SWITCH_DIM(D, DD, rc = launch_assign<DD>(a, blocks, static_cast<hipStream_t>(stream)));
    return rc;
}

}  // extern "C"
