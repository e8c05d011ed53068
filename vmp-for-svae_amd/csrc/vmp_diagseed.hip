// Diagonal-covariance mixture: seeded k-means++ centres and the responsibilities of the nearest centre for complete rows of up to
// VMP_DIAG_MAX_D = 64 columns (include/vmp_hip.h "Diagonal-covariance mixture: seeded start on wide rows").  The mathematics is that
// of "Mixture initialisation" (vmp_seed.hip) without a mask:
//   dist2(n, c) = sum_d (x_nd - c_d)^2, fp32, on the difference, in d order, one fma per coordinate;
//   rounds j = 0 .. K-1, w_n = 1 before round 0:  E_nj = -log u(seed, n, j);  s_n = E_nj / w_n (+inf where w_n = 0);
//   i_j = the row with the smallest (s_n, n), lexicographically;  c_j = x_{i_j};  w_n <- dist2(n, c_0), then min(w_n, dist2(n, c_j)).
// u is word 0 of the Philox block (vmp_philox.h) with counter (n low, n high, j, 0x6b6d2b00) - the stream of vmp_seed.hip, and for
// D <= 8 the arithmetic of its dist2 as well, so both files pick the same rows there.
//
// A row is up to 256 bytes, so a lane does not load its own row: the kernels use the row tile of vmp_diag_stream.h - 4 waves per
// block, wave g owns the rows [g rpw, (g+1) rpw) and walks them in tiles of 64; a tile is copied to the wave's own LDS with coalesced
// dword loads (any alignment of x) and read back with lane = row at an odd row stride.  The centre is wave-uniform: it is read from
// x itself through the constant address space (scalar loads), as diag_pass_kernel reads its pack.
//
// Launches: K + 1 of dseed_round_kernel for the centres, 1 of dseed_assign_kernel.  Launch j = 0 .. K
//   prologue (j > 0): every block reduces the per-block candidates (s, n) of launch j - 1 to i_{j-1} - the same fixed-order reduction
//                     in every block, no atomics; block 0 writes c_{j-1} and i_{j-1} out;
//   body:             launch 0 reads no x (w = 1); launch j > 0 streams the rows once, w <- min(w, dist2(., c_{j-1})) (in the
//                     workspace; launch K writes it to mind2_out) and, for j < K, s_n enters the lane's, the wave's, then the block's
//                     minimum, which goes to the block's candidate slot (double-buffered by the parity of j).
// Launch K without mind2_out is one block that runs the prologue alone.  The geometry depends on (N, D) only.
#include "vmp_diag_stream.h"
#include "vmp_philox.h"

using namespace vmp;

namespace {

constexpr int DSD_ROWS_PER_BLOCK = 1024;         // four tiles per wave before a block is added
constexpr int DSD_FENCE = 16;                    // coordinates between two scheduling fences: bounds the centre words in SGPRs at once
constexpr int DSD_BATCH = 32;                    // dword loads of a lane in flight while a tile is staged
constexpr unsigned DSD_TAG = 0x6b6d2b00u;        // the fourth counter word of the exponential race (vmp_philox.h)
constexpr long long DSD_NO_ROW = 0x7fffffffffffffffLL;

// the tile of a block is 4 x 64 x (D | 1) words: above D = 32 two blocks fit a CU's LDS, so one resident set is 512 blocks
inline int dseed_max_blocks(int D) { return D > 32 ? 512 : 1024; }
inline int dseed_blocks(int64_t N, int D) { return stream_blocks(N, DSD_ROWS_PER_BLOCK, dseed_max_blocks(D)); }

// workspace: [ w (N) fp32, padded to 16 bytes | candidate rows (2, blocks) int64 | candidate values (2, blocks) fp32 ]
inline size_t dseed_w_bytes(int64_t N) { return ((size_t)N * sizeof(float) + 15) / 16 * 16; }
inline size_t dseed_ws_bytes(int64_t N, int D) {
    return dseed_w_bytes(N) + ((size_t)2 * dseed_blocks(N, D) * (sizeof(long long) + sizeof(float)) + 15) / 16 * 16;
}
inline size_t dseed_round_lds(int D) { return (size_t)DIAG_NW * DIAG_TILE * (D | 1) * sizeof(float); }
inline size_t dseed_assign_lds(int D, int K) { return (size_t)DIAG_NW * DIAG_TILE * ((D > K ? D : K) | 1) * sizeof(float); }

struct DSeedArgs {
    const float* x;
    float* w;                 // (N) in the workspace
    float* w_dst;             // where this launch writes w: the workspace, or mind2_out in launch K
    long long* cand_n;        // (2, nblk)
    float* cand_s;            // (2, nblk)
    float* centers;           // (K,D)
    long long* index;         // (K) or NULL
    long long N;
    long long rpw;            // rows per wave, a multiple of 64
    unsigned long long seed;
    int round, K, nblk;
    int rows;                 // 0: prologue only
};

// (bs, bn) <- the lexicographic minimum of (bs, bn) and (s, n)
__device__ __forceinline__ void take_min(float& bs, long long& bn, float s, long long n) {
    const bool lt = s < bs || (s == bs && n < bn);
    bs = lt ? s : bs;
    bn = lt ? n : bn;
}

// the minimum over the block in every thread; called by every thread of the block
__device__ __forceinline__ void block_min(float& bs, long long& bn, int lane, int wave) {
    __shared__ float ls[DIAG_NW];
    __shared__ long long ln[DIAG_NW];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) take_min(bs, bn, __shfl_xor(bs, m), __shfl_xor(bn, m));
    __syncthreads();                             // the previous call's readers are done with ls / ln
    if (lane == 0) { ls[wave] = bs; ln[wave] = bn; }
    __syncthreads();
    bs = ls[0]; bn = ln[0];
#pragma unroll
    for (int j = 1; j < DIAG_NW; ++j) take_min(bs, bn, ls[j], ln[j]);
}

// tile_stage of vmp_diag_stream.h for float with the width a template argument and the loads issued DSD_BATCH at a time ahead of
// their LDS stores: `total` contiguous words of src -> the LDS tile of 64 rows x D with row stride D | 1, the rest zeros.  These
// kernels do a subtraction and an fma per word; with one load in flight per wave (the rolled loop of tile_stage) they would wait
// for memory latency, not bandwidth.  A lane past `total` loads the last word again (no branch around a load) and stores a zero.
template <int D>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, float* dst, int total, int lane) {
    constexpr int XS = D | 1;
    int row = lane / D, col = lane % D;
#pragma unroll
    for (int b = 0; b < D; b += DSD_BATCH) {
        float v[DSD_BATCH];
#pragma unroll
        for (int u = 0; u < DSD_BATCH; ++u) {
            const int i = (b + u) * WAVE + lane;
            if (b + u < D) v[u] = src[i < total ? i : total - 1];
        }
#pragma unroll
        for (int u = 0; u < DSD_BATCH; ++u) {
            const int i = (b + u) * WAVE + lane;
            if (b + u < D) {
                dst[row * XS + col] = i < total ? v[u] : 0.f;
                col += WAVE % D;
                row += WAVE / D;
                if (col >= D) { col -= D; ++row; }
            }
        }
    }
}

// dist2 of the lane's row of the tile to the wave-uniform centre c
template <int D>
__device__ __forceinline__ float tile_dist2(const float* row, cfloat* c) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (d && d % DSD_FENCE == 0) __builtin_amdgcn_sched_barrier(0);
        const float t = row[d] - c[d];
        s = fmaf(t, t, s);
    }
    return s;
}

template <int D>
__global__ __launch_bounds__(DIAG_NW * WAVE) void dseed_round_kernel(DSeedArgs a) {
    extern __shared__ float dsd_lds[];
    constexpr int XS = D | 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = a.round;
    float* xs = dsd_lds + wave * DIAG_TILE * XS;
    long long pick = 0;

    if (j > 0) {                                 // the pick of round j - 1
        const float* cs = a.cand_s + (size_t)((j - 1) & 1) * a.nblk;
        const long long* cn = a.cand_n + (size_t)((j - 1) & 1) * a.nblk;
        float bs = INFINITY;
        long long bn = DSD_NO_ROW;
        for (int i = threadIdx.x; i < a.nblk; i += DIAG_NW * WAVE) take_min(bs, bn, cs[i], cn[i]);
        block_min(bs, bn, lane, wave);
        bn = (bn >= 0 && bn < a.N) ? bn : 0;                                // block 0 always holds a row: never taken
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)bn);   // the same in every thread; now in SGPRs
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)bn >> 32));
        pick = (long long)(((unsigned long long)hi << 32) | lo);
        if (blockIdx.x == 0) {
            if (threadIdx.x < D) a.centers[(size_t)(j - 1) * D + threadIdx.x] = a.x[pick * D + threadIdx.x];
            if (threadIdx.x == 0 && a.index) a.index[j - 1] = pick;
        }
    }
    if (!a.rows) return;
    cfloat* c = (cfloat*)(a.x + pick * D);       // c_{j-1}: the bits of x at the chosen row (launch 0 does not read it)

    const long long g = (long long)blockIdx.x * DIAG_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    float bs = INFINITY;
    long long bn = DSD_NO_ROW;
    for (long long t0 = r0; t0 < r1; t0 += DIAG_TILE) {
        const int rows = r1 - t0 < DIAG_TILE ? (int)(r1 - t0) : DIAG_TILE;
        const bool valid = lane < rows;
        const long long n = t0 + lane;
        float w = 1.f;
        if (j > 0) {
            stage_rows<D>(a.x + t0 * D, xs, rows * D, lane);
            __builtin_amdgcn_wave_barrier();
            const float d2 = tile_dist2<D>(xs + lane * XS, c);
            w = j == 1 ? d2 : fminf(a.w[valid ? n : r1 - 1], d2);           // lanes past the tile: a row of the range, discarded
            __builtin_amdgcn_wave_barrier();
        }
        if (valid) a.w_dst[n] = w;
        if (j < a.K && valid) {
            unsigned cw[4] = {(unsigned)n, (unsigned)((unsigned long long)n >> 32), (unsigned)j, DSD_TAG};
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

struct DAssignArgs {
    const float* x;
    float* r;                 // (N,K) or NULL
    int* z;                   // (N) or NULL
    long long N;
    long long rpw;
    float smooth;
    int K;
};

// The row sits in registers while the K centres go by as scalar operands; the tile's LDS then takes the (64, K) block of r, which is
// contiguous in r_out and leaves with coalesced stores.
template <int D>
__global__ __launch_bounds__(DIAG_NW * WAVE) void dseed_assign_kernel(DAssignArgs a, const float* __restrict__ centers) {
    extern __shared__ float dsd_lds[];
    constexpr int XS = D | 1;
    const int K = a.K, RS = K | 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* tile = dsd_lds + wave * DIAG_TILE * (XS > RS ? XS : RS);
    cfloat* cen = (cfloat*)centers;
    const float lo = a.smooth / (float)K;
    const float hi = (1.0f - a.smooth) + lo;

    const long long g = (long long)blockIdx.x * DIAG_NW + wave;
    const long long r0 = g * a.rpw;
    const long long r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    for (long long t0 = r0; t0 < r1; t0 += DIAG_TILE) {
        const int rows = r1 - t0 < DIAG_TILE ? (int)(r1 - t0) : DIAG_TILE;
        stage_rows<D>(a.x + t0 * D, tile, rows * D, lane);
        __builtin_amdgcn_wave_barrier();
        float x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = tile[lane * XS + d];
        float best = INFINITY;
        int z = 0;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float d2 = tile_dist2<D>(x, cen + k * D);
            z = d2 < best ? k : z;                                          // ties: the lowest k
            best = d2 < best ? d2 : best;
        }
        if (lane < rows && a.z) a.z[t0 + lane] = z;
        __builtin_amdgcn_wave_barrier();                                    // every lane has its row: the tile is free
        if (a.r) {
#pragma unroll 1
            for (int k = 0; k < K; ++k) tile[lane * RS + k] = k == z ? hi : lo;
            __builtin_amdgcn_wave_barrier();
            tile_store(a.r + t0 * K, tile, rows * K, K, RS, lane);
            __builtin_amdgcn_wave_barrier();
        }
    }
}

int launch_rounds(int D, DSeedArgs a, float* mind2_out, int blocks, hipStream_t s) {
    return dispatch_dim<VMP_DIAG_MAX_D>(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        const size_t lds = dseed_round_lds(DD);
        if (lds > 48 * 1024)
            if (const int rc = set_dyn_lds(reinterpret_cast<const void*>(dseed_round_kernel<DD>), lds, "dseed_round_kernel")) return rc;
        for (int j = 0; j <= a.K; ++j) {
            a.round = j;
            a.rows = j < a.K || mind2_out != nullptr;
            a.w_dst = j == a.K ? mind2_out : a.w;
            hipLaunchKernelGGL((dseed_round_kernel<DD>), dim3(a.rows ? blocks : 1), dim3(DIAG_NW * WAVE), lds, s, a);
            if (const int rc = check_launch("dseed_round_kernel")) return rc;
        }
        return 0;
    });
}

int launch_assign(int D, const DAssignArgs& a, const float* centers, int blocks, hipStream_t s) {
    return dispatch_dim<VMP_DIAG_MAX_D>(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        return launch_dyn_lds(dseed_assign_kernel<DD>, "dseed_assign_kernel", blocks, DIAG_NW * WAVE, dseed_assign_lds(DD, a.K), s, a, centers);
    });
}

}  // namespace

extern "C" {

size_t vmp_mixture_diag_seed_workspace_bytes(int64_t N, int D, int K) {
    if (N < 1 || D < 1 || D > VMP_DIAG_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    return dseed_ws_bytes(N, D);
}

int vmp_mixture_diag_seed_centers(const float* x, int64_t N, int D, int K, uint64_t seed, float* centers_out, int64_t* index_out,
                                  float* mind2_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "vmp_mixture_diag_seed_centers";
    int rc = stream_dims(who, D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !centers_out) { set_error("%s: null pointer (%s)", who, !x ? "x" : "centers_out"); return VMP_E_BADARG; }
    if ((rc = workspace_check(who, ws, ws_bytes, dseed_ws_bytes(N, D)))) return rc;
    const int blocks = dseed_blocks(N, D);
    DSeedArgs a{};
    a.x = x;
    a.w = static_cast<float*>(ws);
    a.cand_n = reinterpret_cast<long long*>(static_cast<char*>(ws) + dseed_w_bytes(N));
    a.cand_s = reinterpret_cast<float*>(a.cand_n + (size_t)2 * blocks);
    a.centers = centers_out;
    a.index = reinterpret_cast<long long*>(index_out);
    a.N = N; a.seed = seed; a.K = K; a.nblk = blocks;
    a.rpw = rows_per_wave(N, (long long)blocks * DIAG_NW, DIAG_TILE);
    return launch_rounds(D, a, mind2_out, blocks, static_cast<hipStream_t>(stream));
}

int vmp_mixture_diag_seed_assign(const float* x, int64_t N, int D, int K, const float* centers, float smooth, float* r_out,
                                 int32_t* z_out, void* stream) {
    const char* who = "vmp_mixture_diag_seed_assign";
    int rc = stream_dims(who, D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !centers) { set_error("%s: null pointer (%s)", who, !x ? "x" : "centers"); return VMP_E_BADARG; }
    if (!r_out && !z_out) { set_error("%s: no output requested (r_out and z_out are both NULL)", who); return VMP_E_BADARG; }
    if (!(smooth >= 0.f && smooth < 1.f)) { set_error("%s: smooth must be in [0, 1) (got %g)", who, (double)smooth); return VMP_E_BADARG; }
    const int blocks = dseed_blocks(N, D);
    DAssignArgs a{};
    a.x = x; a.r = r_out; a.z = z_out;
    a.N = N; a.smooth = smooth; a.K = K;
    a.rpw = rows_per_wave(N, (long long)blocks * DIAG_NW, DIAG_TILE);
    return launch_assign(D, a, centers, blocks, static_cast<hipStream_t>(stream));
}

}  // extern "C"
