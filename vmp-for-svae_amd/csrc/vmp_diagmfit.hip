// Diagonal-covariance Gaussian mixture fit on partly observed and weighted rows of up to VMP_DIAG_MAX_D = 64 columns (include/vmp_hip.h
// "Diagonal-covariance mixture: fitting partly observed and weighted rows").  Model, posterior and notation of vmp_diagfit.hip; o(n) /
// m(n) the observed / missing coordinates of row n, D_o(n) = |o(n)|, w_n >= 0 the row's weight (1 without weights), lbar_kd = a_k / b_kd:
//   hl_kd      = -1/2 log lbar_kd
//   log rho_nk = c_k - 1/2 sum_{d in o(n)} lbar_kd (x_nd - m_kd)^2 + sum_{d in m(n)} hl_kd,      r_nk = softmax_k log rho_nk
//   q(x_nd | z_n = k) for d missing: N(m_kd, 1 / lbar_kd)
//   Nk = sum_n w_n r_nk,   M_kd = sum_n w_n r_nk [d in m(n)]
//   sx_kd  = sum_n w_n r_nk [d in o(n)] x_nd   + M_kd m_kd
//   sxx_kd = sum_n w_n r_nk [d in o(n)] x_nd^2 + M_kd (m_kd^2 + 1 / lbar_kd)
//   data   = sum_n w_n ( logsumexp_k log rho_nk - 1/2 D_o(n) log 2 pi )
// The pack is [ m (D) | lbar (D) | hl (D) | c ] per component, fp32.  A weight does not enter a row's own responsibilities.
//
// The pass kernel has the geometry of diag_pass_kernel (vmp_diagfit.hip): 4 waves per block, wave g owns the rows [g rpw, (g+1) rpw)
// and walks them in tiles of 64 rows staged to its own LDS (vmp_diag_stream.h); E-part with lane = row, M-part as
// v_mfma_f32_16x16x4_f32 on y = x - pivot with ONE pivot, fp64 flush every 128 rows, a reducing launch that adds the waves in a fixed
// order.  What differs:
//   weights  the row's weight sits in the wave's LDS next to r; the M-part's A operand is w r, and a row of weight 0 (or past the end)
//            is removed by a select on both operands: whatever its x holds reaches neither the moments nor the data term.  r_out /
//            logr_out carry the unweighted r.  w == NULL is a wave-uniform test: every weight is 1.
//   MASKED   the tile of the mask (uint8) is staged like x.  The E-part holds the row's mask as 64 bits, selects t = miss ? 0 : x - m
//            and adds hl for a missing coordinate; the M-part's B operand is y = miss ? 0 : x - pivot, and a third MFMA chain with B =
//            the 0/1 indicator of a missing entry accumulates M_kd.  The slab of a wave is then K (1 + 3 D) fp64 words.  What a missing
//            slot of x holds never enters arithmetic.  Without MASKED nothing of a mask is read or selected.
//   pivot    the mean of the observed entries of up to 64 evenly strided rows of positive weight (0 for a column without one): a
//            function of (x, mask, w, N, D) alone that no NaN of a missing slot or of a row of weight 0 can reach.
//   fill     x_fill_out: the lane replaces the missing entries of its row by sum_k r_nk m_kd in the x tile (observed entries keep their
//            bits; the M-part never reads a missing entry) and the tile is stored with coalesced stores.
//   reduce   sx = s1 + (Nk - M) p + M m,   sxx = s2 + 2 p s1 + (Nk - M) p^2 + M (m^2 + 1 / lbar) in fp64 with the pack's fp32 m, lbar.
// A row's data term is formed in fp64 from the fp32 log-sum-exp, the integer D_o and the fp32 weight, and added in the fixed order of
// vmp_diagfit.hip.  No atomics; the geometry depends on (N, D, K) only: stats and data are bit-identical from run to run and for every
// set of optional outputs.
#include "vmp_diag_stream.h"

using namespace vmp;

namespace {

constexpr int DM_FLUSH_TILES = 2;             // tiles between two fp32 -> fp64 flushes: 128 rows of a wave
constexpr int DM_ROWS_PER_BLOCK = 2048;
constexpr int DM_RED_GROUPS = 16;             // wave groups of the reduction block
constexpr int DM_PIVOT_ROWS = 64;
constexpr double DM_LOG_2PI = 1.83787706640934548356;

// One geometry and one workspace for both forms: sized for the masked slab of K (1 + 3 D) fp64 words per wave.
inline int dm_max_blocks(int D, int K) { return K * (1 + 3 * D) <= 2048 ? 512 : 256; }
inline int dm_blocks(int64_t N, int D, int K) { return stream_blocks(N, DM_ROWS_PER_BLOCK, dm_max_blocks(D, K)); }
inline size_t dm_slab_bytes(int64_t N, int D, int K) { return (size_t)dm_blocks(N, D, K) * DIAG_NW * K * (1 + 3 * D) * sizeof(double); }
// pivot (64) | per wave: x tile, r tile, weights (64) and, masked, the mask tile (64 rows of D | 1 bytes)
inline size_t dm_lds_bytes(int D, int K, bool masked) {
    return (size_t)(64 + DIAG_NW * (DIAG_TILE * ((D | 1) + (K | 1)) + DIAG_TILE)) * sizeof(float) + (masked ? (size_t)DIAG_NW * DIAG_TILE * (D | 1) : 0);
}

struct DmfitArgs {
    const float* x;
    const uint8_t* mask;  // (N,D), nonzero = missing; NULL in the unmasked form
    const float* w;       // (N) or NULL: every weight 1
    float* r;             // (N,K) or NULL
    float* logr;          // (N,K) or NULL
    float* xfill;         // (N,D) or NULL (masked form only)
    double* slab;         // (waves, K, SW) fp64, SW = 1 + 2 D, masked 1 + 3 D
    double* partials;     // (blocks) fp64
    float* pivot;         // (64) fp32, written by block 0
    long long N;
    long long rpw;        // rows per wave, a multiple of 64
    int K;
};

template <int D, int KTMAX, bool MASKED>
__global__ __launch_bounds__(DIAG_NW * WAVE) void dmfit_cell_kernel(DmfitArgs a, const float* __restrict__ pack) {
    extern __shared__ float dm_lds[];
    __shared__ double wsum[DIAG_NW];
    constexpr int XS = D | 1, MS = D | 1, FT = (D + 15) / 16, PW = 3 * D + 1, SW = 1 + (MASKED ? 3 : 2) * D;
    constexpr int NCH = MASKED ? 3 : 2;
    const int K = a.K, RS = K | 1, KT = (K + 15) / 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15, j4 = lane >> 4;
    const int WF = DIAG_TILE * (XS + RS) + DIAG_TILE;                        // fp32 words of a wave's tiles
    float* pv = dm_lds;
    float* xs = dm_lds + 64 + wave * WF;
    float* rs = xs + DIAG_TILE * XS;
    float* wt = rs + DIAG_TILE * RS;
    uint8_t* ms = reinterpret_cast<uint8_t*>(dm_lds + 64 + DIAG_NW * WF) + wave * DIAG_TILE * MS;

    // the pivot: column means over the observed entries of up to 64 evenly strided rows of positive weight, added in row order
    if (threadIdx.x < D) {
        const long long cnt = a.N < DM_PIVOT_ROWS ? a.N : DM_PIVOT_ROWS, stride = a.N / cnt;
        float s = 0.f;
        int c = 0;
        for (long long j = 0; j < cnt; ++j) {
            const long long row = j * stride;
            bool use = a.w ? a.w[row] > 0.f : true;
            if constexpr (MASKED) use = use && a.mask[row * D + threadIdx.x] == 0;
            if (use) { s += a.x[row * D + threadIdx.x]; ++c; }
        }
        s = c ? s / (float)c : 0.f;
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
    double dsum = 0.0;                                                       // the lane's rows' weighted data terms, in row order

    f32x4 acc[NCH][KTMAX][FT];
    float nk[KTMAX];
#pragma unroll
    for (int kt = 0; kt < KTMAX; ++kt) {
        nk[kt] = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) acc[ch][kt][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    if (r0 >= r1)                                                            // a wave without rows: its moments are zero
        for (int i = lane; i < K * SW; i += WAVE) slab[i] = 0.0;

    int tile = 0;
    for (long long t0 = r0; t0 < r1; t0 += DIAG_TILE, ++tile) {
        const int rows = r1 - t0 < DIAG_TILE ? (int)(r1 - t0) : DIAG_TILE;
        tile_stage(a.x + t0 * D, xs, rows * D, D, XS, lane);
        if constexpr (MASKED) tile_stage(a.mask + t0 * D, ms, rows * D, D, MS, lane);
        const bool valid = lane < rows;
        const float wl = valid ? (a.w ? a.w[t0 + lane] : 1.0f) : 0.f;        // a row past the end: weight 0
        wt[lane] = wl;
        __builtin_amdgcn_wave_barrier();
        {
            float x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = xs[lane * XS + d];
            unsigned mlo = 0u, mhi = 0u;                                     // bit d: coordinate d of the lane's row is missing
            if constexpr (MASKED) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const unsigned bit = ms[lane * MS + d] != 0 ? 1u : 0u;
                    if (d < 32) mlo |= bit << (d & 31); else mhi |= bit << (d & 31);
                }
            }
            auto missing = [&](int d) -> bool { return MASKED && (((d < 32 ? mlo : mhi) >> (d & 31)) & 1u) != 0u; };
            float ml = -INFINITY;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                cfloat* p = cpack + k * PW;
                float q = 0.f, hs = 0.f;
                // the bit tests stay inside the loop: hoisted, their D results per lane cost more registers than the row itself
                if constexpr (MASKED) asm volatile("" : "+v"(mlo), "+v"(mhi));
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if constexpr (MASKED) {
                        const bool md = missing(d);
                        const float t = md ? 0.f : x[d] - p[d];
                        q = fmaf(t * p[D + d], t, q);
                        hs += md ? p[2 * D + d] : 0.f;
                    } else {
                        const float t = x[d] - p[d];
                        q = fmaf(t * p[D + d], t, q);
                    }
                }
                float l = fmaf(-0.5f, q, p[3 * D]);
                if constexpr (MASKED) l += hs;
                rs[lane * RS + k] = l;
                ml = fmaxf(ml, l);
            }
            const float shift = ml == -INFINITY ? 0.f : ml;                  // every term -inf: -inf - (-inf) would be NaN
            float s = 0.f;
#pragma unroll 1
            for (int k = 0; k < K; ++k) s += __expf(rs[lane * RS + k] - shift);
            const float inv = s == 0.f ? 0.f : 1.0f / s;                     // a row without mass: r = 0
            const float lse = shift + logf(s);
            const int dobs = D - (MASKED ? __popc(mlo) + __popc(mhi) : 0);
            if (wl > 0.f) dsum += (double)wl * ((double)lse - 0.5 * (double)dobs * DM_LOG_2PI);   // a select: weight 0 adds nothing
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float l = rs[lane * RS + k];
                if (a.logr && valid) a.logr[(t0 + lane) * K + k] = l - lse;
                rs[lane * RS + k] = valid ? __expf(l - shift) * inv : 0.f;
            }
            if constexpr (MASKED) {
                if (a.xfill) {                                               // wave-uniform: the last pass of an iteration call only
#pragma unroll
                    for (int d = 0; d < D; ++d) x[d] = missing(d) ? 0.f : x[d];
#pragma unroll 1
                    for (int k = 0; k < K; ++k) {
                        cfloat* p = cpack + k * PW;
                        const float rk = rs[lane * RS + k];
                        asm volatile("" : "+v"(mlo), "+v"(mhi));
#pragma unroll
                        for (int d = 0; d < D; ++d) x[d] = missing(d) ? fmaf(rk, p[d], x[d]) : x[d];
                    }
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        if (missing(d)) xs[lane * XS + d] = x[d];            // observed entries keep their bits
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (a.r) tile_store(a.r + t0 * K, rs, rows * K, K, RS, lane);        // the tile of r is contiguous in r_out
        if constexpr (MASKED) {
            if (a.xfill) tile_store(a.xfill + t0 * D, xs, rows * D, D, XS, lane);
        }
        // M-part: four rows per step, lane = (i16, j4): A = w r[row j4][component 16 kt + i16], B = y[row j4][column 16 ft + i16], y^2
        // and, masked, the indicator of a missing entry.  A row of weight 0 has A = 0 and B = 0 in every chain.  The y and y^2 chains run
        // over a 16-row group from zero and are added on the VALU, as in diag_pass_kernel; the chain of M_kd - a sum of non-negative
        // terms, nothing cancels - runs on its accumulator itself over the rows between two flushes: group sums of a third chain do
        // not fit the registers at K > 16 and D > 48 (profiles/NOTES_mix_diagmfit.md).
#pragma unroll 1
        for (int sg = 0; sg < DIAG_TILE / 16; ++sg) {
            float av[4][KTMAX];
            bool live[4];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int row = 16 * sg + 4 * st + j4;
                const float wr = wt[row];
                live[st] = wr > 0.f;
#pragma unroll
                for (int kt = 0; kt < KTMAX; ++kt) {
                    av[st][kt] = (live[st] && 16 * kt + i16 < K) ? rs[row * RS + 16 * kt + i16] * wr : 0.f;
                    nk[kt] += av[st][kt];
                }
            }
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                f32x4 gch[2][KTMAX];
#pragma unroll
                for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                    for (int kt = 0; kt < KTMAX; ++kt) gch[ch][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int row = 16 * sg + 4 * st + j4;
                    const bool col = 16 * ft + i16 < D;
                    bool obs = live[st] && col;
                    float mi = 0.f;
                    if constexpr (MASKED) {
                        const bool md = col && ms[row * MS + 16 * ft + i16] != 0;
                        mi = (live[st] && md) ? 1.0f : 0.f;
                        obs = obs && !md;
                    }
                    const float y = obs ? xs[row * XS + 16 * ft + i16] - pvr[ft] : 0.f;
                    const float y2 = y * y;
#pragma unroll
                    for (int kt = 0; kt < KTMAX; ++kt) {
                        if (kt < KT) {
                            gch[0][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st][kt], y, gch[0][kt], 0, 0, 0);
                            gch[1][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st][kt], y2, gch[1][kt], 0, 0, 0);
                            if constexpr (MASKED) acc[2][kt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st][kt], mi, acc[2][kt][ft], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                    for (int kt = 0; kt < KTMAX; ++kt) {
                        if (kt < KT) acc[ch][kt][ft] += gch[ch][kt];
                    }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (tile % DM_FLUSH_TILES == DM_FLUSH_TILES - 1 || t0 + DIAG_TILE >= r1) {
            // accumulator word v of tile (kt, ft) in lane (i16, j4): component 16 kt + 4 j4 + v, column 16 ft + i16
            const bool first = tile < DM_FLUSH_TILES;
            // the slab words are addressed from a value the compiler cannot see through: hoisted out of the tile loop, the addresses of
            // every (k, f, chain) word are more registers than the kernel has and the masked K > 16 forms spill
            int opaque = 0;
            asm volatile("" : "+v"(opaque));
            double* const fslab = slab + opaque;
#pragma unroll
            for (int kt = 0; kt < KTMAX; ++kt) {
                if (kt < KT) {
#pragma unroll
                    for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int k = 16 * kt + 4 * j4 + v, f = 16 * ft + i16;
                            if (k < K && f < D) {
                                double* w = fslab + k * SW;
#pragma unroll
                                for (int ch = 0; ch < NCH; ++ch)
                                    w[1 + ch * D + f] = (first ? 0.0 : w[1 + ch * D + f]) + (double)acc[ch][kt][ft][v];
                            }
                        }
#pragma unroll
                        for (int ch = 0; ch < NCH; ++ch) acc[ch][kt][ft] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    const float sn = rows4_sum(nk[kt]);
                    const int k = 16 * kt + i16;
                    if (j4 == 0 && k < K) fslab[k * SW] = (first ? 0.0 : fslab[k * SW]) + (double)sn;
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

struct DmfitGatherArgs {
    const double* slab;
    const double* partials;
    const float* pivot;
    const float* pack;    // the pack of the pass: its m and lbar complete the missing entries
    double* stats;        // (K, 1 + 2 D) or NULL
    double* bound;        // (1) or NULL
    int nwaves, nblk, K, D, masked;
};

// One block per component: lane d of wave group j adds Nk, s1_d, s2_d and (masked) M_d of the waves j, j + 16, ... in that order, the
// 16 group sums are added in group order, then the shift by the pivot p is undone on the observed part and the missing part is
// completed with the pack's own fp32 m and lbar (exact in fp64):
//   sx = s1 + (Nk - M) p + M m,   sxx = s2 + 2 p s1 + (Nk - M) p^2 + M (m^2 + 1 / lbar).
// Block 0 also adds the blocks' data terms.
__global__ __launch_bounds__(DM_RED_GROUPS * WAVE) void dmfit_gather_kernel(DmfitGatherArgs a) {
    __shared__ double part[4][DM_RED_GROUPS][WAVE];
    __shared__ double bsum[WAVE];
    const int k = blockIdx.x, grp = threadIdx.x >> 6, d = threadIdx.x & 63;
    const int D = a.D, SW = 1 + (a.masked ? 3 : 2) * D, PW = 3 * D + 1;
    if (a.stats) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (d < D)
            for (int w = grp; w < a.nwaves; w += DM_RED_GROUPS) {
                const double* p = a.slab + ((long long)w * a.K + k) * SW;
                s0 += p[0]; s1 += p[1 + d]; s2 += p[1 + D + d];
                if (a.masked) s3 += p[1 + 2 * D + d];
            }
        part[0][grp][d] = s0; part[1][grp][d] = s1; part[2][grp][d] = s2; part[3][grp][d] = s3;
        __syncthreads();
        if (grp == 0 && d < D) {
            double t0 = part[0][0][d], t1 = part[1][0][d], t2 = part[2][0][d], t3 = part[3][0][d];
#pragma unroll
            for (int j = 1; j < DM_RED_GROUPS; ++j) { t0 += part[0][j][d]; t1 += part[1][j][d]; t2 += part[2][j][d]; t3 += part[3][j][d]; }
            const double p = (double)a.pivot[d];
            double* out = a.stats + (long long)k * (1 + 2 * D);
            double sx = t1 + (t0 - t3) * p;
            double sxx = t2 + 2.0 * p * t1 + (t0 - t3) * p * p;
            if (a.masked) {
                const double m = (double)a.pack[(long long)k * PW + d], lbar = (double)a.pack[(long long)k * PW + D + d];
                sx += t3 * m;
                sxx += t3 * (m * m + 1.0 / lbar);
            }
            if (d == 0) out[0] = t0;
            out[1 + d] = sx;
            out[1 + D + d] = sxx;
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
            *a.bound = t;
        }
    }
}

// psi(x) for x > 0 and finite, NaN otherwise
__device__ __forceinline__ double dm_psi(double x) { return (x > 0.0 && x < 1e300) ? digamma_d(x) : __builtin_nan(""); }

struct DmfitPrepArgs {
    const float *alpha, *beta, *m, *a, *b;
    float* pack;
    int D, K;
};

// one block per component, lane d; the sum over d by lane 0 in d order.  b, a or beta not positive: a NaN row.
__global__ __launch_bounds__(WAVE) void dmfit_prep_kernel(DmfitPrepArgs a) {
    __shared__ double logb[WAVE];
    __shared__ int bad[WAVE];
    const int k = blockIdx.x, d = threadIdx.x, D = a.D, PW = 3 * D + 1;
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
        out[2 * D + d] = nbad ? qnan : (float)(-0.5 * log(lam));
    }
    if (d == 0) {
        double asum = 0.0;
        for (int j = 0; j < a.K; ++j) asum += a.alpha[j];
        const double c = dm_psi((double)a.alpha[k]) - dm_psi(asum) + 0.5 * (D * dm_psi(ak) - s) - 0.5 * D / bk;
        out[3 * D] = nbad ? qnan : (float)c;
    }
}

template <bool MASKED>
int launch_dmfit_dim(int D, const DmfitArgs& a, const float* pack, int blocks, size_t lds, hipStream_t s) {
    return dispatch_dim<VMP_DIAG_MAX_D>(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        return a.K <= 16 ? launch_dyn_lds(dmfit_cell_kernel<DD, 1, MASKED>, "dmfit_cell_kernel", blocks, DIAG_NW * WAVE, lds, s, a, pack)
                         : launch_dyn_lds(dmfit_cell_kernel<DD, 4, MASKED>, "dmfit_cell_kernel", blocks, DIAG_NW * WAVE, lds, s, a, pack);
    });
}

// every refusal of the pass, decided on the host
int dmfit_pass_check(const char* who, const float* x, const uint8_t* mask, int64_t N, int D, int K, const float* pack, const float* r_out,
                     const float* logr_out, const float* x_fill_out, const double* stats_out, const double* bound_out, const void* ws,
                     size_t ws_bytes) {
    int rc = stream_dims(who, D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (N <= 0) { set_error("%s: N must be positive (got %lld)", who, (long long)N); return VMP_E_BADARG; }
    if (!x || !pack) { set_error("%s: null pointer (%s)", who, !x ? "x" : "pack"); return VMP_E_BADARG; }
    if (!r_out && !logr_out && !x_fill_out && !stats_out && !bound_out) {
        set_error("%s: no output requested (r_out, logr_out, x_fill_out, stats_out and bound_out are all NULL)", who);
        return VMP_E_BADARG;
    }
    if (!r_out && logr_out) { set_error("%s: logr_out needs r_out", who); return VMP_E_BADARG; }
    if (x_fill_out && !mask) { set_error("%s: x_fill_out needs mask (a complete row has nothing to fill)", who); return VMP_E_BADARG; }
    return workspace_check(who, ws, ws_bytes, vmp_mixture_diag_mfit_workspace_bytes(N, D, K));
}

}  // namespace

extern "C" {

int vmp_mixture_diag_mfit_pack_words(int D) { return (D < 1 || D > VMP_DIAG_MAX_D) ? 0 : 3 * D + 1; }

size_t vmp_mixture_diag_mfit_workspace_bytes(int64_t N, int D, int K) {
    if (D < 1 || D > VMP_DIAG_MAX_D || K < 1 || K > VMP_MAX_K) return 0;
    // the fp64 moments of every wave (masked size) | one fp64 partial per block | the pivot (64 fp32 words)
    return dm_slab_bytes(N, D, K) + (size_t)dm_blocks(N, D, K) * sizeof(double) + 64 * sizeof(float);
}

int vmp_mixture_diag_mfit_pack(int D, int K, const float* alpha, const float* beta, const float* m, const float* a, const float* b,
                               float* pack, void* stream) {
    int rc = stream_dims("vmp_mixture_diag_mfit_pack", D, K, VMP_DIAG_MAX_D);
    if (rc) return rc;
    if (!alpha || !beta || !m || !a || !b || !pack) {
        set_error("vmp_mixture_diag_mfit_pack: null pointer (posterior or pack)");
        return VMP_E_BADARG;
    }
    DmfitPrepArgs pa{alpha, beta, m, a, b, pack, D, K};
    hipLaunchKernelGGL(dmfit_prep_kernel, dim3(K), dim3(WAVE), 0, static_cast<hipStream_t>(stream), pa);
    return check_launch("dmfit_prep_kernel");
}

int vmp_mixture_diag_mfit_pass(const float* x, const uint8_t* mask, const float* w, int64_t N, int D, int K, const float* pack,
                               float* r_out, float* logr_out, float* x_fill_out, double* stats_out, double* bound_out, void* ws,
                               size_t ws_bytes, void* stream) {
    int rc = dmfit_pass_check("vmp_mixture_diag_mfit_pass", x, mask, N, D, K, pack, r_out, logr_out, x_fill_out, stats_out, bound_out, ws,
                              ws_bytes);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = dm_blocks(N, D, K);
    const long long waves = (long long)blocks * DIAG_NW;
    DmfitArgs a{};
    a.x = x; a.mask = mask; a.w = w; a.r = r_out; a.logr = logr_out; a.xfill = x_fill_out;
    a.slab = static_cast<double*>(ws);
    a.partials = reinterpret_cast<double*>(static_cast<char*>(ws) + dm_slab_bytes(N, D, K));
    a.pivot = reinterpret_cast<float*>(a.partials + blocks);
    a.N = N; a.K = K;
    a.rpw = rows_per_wave(N, waves, DIAG_TILE);
    const size_t lds = dm_lds_bytes(D, K, mask != nullptr);
    rc = mask ? launch_dmfit_dim<true>(D, a, pack, blocks, lds, s) : launch_dmfit_dim<false>(D, a, pack, blocks, lds, s);
    if (rc) return rc;
    if (stats_out || bound_out) {
        DmfitGatherArgs ga{a.slab, a.partials, a.pivot, pack, stats_out, bound_out, (int)waves, blocks, K, D, mask ? 1 : 0};
        hipLaunchKernelGGL(dmfit_gather_kernel, dim3(stats_out ? K : 1), dim3(DM_RED_GROUPS * WAVE), 0, s, ga);
        rc = check_launch("dmfit_gather_kernel");
    }
    return rc;
}

int vmp_mixture_diag_mfit_iterate(const float* x, const uint8_t* mask, const float* w, int64_t N, int D, int K, const float* alpha0,
                                  const float* beta0, const float* m0, const float* a0, const float* b0, float* r, float* logr,
                                  float* x_fill, float* alpha, float* beta, float* m, float* a, float* b, float* xbar, float* S,
                                  float* pi, float* pack, double* stats, double* bound, void* ws, size_t ws_bytes, int iterations,
                                  void* stream) {
    const char* who = "vmp_mixture_diag_mfit_iterate";
    if (!stats) {
        int rc = stream_dims(who, D, K, VMP_DIAG_MAX_D);
        if (rc) return rc;
        set_error("%s: null pointer (stats)", who);
        return VMP_E_BADARG;
    }
    int rc = dmfit_pass_check(who, x, mask, N, D, K, pack, r, logr, x_fill, stats, bound, ws, ws_bytes);
    if (rc) return rc;
    if (iterations < 0) { set_error("%s: iterations must not be negative (got %d)", who, iterations); return VMP_E_BADARG; }
    if (!alpha0 || !beta0 || !m0 || !a0 || !b0 || !alpha || !beta || !m || !a || !b) {
        set_error("%s: null pointer (prior or posterior)", who);
        return VMP_E_BADARG;
    }
    for (int it = 0; it < iterations; ++it) {
        const bool last = it + 1 == iterations;
        if ((rc = vmp_mixture_diag_finalize(stats, D, K, alpha0, beta0, m0, a0, b0, alpha, beta, m, a, b, xbar, S, pi, stream)) != 0) return rc;
        if ((rc = vmp_mixture_diag_mfit_pack(D, K, alpha, beta, m, a, b, pack, stream)) != 0) return rc;
        if ((rc = vmp_mixture_diag_mfit_pass(x, mask, w, N, D, K, pack, last ? r : nullptr, last ? logr : nullptr, last ? x_fill : nullptr,
                                             stats, bound, ws, ws_bytes, stream)) != 0) return rc;
    }
    return 0;
}

}  // extern "C"
