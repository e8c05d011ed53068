// What the streaming mixture kernels share: the deterministic row sum and the host-side geometry and refusals.  Users: vmp_score.hip
// and vmp_seed.hip directly; vmp_impute.hip and vmp_sample.hip through vmp_impute_pack.h (the impute pack); vmp_missfit.hip,
// vmp_wfit.hip and vmp_bound.hip through vmp_fit_cell.h (the fit pack and its cell); vmp_diagfit.hip and vmp_diagscore.hip through
// vmp_diag_stream.h (the diagonal row tile).  Each of the nine files states its own feature's mathematics.
//
// Lane map: lane l = (i16 = l & 15, kk = l >> 4) owns component k = i16 + 16 t of every component tile t and, per loop iteration,
// the data row n + kk (the score kernel: two rows, n + kk and n + 4 + kk): the 16 lanes of a DPP row cover one data row, max and sum
// over k are row_ror all-reduces (vmp_common.h), and a wave walks a contiguous range of rows that depends on (N, blocks) only.
//
// The row sum: the lanes with i16 = 0 add their rows' fp32 results into an fp64 register in row order; lanes 0, 16, 32, 48, then the
// waves of a block, then (second launch, one wave) the blocks are added in a fixed order - no atomics, and the same geometry
// whichever outputs are requested, so the sum is bit-identical from run to run and from one output set to another.
#pragma once
#include "vmp_common.h"
#include "vmp_linalg.h"

namespace vmp {

// acc: per lane, the fp64 sum of its rows' results.  Lanes 0, 16, 32, 48 hold the sums of the rows = kk (mod 4) of the wave's range;
// they are added, then the NW waves of the block, into partials[blockIdx.x].  Called by every thread of the block.
template <int NW>
__device__ __forceinline__ void wave_block_sum(double acc, int lane, int wave, double* __restrict__ partials) {
    __shared__ double wsum[NW];
    const double w = (readlane_d(acc, 0) + readlane_d(acc, 16)) + (readlane_d(acc, 32) + readlane_d(acc, 48));
    if (lane == 0) wsum[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int j = 1; j < NW; ++j) s += wsum[j];
        partials[blockIdx.x] = s;
    }
}

// Fixed-order sum of the per-block partials, the body of a one-wave kernel: lane l adds blocks l, l + 64, ...; the 64 lane sums are
// added in lane order.  The kernel itself stays in each feature's file under the feature's name (score_sum_kernel,
// impute_sum_kernel): the names are what launch errors, profiles and the no-scratch tests of the code object know them by.
__device__ __forceinline__ void block_sum(const double* partials, int nblk, double* out) {
    __shared__ double part[WAVE];
    double s = 0.0;
    for (int j = threadIdx.x; j < nblk; j += WAVE) s += partials[j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
        for (int j = 1; j < WAVE; ++j) t += part[j];
        *out = t;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
inline int stream_dims(const char* who, int D, int K, int max_d = VMP_MAX_D) {
    if (D < 1 || D > max_d) { set_error("%s: D=%d outside compiled range 1..%d", who, D, max_d); return VMP_E_DIM; }
    if (K < 1 || K > VMP_MAX_K) { set_error("%s: K=%d outside compiled range 1..%d", who, K, VMP_MAX_K); return VMP_E_DIM; }
    return 0;
}

// blocks of a streaming launch: one per rows_per_block rows (below that a block is not worth its launch slot), 1 .. max_blocks
inline int stream_blocks(int64_t N, int64_t rows_per_block, int max_blocks) {
    const int64_t b = (N + rows_per_block - 1) / rows_per_block;
    return (int)(b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

// rows per wave, a multiple of the `step` rows a wave advances per iteration: wave g owns rows [g rpw, min(N, (g+1) rpw))
inline long long rows_per_wave(int64_t N, long long waves, int step) { return ((N + waves - 1) / waves + step - 1) / step * step; }

// the refusals of a workspace that holds fp64 words: `need` bytes, 8-byte aligned
inline int workspace_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need) {
        set_error("%s: workspace too small (%zu bytes, need %zu)", who, ws ? ws_bytes : (size_t)0, need);
        return VMP_E_WS;
    }
    if (reinterpret_cast<uintptr_t>(ws) & 7) { set_error("%s: workspace not 8-byte aligned", who); return VMP_E_BADARG; }
    return 0;
}

// the refusals of a requested row sum (sum_out != NULL): the workspace holds one fp64 partial per block
inline int sum_workspace_check(const char* who, const double* sum_out, const void* ws, size_t ws_bytes, size_t need) {
    if (!sum_out) return 0;
    if (!ws || ws_bytes < need) {
        set_error("%s: workspace too small for the row sum (%zu bytes, need %zu)", who, ws ? ws_bytes : (size_t)0, need);
        return VMP_E_WS;
    }
    if (reinterpret_cast<uintptr_t>(ws) & 7) { set_error("%s: workspace not 8-byte aligned", who); return VMP_E_BADARG; }
    return 0;
}

}  // namespace vmp
