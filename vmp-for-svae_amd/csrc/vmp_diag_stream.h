// What the two row-lane tile kernels of the diagonal-covariance mixture share (diag_pass_kernel in vmp_diagfit.hip, dscore_pass_kernel
// in vmp_diagscore.hip): DIAG_NW waves per block, wave g owns the rows [g rpw, (g+1) rpw) and walks them in tiles of DIAG_TILE rows,
// lane = row; a tile lives in the wave's own LDS with an odd row stride and moves to and from global memory with coalesced accesses.
// Here: that movement and the host side of a launch.  The cell arithmetic, the row softmax, the fp64 row sum, the packs and the M-part
// stay in their files: as helpers they compute the same bits from other machine code (profiles/NOTES_mix_diag_shared.md).
#pragma once
#include <type_traits>
#include "vmp_mix_stream.h"

namespace vmp {

constexpr int DIAG_NW = 4;                    // waves per block
constexpr int DIAG_TILE = 64;                 // rows of a tile: one per lane

typedef const __attribute__((address_space(4))) float cfloat;   // the pack, read through the constant address space: scalar loads

// `total` contiguous elements of src -> the LDS tile dst of DIAG_TILE rows x `width` with row stride `stride`; the rest becomes zeros
template <typename T>
__device__ __forceinline__ void tile_stage(const T* src, T* dst, int total, int width, int stride, int lane) {
    int row = lane / width, col = lane % width;
    for (int i = lane; i < DIAG_TILE * width; i += WAVE) {
        dst[row * stride + col] = i < total ? src[i] : T(0);
        col += WAVE;
        while (col >= width) { col -= width; ++row; }
    }
}

// the other way: the first `total` words of the LDS tile (rows of `width`, row stride `stride`) -> contiguous dst
__device__ __forceinline__ void tile_store(float* dst, const float* tile, int total, int width, int stride, int lane) {
    int row = lane / width, col = lane % width;
    for (int i = lane; i < total; i += WAVE) {
        dst[i] = tile[row * stride + col];
        col += WAVE;
        while (col >= width) { col -= width; ++row; }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, D>) for the run-time D in 1..MAX, the value a template argument to f's body; -1 outside (the entry
// points have refused it before)
template <int MAX, typename F>
int dispatch_dim(int D, F&& f) {
    if constexpr (MAX < 1) {
        return -1;
    } else {
        return D == MAX ? f(std::integral_constant<int, MAX>{}) : dispatch_dim<MAX - 1>(D, f);
    }
}

// launch with `lds` bytes of dynamic LDS; above the 48 KB a kernel may use by default its limit is raised first
template <typename Kernel, typename... Args>
int launch_dyn_lds(Kernel kernel, const char* name, int blocks, int threads, size_t lds, hipStream_t s, Args... args) {
    if (lds > 48 * 1024)
        if (const int rc = set_dyn_lds(reinterpret_cast<const void*>(kernel), lds, name)) return rc;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, s, args...);
    return check_launch(name);
}

}  // namespace vmp
