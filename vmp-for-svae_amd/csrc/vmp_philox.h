// The counter-based random stream of the streaming mixture kernels (vmp_sample.hip, vmp_seed.hip): Philox4x32 at
// VMP_PHILOX_ROUNDS rounds - the generator of vmp_svae.hip and of oracle/philox.py philox4x32 - with key = seed and a counter whose
// first two words are the ABSOLUTE row index, so that a value is a function of (seed, row, c2, c3) and of nothing else.  The fourth
// counter word keeps the streams of the library apart: 0 is the cell noise of vmp_svae.hip, SUBSAMPLE_TAG its categorical draw,
// 0x6d78a500 + b the blocks of vmp_sample.hip, 0x6b6d2b00 the exponential race of vmp_seed.hip.
#pragma once
#include "vmp_common.h"

#ifndef VMP_PHILOX_ROUNDS
#define VMP_PHILOX_ROUNDS 7
#endif

namespace vmp {

// c <- Philox4x32(counter = c, key = seed)
__device__ __forceinline__ void philox_rounds(unsigned (&c)[4], unsigned long long seed) {
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < VMP_PHILOX_ROUNDS; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned)p1; c[3] = (unsigned)p0; c[0] = n0; c[2] = n2;
    }
}

// (top 24 bits of a word + 1/2) 2^-24, rounded once to fp32 (ties to even) and kept at most 1 - 2^-24: in (0, 1), never 0, never 1
__device__ __forceinline__ float philox_uniform24(unsigned w) {
    return fminf(fmaf((float)(w >> 8), 5.9604644775390625e-08f, 2.98023223876953125e-08f), 0.99999994f);
}

}  // namespace vmp
