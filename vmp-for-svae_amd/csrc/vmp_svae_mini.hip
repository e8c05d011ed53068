// Minibatch form of the SVAE E-step backward (round 6; launcher: vmp_svae_estep_bwd_n in vmp_svae.hip).  A separate translation unit
// built with -fno-slp-vectorize, like the ring kernels: the SLP vectoriser packs this scalar cell arithmetic into v_pk_*_f32 with
// op_sel on src1, the operand form of the hardware note in vmp_common.h (tools/erratum_scan.py, tests/test_abi.py).
#include "vmp_svae_cell.h"
#include "vmp_tail.h"

using namespace vmp;

namespace {

// ---------------------------------------------------------------------------------------------------------
// Minibatch form of the backward kernel (round 6, Gaussian theta): lane = (cell, sample PAIR), the mirror of svae_estep_fwd1_kernel.
// One block per tile, wave p takes the sample pair p: every wave repeats the cell factorisation and runs the adjoint of ITS two
// samples (w_s = Lt^-1 gx_s, the sums W = sum_s w_s and M = sum_s e_s w_s^T); the L + TRI per-cell sums meet in LDS, wave 0 adds them
// in pair order and does the assembly (Cholesky adjoint, rank-one terms), the per-row gradients and the tile's per-component sums,
// which are this block's partial row.  (The generic kernel's one-tile form walks the S / 2 pairs one after the other behind the
// factorisation: 19 us at N = 64; partial rows: one per TILE here - vmp_svae_bwd_blocks_for.)
// ---------------------------------------------------------------------------------------------------------
constexpr int BWD1_MAX_PAIRS = 8;
// TAIL (round 6, the minibatch training step): the scalar tail of the ELBO runs in here instead of in a launch of its own - every pair
// wave forms dLoss/dT' = -sigma r of its cell; ONE MORE wave (beside the S / 2 pair waves; with S = 16 the block is full and wave 0
// does it) forms dLoss/dlog_z from the cell's S reconstruction sums (tail_cell, vmp_tail.h: the arithmetic of elbo_tail_body), writes
// r = exp(log z) and the tile's terms of the ELBO's two fp64 sums, and hands dLoss/dlog_z to wave 0 through LDS - it is done long
// before the pair waves reach the block barrier.
// STUDENT (the SMM-SVAE's minibatch step, vmp_svae_estep_bwd_tail_t): Student-t theta (nu = a.nu), trainable - every pair wave also
// sums the theta-term adjoint of its two samples (dL/dm = -W^T c y, dL/dW = c y d^T, c = (nu+L)/(nu+delta^2); the generic kernel's
// arithmetic), and these L + TRI per-pair sums meet in wave 0 in a SECOND round through the same LDS area (both rounds at once would
// need 2 x 8 x 44 x 64 floats at L = 8, S = 16: more than the 160 KiB of a CU).  The partial row then carries its theta half
// (words TH..2TH-1: g_mk | g_Wk lower | g_kappa), the layout vmp_svae_bwd_reduce reads for nu != NULL.
template <int L, bool TAIL, bool STUDENT = false>
__global__ __launch_bounds__(BWD1_MAX_PAIRS * WAVE) void svae_estep_bwd1_kernel(EBwdArgs a) {
    constexpr int TRI = SvGeo<L>::TRI, TH = L + TRI + 1, PW = 2 * TH, NV = L + TRI;
    constexpr int PWA = STUDENT ? PW : TH;                  // accumulator rows of wave 0's epilogue
    constexpr int AST = SV_AST;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int K = a.K, S = a.S, LSn = L * S;
    const int RPT = WAVE / K, CT = RPT * K;
    const int np = (S + 1) / 2;                              // pair waves; TAIL: one more wave, if the block has it, runs the scalar tail
    const bool tailw = TAIL && nw > np;
    float* scr = smem + wave * WAVE;                         // [nw][64] row-reduction scratch (the tail wave's slot: dLoss/dlog_z of the cells)
    float* red = smem + nw * WAVE;                           // [np][NV][64] per-pair sums
    float* accl = red;                                       // wave 0, after the sums are read: [PWA][AST] per-lane values of the tile
    float* rows = red + PWA * AST;                           //                                  [2L][AST] row-sum scratch
    const bool lane_on = lane < CT;
    const int r = lane / K, k = lane - r * K, rbase = lane_on ? r * K : 0, kc = lane_on ? k : 0;
    const long long t = blockIdx.x, row = t * RPT + r;
    const bool on = lane_on && row < a.N;
    const long long rowc = on ? row : 0, cellid = rowc * K + kc;
    float Lm[TRI], mu[L], Wsum[L], M[TRI];
    float Tm[STUDENT ? L : 1], Tw[STUDENT ? TRI : 1];        // STUDENT: theta-side sums (dL/dm, dL/dW lower) of this wave's samples
    float glzv = 0.f, gT = 0.f;
    const float lzv = a.lz[cellid];
    if (TAIL && (tailw ? wave == np : wave == 0)) {
        // ---- the scalar tail of the ELBO for this tile's cells (tail_cell: the arithmetic of elbo_tail_body)
        const float* __restrict__ lr = a.ll + cellid * S;
        float lv[2 * BWD1_MAX_PAIRS];                        // all loads in flight together (a run-time loop waits for each in turn)
#pragma unroll
        for (int s = 0; s < 2 * BWD1_MAX_PAIRS; ++s) lv[s] = lr[s < S ? s : 0];
        const float tpv = a.Tp[cellid];
        float A = 0.f;
#pragma unroll
        for (int s = 0; s < 2 * BWD1_MAX_PAIRS; ++s)
            if (s < S) A += lv[s];
        float rr, gtp;
        double wa = 0.0, rg = 0.0;
        tail_cell(lzv, tpv, A, 0.5f / (float)S, a.sigma, rr, glzv, gtp, wa, rg);
        if (on) a.r_out[cellid] = rr;
        wa = tail_wave_sum(on ? wa : 0.0);
        rg = tail_wave_sum(on ? rg : 0.0);
        if (lane == 0) { a.tail_part[2 * blockIdx.x] = wa; a.tail_part[2 * blockIdx.x + 1] = rg; }
        if (tailw) scr[lane] = glzv;                         // (read by wave 0 behind the block barrier)
    }
    if (wave < np) {
    // ---- everything this lane needs, requested at once
    const int s0 = 2 * wave;
    const bool h1 = s0 + 1 < S;
    float xp[2 * L], gp[2 * L];
    {
        const float* __restrict__ xc = a.x + cellid * LSn + s0 * L;
        const float* __restrict__ gc = a.Gx + cellid * LSn + s0 * L;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const float xv = xc[i], gv = gc[i], xw = xc[h1 ? L + i : i], gw = gc[h1 ? L + i : i];
            xp[i] = on ? xv : 0.f; gp[i] = on ? gv : 0.f;
            xp[L + i] = (on && h1) ? xw : 0.f; gp[L + i] = (on && h1) ? gw : 0.f;
        }
    }
    float av[L], hkk[L], mkk[L], Wt[TRI];
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const float e1 = a.eta1[rowc * L + i], e2 = a.eta2d[rowc * L + i], hv = a.hk[kc * L + i], mv = a.mk[kc * L + i];
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const float pv = a.Pk[(kc * L + i) * L + j], wv = a.Wk[(kc * L + i) * L + j];
            Lm[tri(i, j)] = lane_on ? pv : 0.f;
            Wt[tri(i, j)] = lane_on ? wv : 0.f;
        }
        Lm[tri(i, i)] = fmaf(-2.f, on ? e2 : -0.5f, Lm[tri(i, i)]);
        hkk[i] = lane_on ? hv : 0.f; mkk[i] = lane_on ? mv : 0.f;
        av[i] = (on ? e1 : 0.f) + hkk[i];
    }
    float gTv;
    if (TAIL) {
        float rr, g0, g1;
        double d0 = 0.0, d1 = 0.0;
        tail_cell(lzv, 0.f, 0.f, 0.5f / (float)S, a.sigma, rr, g0, gTv, d0, d1);     // dLoss/dT' = -sigma exp(log z): every pair wave needs it
    } else {
        glzv = a.Glz[cellid];
        gTv = a.GT[cellid];
    }
    float ld;
    cell_cholesky<L>(Lm, ld);
    solve_lower<L>(Lm, av);
#pragma unroll
    for (int i = 0; i < L; ++i) mu[i] = av[i];
    solve_lower_t<L>(Lm, mu);                               // mu~ = Pt^-1 ht
    gT = on ? gTv : 0.f;
    const float gts = gT * (1.0f / (float)S);
    float nuk = 1.f;
    if constexpr (STUDENT) {
        const float nv = a.nu[kc];
        nuk = lane_on ? nv : 1.f;
#pragma unroll
        for (int i = 0; i < L; ++i) Tm[i] = 0.f;
#pragma unroll
        for (int i = 0; i < TRI; ++i) Tw[i] = 0.f;
    }
    // ---- this wave's two samples
#pragma unroll
    for (int i = 0; i < L; ++i) Wsum[i] = 0.f;
#pragma unroll
    for (int i = 0; i < TRI; ++i) M[i] = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && !h1) break;
        float xs[L], gx[L], d[L], y[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { xs[i] = xp[h * L + i]; gx[i] = gp[h * L + i]; d[i] = xs[i] - mkk[i]; }
        float del2 = 0.f;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            float yy = 0.f;
#pragma unroll
            for (int j = 0; j <= i; ++j) yy = fmaf(Wt[tri(i, j)], d[j], yy);
            y[i] = yy;
            if (STUDENT) del2 = fmaf(yy, yy, del2);
        }
        // d/dx of the theta term of T':  (1/S) c_s W^T W (x - m),  c_s = 1 (Gaussian) or (nu+L)/(nu+delta^2)
        const float gc = STUDENT ? gts * (nuk + (float)L) / (nuk + del2) : gts;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const float gy = gc * y[i];
#pragma unroll
            for (int j = 0; j <= i; ++j) gx[j] = fmaf(Wt[tri(i, j)], gy, gx[j]);
        }
        if constexpr (STUDENT) {
            // theta is trainable in the SMM model: d/dm = -(the x-gradient of the theta term), d/dW = c y d^T (off cells: gts = 0)
            float tx[L];
#pragma unroll
            for (int j = 0; j < L; ++j) tx[j] = 0.f;
#pragma unroll
            for (int i = 0; i < L; ++i) {
                const float gy = gc * y[i];
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    tx[j] = fmaf(Wt[tri(i, j)], gy, tx[j]);
                    Tw[tri(i, j)] = fmaf(gy, d[j], Tw[tri(i, j)]);
                }
            }
#pragma unroll
            for (int j = 0; j < L; ++j) Tm[j] -= tx[j];
        }
        solve_lower<L>(Lm, gx);                             // w_s = Lt^-1 gx_s
#pragma unroll
        for (int i = 0; i < L; ++i) {
            Wsum[i] += gx[i];
            const float e = xs[i] - mu[i];                  // e_s = Lt^-T eps_s
#pragma unroll
            for (int j = 0; j <= i; ++j) M[tri(i, j)] = fmaf(e, gx[j], M[tri(i, j)]);
        }
    }
    {
        float* rw = red + wave * (NV * WAVE) + lane;
#pragma unroll
        for (int i = 0; i < L; ++i) rw[i * WAVE] = Wsum[i];
#pragma unroll
        for (int i = 0; i < TRI; ++i) rw[(L + i) * WAVE] = M[i];
    }
    }   // pair waves
    __syncthreads();
    if (wave == 0) {
    if (tailw) glzv = smem[np * WAVE + lane];
    for (int w = 1; w < np; ++w) {
        const float* rw = red + w * (NV * WAVE) + lane;
#pragma unroll
        for (int i = 0; i < L; ++i) Wsum[i] += rw[i * WAVE];
#pragma unroll
        for (int i = 0; i < TRI; ++i) M[i] += rw[(L + i) * WAVE];
    }
    }   // wave 0
    if constexpr (STUDENT) {
        // second round: the theta-side sums of the pair waves 1.. through the same LDS area, once wave 0 has read the first
        __syncthreads();
        if (wave > 0 && wave < np) {
            float* rw = red + wave * (NV * WAVE) + lane;
#pragma unroll
            for (int i = 0; i < L; ++i) rw[i * WAVE] = Tm[i];
#pragma unroll
            for (int i = 0; i < TRI; ++i) rw[(L + i) * WAVE] = Tw[i];
        }
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < np; ++w) {
                const float* rw = red + w * (NV * WAVE) + lane;
#pragma unroll
                for (int i = 0; i < L; ++i) Tm[i] += rw[i * WAVE];
#pragma unroll
                for (int i = 0; i < TRI; ++i) Tw[i] += rw[(L + i) * WAVE];
            }
        }
    }
    if (wave == 0) {
    __builtin_amdgcn_wave_barrier();                         // (accl / rows below overlay the sums just read)
    if constexpr (STUDENT) {                                 // theta half of the tile's values; T' has -kappa_k
#pragma unroll
        for (int i = 0; i < L; ++i) accl[(TH + i) * AST + lane] = on ? Tm[i] : 0.f;
#pragma unroll
        for (int i = 0; i < TRI; ++i) accl[(TH + L + i) * AST + lane] = on ? Tw[i] : 0.f;
        accl[(TH + L + TRI) * AST + lane] = on ? -gT : 0.f;
    }
    const float glz = on ? glzv : 0.f;
    const float rnk = on ? __expf(lzv) : 0.f;
    const float gsum = row_sum(glz, scr, lane, rbase, K);
    const float Gc = glz - rnk * gsum;                      // through the log-sum-exp normalisation
    const float Gld = gT - Gc;                              // T' has +ld, c has -ld
    // ---- assemble dLoss/dht and dLoss/dPt (symmetric, lower triangle): as svae_estep_bwd_kernel
    float V[L];
#pragma unroll
    for (int i = 0; i < L; ++i) V[i] = Wsum[i];
    solve_lower_t<L>(Lm, V);                                // V = Pt^-1 sum_s gx_s
    float gh[L];
#pragma unroll
    for (int i = 0; i < L; ++i) gh[i] = fmaf(Gc, mu[i], V[i]);
    float Cs[TRI], dg[L];
#pragma unroll
    for (int i = 0; i < L; ++i) dg[i] = 1.0f / Lm[tri(i, i)];
#pragma unroll
    for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float s2 = 0.f;
#pragma unroll
            for (int p = i; p < L; ++p) {
                const float lpi = (p == i) ? dg[i] : Lm[tri(p, i)];
                s2 = fmaf(lpi, -M[tri(p, j)], s2);
            }
            Cs[tri(i, j)] = (i == j) ? (s2 + Gld) : s2;
        }
    float Y[TRI];
#pragma unroll
    for (int j = 0; j < L; ++j) {
        Y[tri(j, j)] = Lm[tri(j, j)];
#pragma unroll
        for (int i = j + 1; i < L; ++i) {
            float s2 = 0.f;
#pragma unroll
            for (int p = j; p < i; ++p) s2 = fmaf(Lm[tri(i, p)], Y[tri(p, j)], s2);
            Y[tri(i, j)] = -s2 * Lm[tri(i, i)];
        }
    }
    float gP[TRI];
#pragma unroll
    for (int i = 0; i < TRI; ++i) gP[i] = 0.f;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        float Zc[L];
#pragma unroll
        for (int q = 0; q < L; ++q) {
            float s2 = 0.f;
#pragma unroll
            for (int p = j; p < L; ++p) {
                const float cqp = (q >= p) ? Cs[tri(q, p)] : Cs[tri(p, q)];
                s2 = fmaf(cqp, Y[tri(p, j)], s2);
            }
            Zc[q] = s2;
        }
#pragma unroll
        for (int i = j; i < L; ++i) {
            float s2 = 0.f;
#pragma unroll
            for (int p = i; p < L; ++p) s2 = fmaf(Y[tri(p, i)], Zc[p], s2);
            gP[tri(i, j)] = 0.5f * s2;
        }
    }
#pragma unroll
    for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j)
            gP[tri(i, j)] += -0.5f * (V[i] * mu[j] + mu[i] * V[j]) - 0.5f * Gc * mu[i] * mu[j];
    // ---- the tile's values to LDS: per-row sums (encoder gradients) and per-component sums (this block's partial row)
#pragma unroll
    for (int i = 0; i < L; ++i) {
        accl[i * AST + lane] = on ? gh[i] : 0.f;
        rows[i * AST + lane] = on ? gh[i] : 0.f;
        rows[(L + i) * AST + lane] = on ? gP[tri(i, i)] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TRI; ++i) accl[(L + i) * AST + lane] = on ? gP[i] : 0.f;
    accl[(L + TRI) * AST + lane] = on ? Gc : 0.f;
    }   // wave 0
    // ---- the whole block shares the two output loops (the other waves have been waiting for wave 0's assembly)
    __syncthreads();
    for (int q0 = threadIdx.x; q0 < 2 * L * RPT; q0 += blockDim.x) {
        const int rr = q0 / (2 * L), i0 = q0 - rr * (2 * L);
        const float* __restrict__ p0 = rows + i0 * AST + rr * K;
        float sq = 0.f;
#pragma unroll 4
        for (int j = 0; j < K; ++j) sq += p0[j];
        const long long row0 = t * RPT + rr;
        if (row0 < a.N) {
            if (i0 < L) a.g_eta1[row0 * L + i0] = sq;
            else a.g_eta2d[row0 * L + (i0 - L)] = -2.f * sq;   // p = -2 eta2d
        }
    }
    float* out = a.partials + (long long)blockIdx.x * K * PW;
    for (int e = threadIdx.x; e < K * PW; e += blockDim.x) {
        const int kk = e / PW, f = e - kk * PW;
        float sq = 0.f;
        if (f < PWA)
            for (int rr = 0; rr < RPT; ++rr) sq += accl[f * AST + rr * K + kk];
        out[e] = sq;
    }
}

template <int L, bool TAIL, bool STUDENT = false>
int launch_bwd1(const EBwdArgs& a, int ntiles, int P, void* stream) {
    constexpr int TRI = L * (L + 1) / 2;
    constexpr int NV = L + TRI;
    constexpr int TH = L + TRI + 1;
    const int epi = (STUDENT ? 2 * TH : TH) * SV_AST + 2 * L * SV_AST;
    const int work = P * NV * WAVE > epi ? P * NV * WAVE : epi;
    const int nwv = (TAIL && P < BWD1_MAX_PAIRS) ? P + 1 : P;       // the tail wave (with S = 16 the block is full: wave 0 runs the tail)
    const size_t lds1 = (size_t)(nwv * WAVE + work) * sizeof(float);
    if (lds1 > 48 * 1024) {
        if (const int rc = set_dyn_lds(reinterpret_cast<const void*>(svae_estep_bwd1_kernel<L, TAIL, STUDENT>), lds1, "svae_estep_bwd1_kernel")) return rc;
    }
    hipLaunchKernelGGL((svae_estep_bwd1_kernel<L, TAIL, STUDENT>), dim3(ntiles), dim3(nwv * WAVE), lds1, static_cast<hipStream_t>(stream), a);
    return check_launch("svae_estep_bwd1_kernel");
}

}  // namespace

namespace vmp {
int svae_bwd1_launch(const EBwdArgs& a, int L, int ntiles, int P, bool tail, bool student, void* stream) {
    if (student && !tail) { set_error("svae_estep_bwd1_kernel: Student-t theta is compiled with the tail only"); return VMP_E_BADARG; }
    // student: the theta half of every partial row is written
    VMP_SWITCH_DIM(L, LL, return student ? launch_bwd1<LL, true, true>(a, ntiles, P, stream)
                                 : tail ? launch_bwd1<LL, true>(a, ntiles, P, stream) : launch_bwd1<LL, false>(a, ntiles, P, stream));
    return -1;                                // an L outside 1..8
}
}  // namespace vmp
