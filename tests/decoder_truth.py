"""fp64 yardsticks for the fused decoder / encoder backward (csrc/vmp_decoder.hip, dec_bwd_kernel<UT, FS, GIN, BT>) at row counts
where one autograd graph is too big, and a pure-Python restatement of the kernel's tile-range arithmetic.  CPU only: nothing
here touches a GPU (vmp_decoder_launch_plan / vmp_decoder_bwd_blocks are host-only ABI calls).

  truth_chunked       oracle.nets.decoder / oracle.nets.mlp in fp64 with torch autograd, chunk by chunk; memory = one chunk
  two_term_emulation  the same mathematics written out by hand in fp64, with the operands the kernel's BT = 2 path splits into
                      bf16 terms replaced by their 2-term values and each product restricted to the partial products the kernel
                      issues - the "reference arithmetic's own error" yardstick of the 2-term bars (as the __f32 goldens and
                      bar() are in test_mix_gpu.py)
  bwd_plan ...        what the library's launch layer decides (vmp_decoder_launch_plan): instance, split, epilogue form, grid
  bwd_tile_plan       ntiles, grid, tpb, tpp and every wave's (t0, t1) as the top of dec_bwd_kernel computes them
  CASES ...           the shapes tests/test_decoder_tiles_gpu.py runs; tests/test_decoder_truth.py proves the branch of each
"""
import contextlib

import numpy as np
import torch

NET_VARS = ('layer_0/kernel', 'layer_0/bias', 'layer_1/kernel', 'layer_1/bias', 'gaussian_output/kernel',
            'gaussian_output/bias', 'shortcut/W', 'shortcut/b1', 'shortcut/b2')

# Sample rows from which dec_plan (csrc/vmp_decoder.hip, `#define VMP_DEC_BT2_ROWS (1u << 19)`) plans the backward kernel with BT = 2 in
# decoder mode (gradient-input mode keeps BT = 3 at every size).  Stated here and proven against vmp_decoder_launch_plan by
# tests/test_decoder_truth.py; every decision below is asked of the library.
DEC_BT2_ROWS = 1 << 19
BWD_WAVES = 8                         # BWD_THREADS / WAVE
TANH_PRESCALE = float(np.float32(2.8853900817779268))    # fill_images folds 2 log2(e) into the hidden layers' FORWARD weight images
KIND_BWD, KIND_BWD_GIN = 3, 4         # the backward `kind`s of vmp_decoder_launch_plan (include/vmp_hip.h)
PLAN_FIELDS = ('UT', 'FS', 'BT', 'split', 'red_one', 'blocks', 'threads', 'lds_bytes')


def bwd_plan(L, Dy, U, R, gin=False):
    """vmp_decoder_launch_plan's answer for the backward over R sample rows as a dict (pure host: no launch, no device)."""
    import ctypes
    import vmp_for_svae_amd as V
    out = (ctypes.c_int64 * 8)()
    V._lib.check(V._lib.lib().vmp_decoder_launch_plan(KIND_BWD_GIN if gin else KIND_BWD, R, L, Dy, U, 0, out), 'vmp_decoder_launch_plan')
    return dict(zip(PLAN_FIELDS, out))


def bwd_split(U):
    """DecArgs::split as the library plans it - the older wave's % of a SIMD pair's tiles (it depends on U alone)."""
    return bwd_plan(8, 8, U, 16)['split']


def bwd_variant(L, Dy, U, R, gin=False):
    """Template arguments and epilogue form the library plans: (UT, FS, BT, red_one)."""
    p = bwd_plan(L, Dy, U, R, gin)
    return p['UT'], bool(p['FS']), p['BT'], bool(p['red_one'])


def bwd_tile_plan(R, split, grid=None):
    """The tile ranges of dec_bwd_kernel for R sample rows; the grid is what the library launches (the plan's blocks)."""
    lib_plan = bwd_plan(*SHIPPED_NET, R)                                # (grid and BT depend on the rows alone)
    if grid is None:
        grid = lib_plan['blocks']
    ntiles = (R + 15) // 16
    tpb = (ntiles + grid - 1) // grid
    tpp = (tpb + 3) // 4
    older = (tpp * split + 50) // 100 if tpp >= 8 else (tpp + 1) // 2
    waves, empty, busy_max = [], 0, 0
    for b in range(grid):
        b0 = min(b * tpb, ntiles)
        b1 = min(b0 + tpb, ntiles)
        busy = 0
        for w in range(BWD_WAVES):
            p0 = min(b0 + (w & 3) * tpp, b1)
            p1 = min(p0 + tpp, b1)
            pm = min(p0 + older, p1)
            t0, t1 = (p0, pm) if w < 4 else (pm, p1)
            waves.append((t0, t1))
            busy += t1 > t0
        empty += busy == 0
        busy_max = max(busy_max, busy)
    return {'R': R, 'ntiles': ntiles, 'grid': grid, 'tpb': tpb, 'tpp': tpp, 'older': older, 'waves': waves,
            'empty_blocks': empty, 'busy_blocks': grid - empty, 'busy_waves_max': busy_max,
            'max_tiles_per_wave': max(t1 - t0 for t0, t1 in waves),
            'split_branch': tpp >= 8,                                   # pm comes from a.split
            'uneven': tpp >= 8 and older != (tpp + 1) // 2,             # ... and differs from the even share
            'ragged': R % 16 != 0,
            'last_short': 0 < ntiles - (grid - empty - 1) * tpb < tpb,
            'bt': lib_plan['BT']}                                       # decoder mode; gradient-input mode: 3


# ---- the shapes of tests/test_decoder_tiles_gpu.py ----------------------------------------------------------------
ROW_CASES = {  # name: (N, K, S)
    'few_tile_last': (1024, 4, 4),
    'eight_wave_first': (1025, 4, 4),
    'two_tile_first': (1561, 3, 7),
    'even_split_last': (4096, 4, 7),
    'uneven_split_first': (4097, 4, 7),
    'bt3_last': (24966, 3, 7),
    'bt2_first': (24967, 3, 7),
}
SHIPPED_NET = (8, 8, 50)                                                  # L, Dy, U
EXTRA_NETS = ((3, 2, 16), (6, 6, 32), (5, 3, 33), (8, 8, 64))
DECODER_CASES = [(name, SHIPPED_NET) for name in ROW_CASES] + \
    [(name, net) for name in ('two_tile_first', 'uneven_split_first', 'bt2_first') for net in EXTRA_NETS] + \
    [('two_tile_first', (1, 1, 1))]
GIN_ROWS = (32781, 114716, 524286, 524307)
GIN_CASES = [(R, net) for R in GIN_ROWS for net in ((8, 8, 50), (6, 6, 32))] + [(524307, (8, 8, 64))]     # R, (Din, Dout, U)


def case_rows(name):
    N, K, S = ROW_CASES[name]
    return N * K * S


def net_shapes(Ld, Dy, U):
    return ((Ld, U), (U,), (U, U), (U,), (U, 2 * Dy), (2 * Dy,), (Ld, Dy), (Dy,), (Dy,))


def _rng(seed, stream):
    return np.random.Generator(np.random.PCG64([seed, stream]))


def make_inputs(N, K, S, Ld, Dy, U, seed, wscale=0.3):
    """make_case of test_decoder_gpu.py (PCG64, wscale 0.3, x * 1.5, r in [0.05, 1.05)) drawn in fp32, so that truth and kernel
    see identical inputs, and with one generator stream per tensor: the values of a row depend on (seed, row index) only, not
    on N - two runs that differ in N share their common rows."""
    f32 = np.float32
    w = [_rng(seed, 10 + i).standard_normal(s, dtype=f32) * f32(wscale) for i, s in enumerate(net_shapes(Ld, Dy, U))]
    x = _rng(seed, 0).standard_normal((N, K, S, Ld), dtype=f32) * f32(1.5)
    y = _rng(seed, 1).standard_normal((N, Dy), dtype=f32)
    r = _rng(seed, 2).random((N, K), dtype=f32) + f32(0.05)
    return x, y, r, w


def make_gin_inputs(R, Din, Dout, U, seed, wscale=0.3):
    """Inputs of the gradient-input mode (test_fused_encoder_vs_oracle): x (R, Din) and the two upstream gradients (R, Dout)."""
    f32 = np.float32
    w = [_rng(seed, 10 + i).standard_normal(s, dtype=f32) * f32(wscale) for i, s in enumerate(net_shapes(Din, Dout, U))]
    x = _rng(seed, 0).standard_normal((R, Din), dtype=f32) * f32(1.5)
    g1 = _rng(seed, 1).standard_normal((R, Dout), dtype=f32)
    g2 = _rng(seed, 2).standard_normal((R, Dout), dtype=f32)
    return x, g1, g2, w


@contextlib.contextmanager
def _threads(limit=16):
    before = torch.get_num_threads()
    torch.set_num_threads(max(1, min(before, limit)))
    try:
        yield
    finally:
        torch.set_num_threads(before)


def _t64(a):
    return torch.as_tensor(np.asarray(a)).double()


def _chunks(n, per):
    per = max(1, per)
    return [(i, min(i + per, n)) for i in range(0, n, per)]


def truth_chunked(x, y, w, r=None, gmean=None, gvar=None, head='standard', chunk=2 ** 15):
    """fp64 truth through the oracle and torch autograd over chunks of about `chunk` sample rows.
    Decoder mode (gmean is None): x (N,K,S,L), y (N,Dy), r (N,K); loss = sum r A, A = sum_s sum_d (y-mean)^2/var + log(var+1e-8).
      -> {'A': (N,K), 'dx': (N,K,S,L), 'grads': [9]}
    Gradient-input mode: x (R,L), gmean / gvar (R,Dy) = upstream gradients of the two head outputs; loss = sum g1 o1 + sum g2 o2.
      -> {'o1': (R,Dy), 'o2': (R,Dy), 'dx': (R,L), 'grads': [9]}"""
    from oracle import nets
    gin = gmean is not None
    x = _t64(x)
    wt = [_t64(a).requires_grad_(True) for a in w]
    wd = dict(zip(NET_VARS, wt))
    grads = [torch.zeros_like(a) for a in wt]
    outs = {k: [] for k in (('o1', 'o2', 'dx') if gin else ('A', 'dx'))}
    rows_per = 1 if gin else x.shape[1] * x.shape[2]
    with _threads():
        for i0, i1 in _chunks(x.shape[0], chunk // rows_per):
            xc = x[i0:i1].clone().requires_grad_(True)
            if gin:
                o1, o2 = nets.mlp(xc, wd, head)
                loss = (o1 * _t64(gmean[i0:i1])).sum() + (o2 * _t64(gvar[i0:i1])).sum()
                outs['o1'].append(o1.detach())
                outs['o2'].append(o2.detach())
            else:
                mean, var = nets.decoder(xc, wd)
                yy = _t64(y[i0:i1]).unsqueeze(1).unsqueeze(1)
                A = ((yy - mean) ** 2 / var + torch.log(var + 1e-8)).sum(-1).sum(-1)
                loss = (A * _t64(r[i0:i1])).sum()
                outs['A'].append(A.detach())
            g = torch.autograd.grad(loss, [xc] + wt)
            outs['dx'].append(g[0])
            for acc, gi in zip(grads, g[1:]):
                acc += gi
    res = {k: torch.cat(v) for k, v in outs.items()}
    res['grads'] = grads
    return res


def split2(v):
    """The 2-term value of an operand (split_bf16<2>, vmp_common.h): hi = the fp32 value rounded to bf16 (nearest even, as
    v_cvt_pk_bf16_f32), mid = the fp32 remainder rounded to bf16.  Returns (hi, mid) in fp64."""
    v32 = v.float()
    hi = v32.bfloat16().float()
    mid = (v32 - hi).bfloat16().float()
    return hi.double(), mid.double()


def _prod_units(a, W, on):
    """a @ W over hidden units (gemm_units / gemm_units_1 with TERMS = 2): hh + hm + mh of the 2-term operands."""
    if not on:
        return a @ W
    ah, am = split2(a)
    Wh, Wm = split2(W)
    return ah @ Wh + ah @ Wm + am @ Wh


def _prod_slots(d, W, on):
    """d @ W over the 16 output slots (dh1 = W2 . dO and the shortcut part of dx; gemm_slots<2> and its inline twin): the
    (h|m) x (h|h), (h|m) x (m|m) instruction pair = hh + mh + hm + mm, i.e. the product of the two 2-term values."""
    if not on:
        return d @ W
    dh, dm = split2(d)
    Wh, Wm = split2(W)
    return (dh + dm) @ (Wh + Wm)


def two_term_emulation(x, y, w, r=None, gmean=None, gvar=None, head='standard', chunk=2 ** 15, truncate=True):
    """The arithmetic dec_bwd_kernel<.., BT = 2> documents, restated in fp64 (forward recompute and backward written out by
    hand; same return value as truth_chunked, 'A' being the value the BACKWARD launch's recompute yields).  With truncate:
      forward recompute   h0 and h1 and the weight images they meet (W1 * TANH_PRESCALE, W2): 2-term, hh + hm + mh
      backward data path  dh1 = W2 . dO and the shortcut Ws . dO of dx: 2-term values of both, all four products (K = 16 form)
                          dh0 = W1 . dh1pre, dx = W0 . dh0pre: 2-term, hh + hm + mh
    Everything else - layer 0 and the forward shortcut (3-term in every instantiation), tanh, softplus, the reconstruction term,
    the weight-gradient sums - is fp64.  truncate=False: plain fp64 backpropagation, equal to truth_chunked."""
    gin = gmean is not None
    x = _t64(x)
    W0, b0, W1, b1, W2, b2, Ws, bs1, bs2 = [_t64(a) for a in w]
    Dy = Ws.shape[1]
    vscale = 1.0 if head == 'standard' else -0.5
    grads = [torch.zeros_like(a) for a in (W0, b0, W1, b1, W2, b2, Ws, bs1, bs2)]
    outs = {k: [] for k in (('o1', 'o2', 'dx') if gin else ('A', 'dx'))}
    rows_per = 1 if gin else x.shape[1] * x.shape[2]
    sp2 = torch.log1p(torch.exp(bs2))
    W1f = W1 * TANH_PRESCALE
    with _threads():
        for i0, i1 in _chunks(x.shape[0], chunk // rows_per):
            xc = x[i0:i1]
            x2 = xc.reshape(-1, xc.shape[-1])
            h0 = torch.tanh(x2 @ W0 + b0)
            z1 = (_prod_units(h0, W1f, True) / TANH_PRESCALE if truncate else h0 @ W1) + b1
            h1 = torch.tanh(z1)
            O = _prod_units(h1, W2, truncate) + b2
            mean = O[:, :Dy] + x2 @ Ws + bs1
            raw2 = O[:, Dy:]
            var = torch.logaddexp(raw2, torch.zeros_like(raw2)) + sp2
            if gin:
                gm = _t64(gmean[i0:i1])
                gv = _t64(gvar[i0:i1]) * vscale
                outs['o1'].append(mean)
                outs['o2'].append(vscale * var)
            else:
                N_, K_, S_ = xc.shape[:3]
                yy = _t64(y[i0:i1])[:, None, None, :].expand(N_, K_, S_, Dy).reshape(-1, Dy)
                ga = _t64(r[i0:i1])[:, :, None].expand(N_, K_, S_).reshape(-1, 1)
                df = yy - mean
                outs['A'].append((df * df / var + torch.log(var + 1e-8)).sum(-1).reshape(N_, K_, S_).sum(-1))
                gm = ga * (-2.0 * df / var)
                gv = ga * (1.0 / (var + 1e-8) - df * df / (var * var))
            dO = torch.cat([gm, gv * torch.sigmoid(raw2)], dim=1)
            dh1 = _prod_slots(dO, W2.t(), truncate) * (1.0 - h1 * h1)
            dh0 = _prod_units(dh1, W1.t(), truncate) * (1.0 - h0 * h0)
            dx = _prod_units(dh0, W0.t(), truncate) + _prod_slots(gm, Ws.t(), truncate)
            outs['dx'].append(dx.reshape(xc.shape))
            for acc, gi in zip(grads, (x2.t() @ dh0, dh0.sum(0), h0.t() @ dh1, dh1.sum(0), h1.t() @ dO, dO.sum(0), x2.t() @ gm,
                                       gm.sum(0), gv.sum(0) * torch.sigmoid(bs2))):
                acc += gi
    res = {k: torch.cat(v) for k, v in outs.items()}
    res['grads'] = grads
    return res


def relmax(got, want):
    """max |got - want| / max |want|, as relerr of test_decoder_gpu.py."""
    want = want.detach().double().cpu()
    return ((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()
