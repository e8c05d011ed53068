"""dec_bwd_kernel<UT, FS, GIN, BT> (csrc/vmp_decoder.hip) against the chunked fp64 truth of tests/decoder_truth.py at the row
counts where its tile-range arithmetic changes branch (few-tile grid <-> eight-wave grid, first two-tile waves and tile-less
blocks, even <-> a.split shares, BT = 3 <-> BT = 2 at 2^19 rows) and at every unit-tile count / bias-gradient form / epilogue
form, in decoder and in gradient-input (encoder) mode.  tests/test_decoder_truth.py proves on the CPU that each case sits on the
branch it is named for.  Errors are relative to the largest magnitude of each tensor (relerr of test_decoder_gpu.py).

Bars.  BT = 3: 1e-5 for everything (the bar of test_decoder_gpu.py).  BT = 2: the forward launch's values (always 3-term) and
the nine parameter gradients stay at 1e-5 - the claim of the BT comment at dec_bwd_kernel; the per-row quantities that are not
sums over rows (dx, and A as the backward launch's recompute writes it) get max(1e-5, 2 x the error of two_term_emulation
against the truth on the same inputs and tensor) - "no worse than twice the reference arithmetic's own error"; the bar never
comes from the kernel's output.  BT = 2 is decoder mode from 2^19 rows only: in gradient-input mode the 2-term form missed the
1e-5 parameter-gradient bar at 524 307 rows (db0 1.0e-5 .. 1.7e-5, dW1 up to 1.2e-5, db1 1.03e-5, dW0 1.06e-5), so
dec_bwd_launch now keeps that mode 3-term at every size and all its bars here are 1e-5."""
import numpy as np
import pytest
import torch

import decoder_truth as T
import parity_log

pytestmark = pytest.mark.gpu
BAR = 1e-5
_CACHE = {}                      # (kind, case) -> inputs / truth / emulation / kernel outputs, computed once and left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _seed(rows_per_cell, net):
    Ld, Dy, U = net
    return 100000 * rows_per_cell + 1000 * U + 10 * Ld + Dy             # not a function of N: runs that differ in N share rows


def dec_inputs(name, net):
    N, K, S = T.ROW_CASES[name]
    return _cached(('dec_in', name, net), lambda: T.make_inputs(N, K, S, *net, seed=_seed(K * S, net)))


def dec_truth(name, net):
    x, y, r, w = dec_inputs(name, net)
    return _cached(('dec_truth', name, net), lambda: T.truth_chunked(x, y, w, r=r))


def dec_emulation(name, net):
    x, y, r, w = dec_inputs(name, net)
    return _cached(('dec_emu', name, net), lambda: T.two_term_emulation(x, y, w, r=r))


def gin_inputs(R, net):
    return _cached(('gin_in', R, net), lambda: T.make_gin_inputs(R, *net, seed=_seed(1, net)))


def gin_truth(R, net, head):
    x, g1, g2, w = gin_inputs(R, net)
    return _cached(('gin_truth', R, net, head), lambda: T.truth_chunked(x, None, w, gmean=g1, gvar=g2, head=head))


def f32(a):
    return torch.tensor(a, dtype=torch.float32, device='cuda')


class Checks(object):
    """Every figure is printed and recorded before anything is asserted, so that one run shows all of them."""

    def __init__(self):
        self.bad = []

    def __call__(self, what, got, want, bar=BAR):
        assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
        err = parity_log.record('rel', T.relmax(got, want), tol=bar, what=what)
        print('%-44s err %.3e  bar %.3e' % (what, err, bar))
        if not err < bar:
            self.bad.append((what, err, bar))
        return err

    def done(self):
        assert not self.bad, self.bad


def two_term_bar(what, emu, truth):
    """max(1e-5, 2 x err), err = the 2-term emulation against the truth on the same tensor; recorded beside the kernel's error."""
    err = parity_log.record('rel', T.relmax(emu, truth), what='emulation ' + what)
    print('%-44s err %.3e' % ('emulation ' + what, err))
    return max(BAR, 2.0 * err)


def run_decoder(x, y, r, w):
    """Two-launch DecoderLoglikeFn: A from the (3-term) forward launch, dx and the nine parameter gradients from the backward."""
    from vmp_for_svae_amd.models import _svae_ops
    xg = f32(x).requires_grad_(True)
    wg = [f32(a).requires_grad_(True) for a in w]
    A = _svae_ops.DecoderLoglikeFn.apply(f32(y), xg, *wg)
    g = torch.autograd.grad((A * f32(r)).sum(), [xg] + wg)
    return A.detach(), g[0], list(g[1:])


def run_weighted(x, y, r, w):
    """Single-launch DecoderWeightedLoglikeFn: the value and A (= the gradient w.r.t. the weights) come out of the backward
    kernel's own recompute."""
    from vmp_for_svae_amd.models import _svae_ops
    xg, rg = f32(x).requires_grad_(True), f32(r).requires_grad_(True)
    wg = [f32(a).requires_grad_(True) for a in w]
    out = _svae_ops.DecoderWeightedLoglikeFn.apply(f32(y), xg, rg, *wg)
    g = torch.autograd.grad(out, [xg, rg] + wg)
    return out.detach(), g[1], g[0], list(g[2:])


def run_encoder(x, g1, g2, w, net, head):
    from vmp_for_svae_amd.models import vae
    Din, Dout, U = net
    vae.reset_variables()
    try:
        for n_, a in zip(T.NET_VARS, w):
            vae.VARIABLES['encoder_net/' + n_] = torch.nn.Parameter(f32(a))
        xg = f32(x).requires_grad_(True)
        e1, e2 = vae.make_encoder(xg, [(U, torch.tanh), (U, torch.tanh), (Dout, head)])
        ps = [vae.VARIABLES['encoder_net/' + n_] for n_ in T.NET_VARS]
        g = torch.autograd.grad((e1 * f32(g1)).sum() + (e2 * f32(g2)).sum(), [xg] + ps)
    finally:
        vae.reset_variables()
    return e1.detach(), e2.detach(), g[0], list(g[1:])


_ids = lambda c: '%s-%s' % (c[0], 'x'.join(str(v) for v in c[1]))


@pytest.mark.parametrize('case', T.DECODER_CASES, ids=_ids)
def test_decoder_backward_vs_fp64_truth(case):
    name, net = case
    x, y, r, w = dec_inputs(name, net)
    tr = dec_truth(name, net)
    bt2 = T.case_rows(name) >= T.DEC_BT2_ROWS
    bar_dx = two_term_bar('dx', dec_emulation(name, net)['dx'], tr['dx']) if bt2 else BAR
    bar_ll = two_term_bar('A (backward recompute)', dec_emulation(name, net)['A'], tr['A']) if bt2 else BAR
    chk = Checks()
    A, dx, gp = run_decoder(x, y, r, w)
    chk('A (forward launch)', A, tr['A'])
    chk('dx', dx, tr['dx'], bar_dx)
    for n_, g, gt in zip(T.NET_VARS, gp, tr['grads']):
        chk(n_, g, gt)
    if name == 'bt3_last' or name == 'bt2_first':
        _CACHE[('dec_dx_gpu', name, net)] = dx.cpu()
    value, A2, dx2, gp2 = run_weighted(x, y, r, w)
    chk('weighted: value', value, (tr['A'] * torch.tensor(r).double()).sum())
    chk('weighted: A (backward recompute)', A2, tr['A'], bar_ll)
    chk('weighted: dx', dx2, tr['dx'], bar_dx)
    for n_, g, gt in zip(T.NET_VARS, gp2, tr['grads']):
        chk('weighted: ' + n_, g, gt)
    chk.done()


@pytest.mark.parametrize('head', ['natparam', 'standard'])
@pytest.mark.parametrize('case', T.GIN_CASES, ids=_ids)
def test_encoder_backward_vs_fp64_truth(case, head):
    R, net = case
    x, g1, g2, w = gin_inputs(R, net)
    tr = gin_truth(R, net, head)
    assert T.bwd_variant(*net, R, gin=True)[2] == 3                          # 3-term at every size: every bar is 1e-5
    chk = Checks()
    e1, e2, dx, gp = run_encoder(x, g1, g2, w, net, head)
    chk('out1 (forward launch)', e1, tr['o1'])
    chk('out2 (forward launch)', e2, tr['o2'])
    chk('dx', dx, tr['dx'])
    for n_, g, gt in zip(T.NET_VARS, gp, tr['grads']):
        chk(n_, g, gt)
    if R in (T.case_rows('bt3_last'), T.case_rows('bt2_first')):
        _CACHE[('gin_dx_gpu', R, net, head)] = dx.cpu()
    chk.done()


def _side_by_side(what, dx3, dx2, truth3, bar2):
    """The rows the two runs share carry identical inputs: their dx must agree within the sum of the two runs' bars (relative to
    the largest |dx| of the truth) - a 2-term instance that is right on average and wrong on a lane does not."""
    n = dx3.shape[0]
    err = ((dx2[:n].double() - dx3.double()).abs().max() / truth3.abs().max()).item()
    parity_log.record('rel', err, tol=BAR + bar2, what=what)
    print('%-44s err %.3e  bar %.3e' % (what, err, BAR + bar2))
    assert err < BAR + bar2, (what, err, BAR + bar2)


def test_both_sides_of_the_two_term_threshold_agree_decoder():
    net = T.SHIPPED_NET
    dx = {}
    for name in ('bt3_last', 'bt2_first'):
        dx[name] = _cached(('dec_dx_gpu', name, net), lambda: run_decoder(*dec_inputs(name, net))[1].cpu())
    x3, x2 = dec_inputs('bt3_last', net)[0], dec_inputs('bt2_first', net)[0]
    assert np.array_equal(x3, x2[:x3.shape[0]])
    bar2 = two_term_bar('dx', dec_emulation('bt2_first', net)['dx'], dec_truth('bt2_first', net)['dx'])
    _side_by_side('dx: BT = 2 run against BT = 3 run', dx['bt3_last'], dx['bt2_first'], dec_truth('bt3_last', net)['dx'], bar2)


@pytest.mark.parametrize('head', ['natparam', 'standard'])
@pytest.mark.parametrize('net', [(8, 8, 50), (6, 6, 32)], ids=lambda n: 'x'.join(str(v) for v in n))
def test_both_sides_of_the_two_term_threshold_agree_encoder(net, head):
    R3, R2 = T.case_rows('bt3_last'), T.case_rows('bt2_first')
    dx = {}
    for R in (R3, R2):
        dx[R] = _cached(('gin_dx_gpu', R, net, head), lambda: run_encoder(*gin_inputs(R, net), net, head)[2].cpu())
    assert np.array_equal(gin_inputs(R3, net)[0], gin_inputs(R2, net)[0][:R3])
    _side_by_side('dx: 524 307-row run against 524 286-row run', dx[R3], dx[R2], gin_truth(R3, net, head)['dx'], BAR)


# ---- structure: fixed ranges -> fixed bits; every block writes its whole partial row; rows do not see their tile -----------

def _abi_backward(mode, net, x, y, r, w, fill):
    """One direct vmp_decoder_loglike_bwd / vmp_mlp_gauss_head_bwd call with a workspace of our own, filled with `fill` first
    and followed by a guard of NaN words the launch must not touch.  -> (per-row ll or None, dx, dparams, workspace words)."""
    import vmp_for_svae_amd as V
    L = V._lib
    Ld, Dy, U = net
    xg = f32(x)
    wg = [f32(a) for a in w]
    PW = L.lib().vmp_decoder_param_words(Ld, U, Dy)
    rows = xg.numel() // Ld
    nbytes = L.lib().vmp_decoder_bwd_blocks(rows) * PW * 4
    assert nbytes == (L.lib().vmp_decoder_workspace_bytes(*xg.shape[:3], Ld, U, Dy) if mode == 'decoder' else
                      L.lib().vmp_decoder_workspace_bytes(rows, 1, 1, Ld, U, Dy))
    guard = 1024
    ws = torch.full((nbytes // 4 + guard,), fill, dtype=torch.float32, device='cuda')
    ws[nbytes // 4:] = float('nan')
    dx = torch.full_like(xg, float('nan'))
    dp = torch.full((PW,), float('nan'), dtype=torch.float32, device='cuda')
    ps = [L.ptr(p) for p in wg]
    if mode == 'decoder':
        N, K, S = xg.shape[:3]
        yg, rg = f32(y), f32(r)
        ll = torch.full((N, K, S), float('nan'), dtype=torch.float32, device='cuda')
        L.check(L.lib().vmp_decoder_loglike_bwd(L.ptr(xg), L.ptr(yg), L.ptr(rg), *ps, N, K, S, Ld, Dy, U, L.ptr(dx), L.ptr(dp),
                                                L.ptr(ll), L.ptr(ws), nbytes, L.stream()), 'vmp_decoder_loglike_bwd')
    else:
        g1, g2 = f32(y), f32(r)
        ll = None
        L.check(L.lib().vmp_mlp_gauss_head_bwd(L.ptr(xg), L.ptr(g1), L.ptr(g2), -0.5, *ps, rows, Ld, Dy, U, L.ptr(dx), L.ptr(dp),
                                               L.ptr(ws), nbytes, L.stream()), 'vmp_mlp_gauss_head_bwd')
    torch.cuda.synchronize()
    return ll, dx, dp, ws, nbytes // 4


@pytest.mark.parametrize('U', [50, 64])
@pytest.mark.parametrize('mode', ['decoder', 'gin'])
def test_backward_structure_at_the_uneven_split_size(mode, U):
    """114 716 rows = 7 170 tiles: tpp = 8, 248 busy blocks (the last one short, its last tile ragged) and 8 tile-less ones.
      1. two launches on the same inputs give the same bits (static ranges: fixed summation order);
      2. the second launch starts from a workspace full of NaN: every block, the tile-less ones included, writes its whole
         PW-word partial row - the results stay finite and bit-identical, no NaN is left in the partials, the guard behind them is
         untouched;
      3. the two halves of the batch, cut at a row that is no multiple of 16, give dx (and the per-row ll) of the whole, bit for
         bit: a row's result does not depend on the tile or the wave it lands in."""
    net = (8, 8, U)
    if mode == 'decoder':
        x, y, r, w = dec_inputs('uneven_split_first', net)
        cut = 2051                                                         # 2 051 * 28 = 57 428 rows = 3 589 tiles + 4 rows
        assert (cut * 28) % 16 != 0
    else:
        R = T.case_rows('uneven_split_first')
        x, y, r, w = gin_inputs(R, net)                                    # (x, g1, g2, w)
        cut = 57431
        assert cut % 16 != 0
    p = T.bwd_tile_plan(T.case_rows('uneven_split_first'), T.bwd_split(U))
    assert p['empty_blocks'] == 8 and p['split_branch'] and p['ragged']
    ll_a, dx_a, dp_a, ws_a, n_a = _abi_backward(mode, net, x, y, r, w, 0.0)
    ll_b, dx_b, dp_b, ws_b, n_b = _abi_backward(mode, net, x, y, r, w, float('nan'))
    for t in (dx_a, dp_a) + ((ll_a,) if ll_a is not None else ()):
        assert torch.isfinite(t).all()
    assert torch.equal(dx_a, dx_b) and torch.equal(dp_a, dp_b)
    assert ll_a is None or torch.equal(ll_a, ll_b)
    assert torch.isfinite(ws_b[:n_b]).all() and torch.equal(ws_a[:n_a], ws_b[:n_b])
    assert torch.isnan(ws_b[n_b:]).all() and torch.isnan(ws_a[n_a:]).all()
    PW = n_b // p['grid']
    assert (ws_b[:n_b].reshape(p['grid'], PW)[p['busy_blocks']:] == 0).all()          # a tile-less block's partial row is zeros
    ll_1, dx_1, dp_1, _, _ = _abi_backward(mode, net, x[:cut], y[:cut], r[:cut], w, float('nan'))
    ll_2, dx_2, dp_2, _, _ = _abi_backward(mode, net, x[cut:], y[cut:], r[cut:], w, float('nan'))
    assert torch.equal(torch.cat([dx_1, dx_2]), dx_a)
    assert ll_a is None or torch.equal(torch.cat([ll_1, ll_2]), ll_a)
    scale = dp_a.abs().max()
    err = parity_log.record('rel', ((dp_1 + dp_2 - dp_a).abs().max() / scale).item(), tol=BAR, what='parameter gradients: halves against whole')
    assert err < BAR
    # the product path (autograd Functions, cached workspace) runs the same launch: same bits
    if mode == 'decoder':
        _, dx_f, gp_f = run_decoder(x, y, r, w)
        assert torch.equal(dx_f, dx_a) and torch.equal(torch.cat([g.reshape(-1) for g in gp_f]), dp_a)
    else:
        _, _, dx_f, gp_f = run_encoder(x, y, r, w, net, 'natparam')
        assert torch.equal(dx_f, dx_a) and torch.equal(torch.cat([g.reshape(-1) for g in gp_f]), dp_a)
