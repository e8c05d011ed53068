"""tests/svae_estep_truth.py checked on the CPU: the generic parameters have what they promise, the truth notices the bugs the init
point hides, and for every seed and shape of the GPU sweeps the oracle's fp64 and fp32 picks of the one-draw sub-sample agree
(so a device pick that differs from the fp64 oracle's is the device's doing)."""
import numpy as np
import pytest
import torch

import svae_estep_truth as T
from oracle import philox

MUT_SHAPE = (37, 5, 3, 4)


def _offdiag_ratio(M):
    """largest |off-diagonal| over largest |diagonal| entry of a (K, L, L) stack"""
    L = M.shape[-1]
    eye = torch.eye(L, dtype=torch.bool)
    return float(M[:, ~eye].abs().max() / M[:, eye].abs().max())


@pytest.mark.parametrize('K,L', [(3, 2), (5, 3), (16, 4), (7, 5), (16, 6), (33, 7), (16, 8), (10, 8), (64, 8)])
def test_generic_params_have_no_symmetry_to_hide_behind(K, L):
    p = T.generic_params(K, L, np.random.Generator(np.random.PCG64(K * 100 + L)))
    P, W = T.recognition_P(p.phi), T.theta_W(p.theta)
    assert _offdiag_ratio(P) >= 0.1 and _offdiag_ratio(W) >= 0.1, (_offdiag_ratio(P), _offdiag_ratio(W))
    assert float(torch.triu(W, 1).abs().max()) == 0.0                                      # W is the packed lower factor
    for M in (P, W, torch.as_tensor(p.phi[0]), torch.as_tensor(p.theta[2])):               # the components differ pairwise
        flat = M.reshape(K, -1)
        d = (flat[:, None, :] - flat[None, :, :]).abs().amax(-1) + torch.eye(K) * 1e9
        assert float(d.min()) > 1e-3 * float(flat.abs().max()), float(d.min())
    beta, _, _, v = T.dists.niw_natural_to_standard(*[torch.as_tensor(a) for a in p.theta[1:]])
    alpha = torch.as_tensor(p.theta[0]) + 1
    assert len(set(np.round(beta.numpy(), 9))) == K and len(set(np.round(v.numpy(), 9))) == K
    assert bool((v > L + 1).all()) and bool((alpha > 0.1).all()) and bool((alpha < 3.0).all())
    p32 = p.as_torch(torch.float32)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in p32[0] + p32[1])
    # the init point HAS the symmetry: P_k and W_k are multiples of the identity
    q = T.init_point_params(K, L, np.random.Generator(np.random.PCG64(1)))
    assert _offdiag_ratio(T.recognition_P(q.phi)) == 0.0 and _offdiag_ratio(T.theta_W(q.theta)) < 1e-12


def _case(params, shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    e1, e2, _ = T.inputs(shape, rng)
    N, K, L, S = shape
    return e1, e2, rng.standard_normal((N, K, L, S))


@pytest.mark.parametrize('name,kw,hidden_at_init', [('P_k transposed', dict(mut_unpack=T.mut_P_transposed), True),
                                                     ('P_0 <-> P_1', dict(mut_unpack=T.mut_P_swapped), True),
                                                     ('W_k off-diagonal dropped', dict(mut_W=T.mut_W_offdiag), True)])
def test_the_truth_sees_what_the_init_point_hides(name, kw, hidden_at_init):
    """Each mutation moves x, r or T' by more than 100 x that quantity's bar at generic parameters; none of them moves
    ANYTHING at the init point (P_k and W_k are one multiple of the identity for every k there) - the gap the older tests leave."""
    N, K, L, S = MUT_SHAPE
    rng = np.random.Generator(np.random.PCG64(7))
    gen, init = T.generic_params(K, L, rng), T.init_point_params(K, L, rng)
    e1, e2, noise = _case(gen, MUT_SHAPE, 11)
    t64 = T.estep_truth(gen, e1, e2, noise)
    t32 = T.estep_truth(gen, e1, e2, noise.astype(np.float32), dtype=torch.float32)
    bar, _ = T.bars(t64, t32)
    mut = T.estep_truth(gen, e1, e2, noise, **kw)
    moved = dict(x=float((mut['x'] - t64['x']).abs().max() / t64['x'].abs().max()), r=float((mut['r'] - t64['r']).abs().max()),
                 Tp=float((mut['Tp'] - t64['Tp']).abs().max() / t64['Tp'].abs().max()))
    assert any(moved[k] > 100 * bar[k] for k in bar), (name, moved, bar)
    i64 = T.estep_truth(init, e1, e2, noise)
    imut = T.estep_truth(init, e1, e2, noise, **kw)
    same = all(float((imut[k] - i64[k]).abs().max()) <= 1e-12 * float(i64[k].abs().max()) for k in ('x', 'lz', 'Tp'))
    assert same == hidden_at_init, name


def test_truth_gradients_are_the_probe_loss_gradients():
    """finite differences of the probe loss in fp64 against estep_truth's autograd gradients (one entry per input)"""
    shape = (6, 3, 2, 3)
    rng = np.random.Generator(np.random.PCG64(3))
    p = T.generic_params(3, 2, rng)
    e1, e2, wx = T.inputs(shape, rng)
    noise = rng.standard_normal((6, 3, 2, 3))

    def loss(e1_):
        t = T.estep_truth(p, e1_, e2, noise)
        return float((t['x'] * torch.as_tensor(wx)).sum() + (t['r'] * (t['Tp'] + t['lz'])).sum())
    g = T.estep_truth(p, e1, e2, noise, wx=wx)['grads']
    assert len(g) == 5
    d = np.zeros_like(e1)
    d[2, 1] = 1e-6
    fd = (loss(e1 + d) - loss(e1 - d)) / 2e-6
    assert abs(fd - float(g[0][2, 1])) <= 1e-6 * max(1.0, abs(fd))


def _pick_agreement(r64, r32, key, N):
    z64, near = T.picks(r64, key, margin=1e-5)
    z32 = T.picks(r32, key)
    if N <= 2000:
        return bool((z64 == z32).all()), 0.0
    keep = ~near
    return bool((z64[keep] == z32[keep]).all()), float(near.double().mean())


RNG_SWEEP = [(f, s, False) for f, s in T.RNG_CASES] + [(f, s, True) for f, s in T.RNG_CASES_T]


@pytest.mark.parametrize('form,shape,student', RNG_SWEEP, ids=['%s-%s-%s' % (f, 'x'.join(map(str, s)), 't' if st else 'g') for f, s, st in RNG_SWEEP])
def test_oracle_picks_agree_between_fp64_and_fp32_on_the_forward_sweep(form, shape, student):
    """the in-kernel noise here is oracle.philox.cell_noise of the case's key (the device's stream within 2e-5, tests/test_philox.py)"""
    N, K, L, S = shape
    p, e1, e2, _, seed = T.sweep_case(shape, student)
    noise = philox.cell_noise(seed, np.arange(N * K), L, 1).reshape(N, K, L, 1)             # log z does not depend on the noise
    r64 = T.estep_truth(p, e1, e2, noise)['r']
    r32 = T.estep_truth(p, e1.astype(np.float32), e2.astype(np.float32), noise.astype(np.float32), dtype=torch.float32)['r']
    ok, excluded = _pick_agreement(r64, r32, seed, N)
    assert ok and excluded <= 0.005, (shape, excluded)


@pytest.mark.parametrize('smm', [False, True])
@pytest.mark.parametrize('shape', T.DIRECT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_oracle_picks_agree_between_fp64_and_fp32_on_the_direct_step_sweep(shape, smm):
    su = T.direct_setup(shape, smm)
    lz64 = T.direct_oracle_logz(su, shape, su['model_seed'], torch.float64)
    lz32 = T.direct_oracle_logz(su, shape, su['model_seed'], torch.float32)
    z64, z32 = T.picks(torch.exp(lz64), su['model_seed']), T.picks(torch.exp(lz32.double()), su['model_seed'])
    assert bool((z64 == z32).all()), (shape, smm, (z64 != z32).nonzero())
