"""Conditions on the truths of tests/mix_hard_truth.py, asserted on the truth alone (no GPU): what keeps tests/test_mix_hard_gpu.py
honest.  For every case that file uses: enough rows stay soft at the posterior the compared step starts from (otherwise a comparison
of r compares zeros and ones), the conditioning and the column scales the cases are there for are reached by the FITTED posterior,
a component without rows occurs, the fp32 oracle itself stays usable (a cap: a case that breaks it is replaced by a milder one, never
given a wider bar), and each case lands in the kernel form it is meant for (vmp_mix_pass_plan: pure host)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mix_hard_truth as H  # noqa: E402
import mix_tiled_shapes as S  # noqa: E402

BOTH = [(name, fl) for name in H.LOOP_CASES for fl in H.FLAVOURS]


def test_the_generator_is_deterministic_in_its_seed():
    a, b = H.hard(300, 4, 5, 1e4, 3, 1.0, 9), H.hard(300, 4, 5, 1e4, 3, 1.0, 9)
    c = H.hard(300, 4, 5, 1e4, 3, 1.0, 10)
    assert a[0].dtype == np.float32 and a[1].dtype == np.float32
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    assert np.allclose(a[1].sum(1), 1.0, atol=1e-6)
    d = H.hard(300, 4, 5, 1e4, 3, 1.0, 9, offset=(1, 1e3))
    assert np.array_equal(np.delete(d[0], 1, 1), np.delete(a[0], 1, 1)) and np.allclose(d[0][:, 1] - a[0][:, 1], 1e3, atol=1e-3)
    e, f = H.hard_diag(200, 17, 5, 3.0, 4), H.hard_diag(200, 17, 5, 3.0, 4)
    assert np.array_equal(e[0], f[0]) and np.array_equal(e[1], f[1])


def test_the_generator_gives_the_conditioning_and_the_scales_it_states():
    x, _ = H.hard(20000, 4, 1, 1e4, 0, 1.0, 3)
    ev = np.linalg.eigvalsh(np.cov(x.astype(np.float64).T))
    assert 0.7e4 < ev[-1] / ev[0] < 1.4e4
    x3, _ = H.hard(20000, 4, 1, 1.0, 3, 1.0, 3)
    sd = x3.astype(np.float64).std(0)
    assert np.allclose(np.log10(sd / sd[0]), [0, 1, 2, 3], atol=0.05)
    xd, _ = H.hard_diag(1031, 64, 16, 3.0, 21)
    sd = xd.astype(np.float64).std(0)
    flat = np.arange(64) % 4 == 3
    assert np.log10(sd[~flat].max() / sd[~flat].min()) > 2.5                    # the columns span about three decades
    assert (sd[flat] / np.abs(xd.astype(np.float64).mean(0))[flat] < 2e-3).all()   # a quarter of them almost constant


@pytest.mark.parametrize('name,flavour', BOTH + [(H.FIT_CASE, 'gmm')])
def test_enough_rows_stay_soft(name, flavour):
    tr = H.converged(name, flavour == 'smm')
    N = tr['rT'].shape[0]
    soft = H.soft_rows(tr['rT'])
    print('%s %s: %d soft rows of %d (%.1f %%)' % (name, flavour, soft, N, 100.0 * soft / N))
    assert soft >= 40 and soft >= 0.02 * N, (name, flavour, soft, N)


@pytest.mark.parametrize('name', sorted(H.DIAG_CASES))
def test_enough_rows_stay_soft_in_the_diagonal_cases(name):
    rT = H.diag(name)[1]
    soft = H.soft_rows(rT)
    print('%s: %d soft rows of %d, %d components without rows' % (name, soft, rT.shape[0], int((rT.sum(0) < 1e-3).sum())))
    assert soft >= 40 and soft >= 0.02 * rT.shape[0], (name, soft)


def test_a_component_without_rows_occurs():
    empty = {(name, fl): int((torch.as_tensor(H.converged(name, fl == 'smm')['rT']).double().sum(0) < 1e-3).sum()) for name, fl in BOTH}
    print(empty)
    assert any(empty.values())
    assert any(n for (name, fl), n in empty.items() if fl == 'gmm') and any(n for (name, fl), n in empty.items() if fl == 'smm')


def test_the_fitted_posteriors_reach_the_conditioning():
    cond = {(name, fl): float(H.condition_numbers(H.converged(name, fl == 'smm')['theta0'][3]).max()) for name, fl in BOTH}
    print({k: '%.1e' % v for k, v in cond.items()})
    for fl in H.FLAVOURS:
        assert max(v for (name, f), v in cond.items() if f == fl) >= 1e4
    assert cond[(H.SURFACE_CASE, 'gmm')] >= 1e4 and cond[(H.AUTO_CASE, 'gmm')] >= 1e4          # what score / impute / bound are handed
    for fl in H.FLAVOURS:
        mv = H.marginal_variances(H.converged(H.AUTO_CASE, fl == 'smm')['theta0'])
        assert float(mv.max() / mv.min()) >= 1e5, (fl, mv)


@pytest.mark.parametrize('name,flavour', BOTH)
def test_the_fp32_oracle_stays_usable(name, flavour):
    tr = H.converged(name, flavour == 'smm')
    print(name, flavour, {k: '%.2e' % v for k, v in tr['e32'].items()})
    assert tr['finite32']
    assert tr['e32']['r'] <= 1e-4
    for n_ in H.NAMES:
        assert tr['e32'][n_] <= 1e-5, n_
    if flavour == 'smm':
        assert tr['e32']['u'] <= 1e-5


def test_the_other_loops_have_finite_truths_and_usable_restatements():
    for what, tr in (('masked', H.masked()[3]), ('weighted', H.weighted()[3])) + tuple((n, H.diag(n)[3]) for n in H.DIAG_CASES):
        errs = {k: v for k, v in tr.items() if k.startswith('e_')}
        print(what, {k: '%.2e' % v for k, v in errs.items()})
        assert all(np.isfinite(v) for v in errs.values()), what
        # no cap of the issue's applies to these restatements (their bars are the existing tests' max(1e-5, 3 x e), unchanged): this
        # only keeps such a bar from growing past 3e-4 unnoticed
        assert errs['e_r'] <= 1e-4 and all(v <= 1e-4 for v in errs.values()), what
    xm, _, miss, _ = H.masked()
    assert 0.25 < miss.mean() < 0.35 and miss[0].all() and not miss[1].any() and np.isnan(xm[miss != 0]).all()
    xw, _, w, tr = H.weighted()
    gone = np.isnan(xw).all(1)
    assert set(np.unique(w)) == {0.0, 1.0, 2.0, 3.0} and gone.sum() >= 50 and (w[gone] == 0).all() and (w == 0).sum() > gone.sum()
    assert torch.isfinite(tr['stats']).all() and np.isfinite(tr['bound'])


def _plan(name, flavour, mode=S.FUSED):
    import vmp_for_svae_amd as V
    c = H.CASES[name]
    return S.plan(V._lib.lib(), c['N'], c['D'], c['K'], flavour, mode)


@pytest.mark.parametrize('flavour', H.FLAVOURS)
def test_every_case_lands_in_the_kernel_form_it_is_meant_for(flavour):
    assert set(H.FORMS) == set(H.LOOP_CASES) and (H.TILED, H.XDL) == (S.TILED, S.XDL)
    for name, (form, kt_mt) in H.FORMS.items():
        p = _plan(name, flavour)
        assert (p['form'], p['kt_mt']) == (form, kt_mt), (name, flavour, p)        # kt_mt of the XDL form: terms per moment operand
    assert H.CASES['mom2_d8k16']['N'] == 65537
