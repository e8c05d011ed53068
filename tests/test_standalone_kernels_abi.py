"""Host-side argument checks of the 12 stand-alone entry points of csrc/vmp_density.hip and csrc/vmp_loglike.hip
(include/vmp_hip.h): vmp_gauss_logprob_nat, vmp_gauss_logprob_nat_per_samp (+ _bwd), vmp_student_t_logprob (+ _bwd),
vmp_student_t_bwd_blocks, vmp_mix_mahalanobis, vmp_diag_gauss_loglike_fwd / _bwd, vmp_eval_cell_metrics,
vmp_bernoulli_rows_fwd / _bwd.  Every refusal below happens before any launch: the library's own refusals return a NEGATIVE
code (VMP_E_BADARG = -1, VMP_E_DIM = -2), a call that reached a launch returns 0 or hipGetLastError()'s POSITIVE code - so
`rc < 0` on a machine without a GPU is the statement "nothing was launched".  The Python wrappers' shape refusals follow;
those that validate the device first need one (marker gpu)."""
import ctypes

import pytest
import torch

P = ctypes.c_void_p(64)          # never dereferenced: every call below is refused on the host
BADARG, DIM = -1, -2


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


# name -> (argument list of a valid-looking call, required pointers, optional pointers, {dimension name: index})
#   density file: N, K, S, D checked by one helper (N, S positive; 1 <= D <= 8; 1 <= K <= 64)
#   loglike file: N, K, S, Dy positive
ENTRIES = {
    #                            x  e1 e2 lw  N   K  D  out stream
    'vmp_gauss_logprob_nat': ([P, P, P, P, 37, 5, 3, P, None], (0, 1, 2, 7), (3, 8), dict(N=4, K=5, D=6)),
    #                                     x  e1 e2  N   K  S  D  out stream
    'vmp_gauss_logprob_nat_per_samp': ([P, P, P, 37, 5, 3, 3, P, None], (0, 1, 2, 7), (8,), dict(N=3, K=4, S=5, D=6)),
    #                                         x  e1 e2 g   N   K  S  D  gx ge1 ge2 stream
    'vmp_gauss_logprob_nat_per_samp_bwd': ([P, P, P, P, 37, 5, 3, 3, P, P, P, None], (0, 1, 2, 3, 8, 9, 10), (11,),
                                           dict(N=4, K=5, S=6, D=7)),
    #                            y  mu W  cst nu  N   K  S  D  out stream
    'vmp_student_t_logprob': ([P, P, P, P, P, 37, 5, 3, 3, P, None], (0, 1, 2, 3, 4, 9), (10,), dict(N=5, K=6, S=7, D=8)),
    #                                y  mu W  nu g   N   K  S  D  gy part stream
    'vmp_student_t_logprob_bwd': ([P, P, P, P, P, 37, 5, 3, 3, P, P, None], (0, 1, 2, 3, 4, 9, 10), (11,),
                                  dict(N=5, K=6, S=7, D=8)),
    #                          x  m  P  v  beta mask N  D  K  out stream
    'vmp_mix_mahalanobis': ([P, P, P, P, P, P, 37, 3, 5, P, None], (0, 1, 2, 3, 4, 9), (5, 10), dict(N=6, D=7, K=8)),
    #                                 y  mean var N   K  S  Dy  eps  A  stream
    'vmp_diag_gauss_loglike_fwd': ([P, P, P, 37, 5, 3, 4, 1e-8, P, None], (0, 1, 2, 8), (9,), dict(N=3, K=4, S=5, Dy=6)),
    #                                 y  mean var gA  N   K  S  Dy  eps  gm gv stream
    'vmp_diag_gauss_loglike_bwd': ([P, P, P, P, 37, 5, 3, 4, 1e-8, P, P, None], (0, 1, 2, 3, 9, 10), (11,),
                                   dict(N=4, K=5, S=6, Dy=7)),
    #                            y  mean var lw per mask mm  N   K  S  Dy mse lse stream
    'vmp_eval_cell_metrics': ([P, P, P, P, 0, P, 0, 37, 5, 3, 4, P, P, None], (0, 1), (3, 5, 13), dict(N=7, K=8, S=9, Dy=10)),
    #                             y  lg mask N   K  S  D  rows stream
    'vmp_bernoulli_rows_fwd': ([P, P, P, 37, 5, 3, 40, P, None], (0, 1, 7), (2, 8), dict(N=3, K=4, S=5, Dy=6)),
    #                             y  lg mask g   N   K  S  D  gl stream
    'vmp_bernoulli_rows_bwd': ([P, P, P, P, 37, 5, 3, 40, P, None], (0, 1, 3, 8), (2, 9), dict(N=4, K=5, S=6, Dy=7)),
}
DENSITY = ('vmp_gauss_logprob_nat', 'vmp_gauss_logprob_nat_per_samp', 'vmp_gauss_logprob_nat_per_samp_bwd',
           'vmp_student_t_logprob', 'vmp_student_t_logprob_bwd', 'vmp_mix_mahalanobis')


def _bad_dims(name, dims):
    """[(index, value)]: N = 0, S = 0, K = 0 everywhere; K = 65, D = 0, D = 9 in the density file (the compiled range of its
    templates and of the K lanes of a wave; the loglike file's kernels take any K); Dy = 0 in the loglike file"""
    out = [(dims[k], 0) for k in ('N', 'S', 'K') if k in dims]
    if name in DENSITY:
        out += [(dims['K'], 65), (dims['D'], 0), (dims['D'], 9)]
    else:
        out += [(dims['Dy'], 0)]
    return out


def test_the_table_covers_the_signature_table():
    """The argument lists above are as long as the ctypes signatures, pointers where those have pointers."""
    import vmp_for_svae_amd as V
    for name, (args, req, opt, dims) in ENTRIES.items():
        res, argtypes = V._lib._SIGNATURES[name]
        assert len(args) == len(argtypes), name
        for i, (a, t) in enumerate(zip(args, argtypes)):
            assert (t is ctypes.c_void_p) == (a is P or a is None), (name, i)
        assert all(argtypes[i] is ctypes.c_void_p for i in req + opt), name
        cond = (2, 11, 12) if name == 'vmp_eval_cell_metrics' else ()     # var, mse, lse: test_eval_cell_metrics_output_rules
        assert set(req + opt + cond) == {i for i, t in enumerate(argtypes) if t is ctypes.c_void_p}, name
    assert len(ENTRIES) + 1 == 12 and 'vmp_student_t_bwd_blocks' in V._lib._SIGNATURES


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_null_required_pointer_is_refused_and_named(name):
    lib = _lib()
    args, req, opt, dims = ENTRIES[name]
    fn = getattr(lib, name)
    for i in req:
        rc = fn(*[None if j == i else a for j, a in enumerate(args)])
        assert rc == BADARG, (name, i, rc)
        assert name.encode() in lib.vmp_last_error(), (name, i, lib.vmp_last_error())


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_dimensions_outside_the_range_are_refused(name):
    lib = _lib()
    args, req, opt, dims = ENTRIES[name]
    fn = getattr(lib, name)
    for idx, v in _bad_dims(name, dims):
        rc = fn(*[v if j == idx else a for j, a in enumerate(args)])
        assert rc in (BADARG, DIM), (name, idx, v, rc)
        assert lib.vmp_last_error(), (name, idx, v)
    if name in DENSITY:                                  # the range errors carry their own code and say which range
        for key, v in (('K', 65), ('D', 9), ('D', 0)):
            rc = fn(*[v if j == dims[key] else a for j, a in enumerate(args)])
            assert rc == DIM and ('%s=%d' % (key, v)).encode() in lib.vmp_last_error(), (name, key, v)
    rc = fn(*[-5 if j == dims['N'] else a for j, a in enumerate(args)])
    assert rc == BADARG, name


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_null_optional_pointers_reach_the_dimension_check(name):
    """mask / log-weights / stream NULL and a bad dimension: the dimension error, no crash, nothing launched"""
    lib = _lib()
    args, req, opt, dims = ENTRIES[name]
    fn = getattr(lib, name)
    for idx, v in _bad_dims(name, dims):
        rc = fn(*[None if j in opt else (v if j == idx else a) for j, a in enumerate(args)])
        assert rc in (BADARG, DIM), (name, idx, v, rc)
        if name in DENSITY and v in (65, 9):
            assert rc == DIM and b'compiled range' in lib.vmp_last_error(), (name, idx, v)


def test_eval_cell_metrics_output_rules():
    lib = _lib()
    args = ENTRIES['vmp_eval_cell_metrics'][0]
    neither = [None if j in (11, 12) else a for j, a in enumerate(args)]
    assert lib.vmp_eval_cell_metrics(*neither) == BADARG and b'vmp_eval_cell_metrics' in lib.vmp_last_error()
    lse_without_var = [None if j == 2 else a for j, a in enumerate(args)]
    assert lib.vmp_eval_cell_metrics(*lse_without_var) == BADARG and b'vmp_eval_cell_metrics' in lib.vmp_last_error()
    # var NULL is fine for an mse-only call: with lse NULL too, the call gets past this rule and is refused for N = 0
    mse_only = [None if j in (2, 12) else (0 if j == 7 else a) for j, a in enumerate(args)]
    assert lib.vmp_eval_cell_metrics(*mse_only) == BADARG


@pytest.mark.parametrize('N,S,want', [(1, 1, 1), (25, 10, 1), (26, 10, 2), (16384 // 10, 10, 64), (1639, 10, 64),
                                      (10 ** 6, 10, 64), (2 ** 40, 1, 64), (2 ** 33, 2 ** 20, 64), (2 ** 62, 1, 64)])
def test_student_t_bwd_blocks_stays_in_range(N, S, want):
    """ceil(N S / 256) clipped to 1..64; the product is taken in 64 bits (2^33 * 2^20 fits them; as a 32-bit product it is 0,
    which would clip to 1)"""
    b = _lib().vmp_student_t_bwd_blocks(N, S)
    assert 1 <= b <= 64 and b == want, (N, S, b)
    assert b == max(1, min(64, (N * S + 255) // 256))


def test_student_t_logprob_wrapper_refuses_shape_mismatch():
    """checked before the device is touched: CPU tensors"""
    from vmp_for_svae_amd.distributions import student_t
    y, mu, sig, v = torch.zeros(5, 3, 2, 4), torch.zeros(3, 4), torch.eye(4).expand(3, 4, 4), torch.full((3,), 4.0)
    for bad in ((y, torch.zeros(3, 5), sig, v), (y, torch.zeros(4, 4), sig, v), (y, mu, torch.eye(4).expand(2, 4, 4), v),
                (y, mu, torch.zeros(3, 4, 5), v), (y, mu, sig, torch.full((4,), 4.0)), (y, mu, sig, torch.full((3, 1), 4.0))):
        with pytest.raises(AssertionError, match='shape mismatch'):
            student_t.log_probability_per_samp(*bad)


def test_wrappers_refuse_cpu_tensors():
    """no fall-back: the operand check names the tensor and raises before any shape is looked at"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd import losses
    from vmp_for_svae_amd.distributions import gaussian
    from vmp_for_svae_amd.models import _svae_ops, gmm
    E = V._lib.VmpError
    with pytest.raises(E):
        gaussian.log_probability_nat(torch.zeros(5, 3), torch.zeros(5, 2, 3), torch.zeros(5, 2, 3, 3))
    with pytest.raises(E):
        gaussian.log_probability_nat_per_samp(torch.zeros(5, 2, 4, 3), torch.zeros(5, 2, 3), torch.zeros(5, 2, 3, 3))
    with pytest.raises(E):
        losses._cell_metrics(torch.zeros(5, 3), torch.zeros(5, 2, 4, 3), None, None, None, True, False)
    with pytest.raises(E):
        _svae_ops.BernoulliRowsFn.apply(torch.ones(5, 3), torch.zeros(5, 2, 4, 3), None)
    with pytest.raises(E):
        _svae_ops.DiagGaussLoglikeFn.apply(torch.zeros(5, 3), torch.zeros(5, 2, 4, 3), torch.ones(5, 2, 4, 3))
    with pytest.raises(E):
        gmm.compute_expct_mahalanobis_dist(torch.zeros(5, 3), torch.ones(2), torch.zeros(2, 3), torch.eye(3).expand(2, 3, 3),
                                           torch.ones(2))


@pytest.mark.gpu
def test_gauss_logprob_nat_wrapper_refuses_a_2d_eta1():
    from vmp_for_svae_amd.distributions import gaussian
    z = lambda *s: torch.zeros(*s, device='cuda')
    with pytest.raises(AssertionError, match=r'eta1 must be of shape \(N,K,D\)'):
        gaussian.log_probability_nat(z(5, 3), z(5, 3), z(5, 2, 3, 3))
    import vmp_for_svae_amd as V
    with pytest.raises(V._lib.VmpError, match='eta2'):
        gaussian.log_probability_nat(z(5, 3), z(5, 2, 3), z(5, 2, 3))
    with pytest.raises(V._lib.VmpError, match='weights'):
        gaussian.log_probability_nat(z(5, 3), z(5, 2, 3), z(5, 2, 3, 3), weights=torch.ones(3, device='cuda'))


@pytest.mark.gpu
def test_cell_metrics_wrapper_refuses_wrong_shapes():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd import losses
    z = lambda *s: torch.zeros(*s, device='cuda')
    mean, var = z(5, 2, 4, 3), torch.ones(5, 2, 4, 3, device='cuda')
    with pytest.raises(AssertionError, match='y_true'):
        losses._cell_metrics(z(5, 4), mean, var, None, None, True, True)
    with pytest.raises(AssertionError, match='y_true'):
        losses._cell_metrics(z(6, 3), mean, var, None, None, True, True)
    with pytest.raises(AssertionError, match='mask'):
        losses._cell_metrics(z(5, 3), mean, var, None, torch.zeros(5, 4, dtype=torch.bool, device='cuda'), True, True)
    with pytest.raises(AssertionError, match='mask'):
        losses._cell_metrics(z(5, 3), mean, var, None, torch.zeros(5, dtype=torch.bool, device='cuda'), True, True)
    for bad in ((5, 3), (5, 2, 3), (5, 2, 4, 1), (2, 5)):
        with pytest.raises(AssertionError, match='log_weights'):
            losses._cell_metrics(z(5, 3), mean, var, z(*bad), None, False, True)
    with pytest.raises(V._lib.VmpError, match='var'):
        losses._cell_metrics(z(5, 3), mean, torch.ones(5, 2, 4, 2, device='cuda'), None, None, False, True)


@pytest.mark.gpu
def test_bernoulli_rows_wrapper_refuses_wrong_shapes():
    from vmp_for_svae_amd.models import _svae_ops
    y, lg = torch.ones(5, 3, device='cuda'), torch.zeros(5, 2, 4, 3, device='cuda')
    for bad in ((5, 4), (4, 3), (5, 2, 3)):
        with pytest.raises(AssertionError, match='mask'):
            _svae_ops.BernoulliRowsFn.apply(y, lg, torch.zeros(*bad, dtype=torch.bool, device='cuda'))
    with pytest.raises(AssertionError, match='y_binary'):
        _svae_ops.BernoulliRowsFn.apply(torch.ones(5, 4, device='cuda'), lg, None)
