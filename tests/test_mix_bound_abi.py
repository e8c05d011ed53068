"""Host side of the variational lower bound (csrc/vmp_bound.hip; include/vmp_hip.h "Variational lower bound"): the three exports exist
and agree with the ctypes table, the size query is host arithmetic, every argument refusal happens before any launch (a negative
code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a launch on a machine without a GPU would return a
positive HIP code), and the Python surface refuses what it cannot do before it touches a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, 8-byte aligned, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_bound_workspace_bytes', 'vmp_mixture_bound_pass', 'vmp_mixture_bound_terms')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_three_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert 'Variational lower bound' in header
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n
        assert getattr(_lib(), n).argtypes == V._lib._SIGNATURES[n][1], n


def test_workspace_bytes():
    lib = _lib()
    for D in range(0, 11):
        for K in (0, 1, 2, 16, 17, 64, 65, 100):
            b = lib.vmp_mixture_bound_workspace_bytes(1000, D, K)
            if 1 <= D <= 8 and 1 <= K <= 64:
                assert b > 0 and b % 8 == 0, (D, K, b)
            else:
                assert b == 0, (D, K, b)
    prev = 0
    for N in (1, 2, 255, 256, 257, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
        b = lib.vmp_mixture_bound_workspace_bytes(N, 8, 16)
        assert b > 0 and b % 8 == 0 and b >= prev, (N, b, prev)
        prev = b
    assert prev == lib.vmp_mixture_bound_workspace_bytes(2 ** 50, 8, 16) and prev <= 1 << 20      # one fp64 word per block of a capped grid
    assert lib.vmp_mixture_bound_workspace_bytes(10 ** 6, 3, 64) == lib.vmp_mixture_bound_workspace_bytes(10 ** 6, 8, 16)


#          x  mask N    D  K   pack lse data ws ws_bytes  stream
PASS_OK = [P, P, 100, 8, 16, P, P, P, P, 1 << 30, None]
PASS_IDX = dict(x=0, mask=1, N=2, D=3, K=4, pack=5, lse=6, data=7, ws=8, ws_bytes=9)
#           D  K   prior x 5      posterior x 5  out stream
TERMS_OK = [8, 16, P, P, P, P, P, P, P, P, P, P, P, None]


def _call(**kw):
    args = list(PASS_OK)
    for k, v in kw.items():
        args[PASS_IDX[k]] = v
    lib = _lib()
    return lib.vmp_mixture_bound_pass(*args), lib.vmp_last_error()


@pytest.mark.parametrize('mask', [P, None])
@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=9), DIM, b'D=9'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(pack=None), BADARG, b'(fit_pack)'),
    (dict(data=None), BADARG, b'(data_out)'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'aligned'),
    (dict(D=9, N=0, x=None), DIM, b'D=9'),                     # the order of the checks: dimensions, N, pointers, workspace
    (dict(N=0, x=None, ws=None), BADARG, b'N must be positive'),
    (dict(x=None, ws=None), BADARG, b'(x)'),
])
def test_pass_argument_checks_happen_on_the_host(kw, code, word, mask):
    rc, msg = _call(mask=mask, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_bound_pass' in msg and word in msg, (kw, msg)


def test_workspace_bound_is_exact():
    need = _lib().vmp_mixture_bound_workspace_bytes(10 ** 6, 8, 16)
    rc, msg = _call(N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS and b'need %d' % need in msg, (rc, msg)


def test_terms_argument_checks_happen_on_the_host():
    lib = _lib()
    fn = lib.vmp_mixture_bound_terms
    for D, K, word in ((0, 4, b'D=0'), (9, 4, b'D=9'), (3, 65, b'K=65'), (3, 0, b'K=0')):
        args = list(TERMS_OK)
        args[0], args[1] = D, K
        assert fn(*args) == DIM and word in lib.vmp_last_error() and b'vmp_mixture_bound_terms' in lib.vmp_last_error(), (D, K)
    for i in range(2, 13):
        args = list(TERMS_OK)
        args[i] = None
        assert fn(*args) == BADARG and b'vmp_mixture_bound_terms' in lib.vmp_last_error() and b'null pointer' in lib.vmp_last_error(), i


def _theta(K, D):
    return (torch.ones(K), torch.ones(K), torch.zeros(K, D), torch.eye(D).expand(K, D, D).contiguous(), torch.full((K,), D + 2.0))


def test_python_surface_refuses_shapes_before_the_device():
    """CPU tensors throughout: each call is refused for the stated reason, not for being on the CPU"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix, gmm
    E = V._lib.VmpError
    N, D, K = 7, 3, 4
    x, th = torch.zeros(N, D), _theta(K, D)
    miss = torch.zeros(N, D, dtype=torch.bool)
    for fn in (lambda x, th, **kw: _mix.lower_bound(x, th, **kw), lambda x, th, **kw: gmm.lower_bound(x, *th, **kw)):
        for i, bad in enumerate((torch.ones(3), torch.ones(K, 1), torch.zeros(K, D + 1), torch.zeros(K, D, 2), torch.ones(K, 2))):
            args = list(th)
            args[i] = bad
            with pytest.raises(E, match='shape|must be \\(K,3\\)'):
                fn(x, tuple(args))
        with pytest.raises(E, match='x must be'):
            fn(torch.zeros(N), th)
        with pytest.raises(E, match='no rows'):
            fn(torch.zeros(0, D), th)
        with pytest.raises(E, match='D=9'):
            fn(torch.zeros(N, 9), _theta(K, 9))
        with pytest.raises(E, match='K=65'):
            fn(x, _theta(65, D))
        for bad in (miss[:, :2], miss[:3], torch.zeros(N), 'mask', torch.zeros(N, D, 1)):
            with pytest.raises(E, match='mask has shape'):
                fn(x, th, miss=bad)
        with pytest.raises(E, match='mask is on meta'):
            fn(x, th, miss=torch.zeros(N, D, dtype=torch.uint8, device='meta'))
        for i, bad in enumerate((torch.ones(3), torch.ones(K, 2), torch.zeros(K, D + 1), torch.zeros(K, D, 2), torch.ones(K + 1))):
            prior = list(_mix.default_prior(K, D, 'cpu'))
            prior[i] = bad
            with pytest.raises(E, match='shape'):
                fn(x, th, prior=tuple(prior))
        # well-formed calls on CPU tensors: no CPU fallback
        with pytest.raises(E, match='cpu'):
            fn(x, th)
        with pytest.raises(E, match='cpu'):
            fn(x, th, miss=miss, prior=_mix.default_prior(K, D, 'cpu'))
    with pytest.raises(E, match='shape'):
        _mix.bound_terms(_mix.default_prior(K, D, 'cpu'), th[:3] + (torch.zeros(K, D, 1),) + th[4:])
    with pytest.raises(E, match='m_k must be'):
        _mix.bound_terms(_mix.default_prior(K, D, 'cpu'), th[:2] + (torch.zeros(K, D, 1),) + th[3:])
    with pytest.raises(E, match='cpu'):
        _mix.bound_terms(_mix.default_prior(K, D, 'cpu'), th)


def test_mixture_bound_refuses_a_pack_of_the_wrong_width_before_the_device():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    E = V._lib.VmpError
    N, D, K = 7, 3, 4
    x = torch.zeros(N, D)
    fit_words = D + D * (D + 1) // 2 + 1
    for words in (fit_words + 3, 2 * D + D * (D + 1) // 2 + 5, fit_words - 1):          # a score pack, an impute pack, one word short
        with pytest.raises(E, match='no fit pack'):
            _mix.mixture_bound(x, None, torch.zeros(K, words))
    with pytest.raises(E, match='pack must be'):
        _mix.mixture_bound(x, None, torch.zeros(K))
    with pytest.raises(E, match='mask has shape'):
        _mix.mixture_bound(x, torch.zeros(N, D + 1), torch.zeros(K, fit_words))
    with pytest.raises(E, match='cpu'):
        _mix.mixture_bound(x, None, torch.zeros(K, fit_words))
    with pytest.raises(E, match='cpu'):
        _mix.mixture_bound(x, torch.zeros(N, D, dtype=torch.uint8), torch.zeros(K, fit_words), want_rows=True)


def test_loop_refusals_come_before_the_device():
    """lower_bound() / run_until_bound() decide from the loop's flavour and iteration count alone: a loop object that owns no device
    memory at all (none can be built on the CPU) is refused for the stated reason"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    E = V._lib.VmpError
    loop = object.__new__(_mix.VMPLoop)
    loop.flavour, loop.iterations = V._lib.VMP_SMM, 3
    with pytest.raises(E, match='Gaussian mixture'):
        loop.lower_bound()
    with pytest.raises(E, match='Gaussian mixture'):
        loop.run_until_bound(1e-6)
    loop.flavour, loop.iterations = V._lib.VMP_GMM, 0
    with pytest.raises(E, match='at least one iteration'):
        loop.lower_bound()
    with pytest.raises(E, match='check_every'):
        loop.run_until_bound(1e-6, check_every=0)
