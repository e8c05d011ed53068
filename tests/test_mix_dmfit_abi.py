"""Host side of the diagonal mixture fit on partly observed and weighted rows (csrc/vmp_diagmfit.hip; include/vmp_hip.h
"Diagonal-covariance mixture: fitting partly observed and weighted rows"): the exports exist and agree with the ctypes table, the size
queries are host arithmetic, every argument refusal happens before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2,
VMP_E_WS = -3), the Python layer refuses what it cannot do before it touches a device, DiagLoop keeps refusing masks and weights, and
no instantiation of the new kernels uses private memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, 8-byte aligned, never dereferenced: every call below is refused on the host
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_diag_mfit_pack_words', 'vmp_mixture_diag_mfit_pack', 'vmp_mixture_diag_mfit_workspace_bytes',
         'vmp_mixture_diag_mfit_pass', 'vmp_mixture_diag_mfit_iterate')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert 'Diagonal-covariance mixture: fitting partly observed and weighted rows' in header
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n


def _blocks(N, D, K):
    cap = 512 if K * (1 + 3 * D) <= 2048 else 256
    return min(cap, max(1, -(-N // 2048)))


def test_size_queries_are_host_arithmetic():
    lib = _lib()
    for D in (1, 9, 17, 64):
        assert lib.vmp_mixture_diag_mfit_pack_words(D) == 3 * D + 1
    assert lib.vmp_mixture_diag_mfit_pack_words(0) == 0 and lib.vmp_mixture_diag_mfit_pack_words(65) == 0
    for D, K in ((16, 16), (33, 33), (64, 64)):
        prev = 0
        for N in (1, 63, 64, 65, 2047, 2048, 2049, 4099, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31, 2 ** 40):
            b = lib.vmp_mixture_diag_mfit_workspace_bytes(N, D, K)
            blocks = _blocks(N, D, K)
            # the fp64 moments of every wave (4 per block, the masked slab), one fp64 word per block, the pivot
            assert b == blocks * 4 * K * (1 + 3 * D) * 8 + blocks * 8 + 256, (N, D, K, b)
            assert b % 8 == 0 and b >= prev
            prev = b
        assert prev <= 120 << 20
    for D, K in ((0, 4), (65, 4), (3, 0), (3, 65)):
        assert lib.vmp_mixture_diag_mfit_workspace_bytes(1000, D, K) == 0


#          x  mask w  N    D   K   pack r  logr fill stats bound ws ws_bytes stream
PASS_OK = [P, P, P, 100, 33, 16, P, P, P, P, P, P, P, 1 << 30, None]
PASS_IDX = dict(x=0, mask=1, w=2, N=3, D=4, K=5, pack=6, r=7, logr=8, fill=9, stats=10, bound=11, ws=12, ws_bytes=13)
#          x  mask w  N    D   K   prior x 5      r  logr fill posterior x 8           pack stats bound ws ws_bytes its stream
ITER_OK = [P, P, P, 100, 33, 16, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 1 << 30, 3, None]
ITER_IDX = dict(x=0, mask=1, w=2, N=3, D=4, K=5, alpha0=6, b0=10, r=11, logr=12, fill=13, alpha=14, b=18, xbar=19, S=20, pi=21, pack=22,
                stats=23, bound=24, ws=25, ws_bytes=26, iterations=27)


def _call(name, ok, idx, **kw):
    args = list(ok)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return getattr(lib, name)(*args), lib.vmp_last_error()


COMMON = [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=65), DIM, b'D=65'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(r=None), BADARG, b'logr_out needs r_out'),
    (dict(mask=None), BADARG, b'x_fill_out needs mask'),
    (dict(ws_bytes=4), WS, b'workspace'),
    (dict(ws=None), WS, b'workspace'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'aligned'),
]


@pytest.mark.parametrize('kw,code,word', COMMON + [
    (dict(r=None, logr=None, fill=None, stats=None, bound=None), BADARG, b'no output'),
])
def test_pass_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_diag_mfit_pass', PASS_OK, PASS_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_mfit_pass' in msg and word in msg, (kw, msg)


@pytest.mark.parametrize('kw,code,word', COMMON + [
    (dict(iterations=-1), BADARG, b'iterations'),
    (dict(alpha0=None), BADARG, b'null pointer'),
    (dict(b0=None), BADARG, b'null pointer'),
    (dict(alpha=None), BADARG, b'null pointer'),
    (dict(b=None), BADARG, b'null pointer'),
    (dict(stats=None), BADARG, b'null pointer (stats)'),
])
def test_iterate_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call('vmp_mixture_diag_mfit_iterate', ITER_OK, ITER_IDX, **kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_mfit_iterate' in msg and word in msg, (kw, msg)


def test_iterate_with_zero_iterations_launches_nothing():
    rc, msg = _call('vmp_mixture_diag_mfit_iterate', ITER_OK, ITER_IDX, iterations=0)
    assert rc == 0, (rc, msg)
    rc, msg = _call('vmp_mixture_diag_mfit_iterate', ITER_OK, ITER_IDX, iterations=0, mask=None, w=None, r=None, logr=None, fill=None,
                    bound=None, xbar=None, S=None, pi=None)
    assert rc == 0, (rc, msg)


def test_workspace_bound_is_exact():
    need = _lib().vmp_mixture_diag_mfit_workspace_bytes(10 ** 6, 33, 16)
    rc, msg = _call('vmp_mixture_diag_mfit_pass', PASS_OK, PASS_IDX, N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)


def test_pack_builder_refuses_on_the_host():
    lib = _lib()
    ok = [33, 16, P, P, P, P, P, P, None]
    fn = lib.vmp_mixture_diag_mfit_pack
    for at, v in ((0, 0), (0, 65), (1, 0), (1, 65)):
        assert fn(*[v if j == at else a for j, a in enumerate(ok)]) == DIM and b'vmp_mixture_diag_mfit_pack' in lib.vmp_last_error()
    for i in range(2, 8):
        assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == BADARG and b'null pointer' in lib.vmp_last_error(), i


def test_python_refusals_come_before_the_device():
    """CPU tensors throughout: each call is refused for the stated reason, not for being on the CPU"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _diag, _mix, gmm
    E = V._lib.VmpError
    N, D, K = 7, 12, 3
    x, r0 = torch.zeros(N, D), torch.full((N, K), 1.0 / K)
    miss, w = torch.zeros(N, D, dtype=torch.bool), torch.ones(N)
    assert _mix.DiagFitLoop is _diag.DiagFitLoop and issubclass(_mix.DiagFitLoop, _mix.DiagLoop)
    assert _mix.mixture_diag_mfit_pass is _diag.mixture_diag_mfit_pass and _mix.diag_mfit_pack is _diag.diag_mfit_pack
    # the complete-row loop keeps refusing, with its words
    with pytest.raises(E, match='no masks'):
        _mix.DiagLoop(x, r0, miss=miss)
    with pytest.raises(E, match='no weights'):
        _mix.DiagLoop(x, r0, weights=w)
    with pytest.raises(E, match='DiagLoop'):
        _mix.DiagFitLoop(x, r0)
    with pytest.raises(E, match='D=65'):
        _mix.DiagFitLoop(torch.zeros(N, 65), r0, weights=w)
    with pytest.raises(E, match='K=65'):
        _mix.DiagFitLoop(x, torch.zeros(N, 65), weights=w)
    with pytest.raises(E, match='r_init has shape'):
        _mix.DiagFitLoop(x, r0[:3], weights=w)
    with pytest.raises(E, match='alpha_0 has shape'):
        _mix.DiagFitLoop(x, r0, weights=w, prior=_mix.default_diag_prior(x, K + 1))
    with pytest.raises(E, match='mask must be'):
        _mix.DiagFitLoop(x, r0, miss=miss[:, :3])
    with pytest.raises(E, match='weights have shape'):
        _mix.DiagFitLoop(x, r0, weights=w[:3])
    with pytest.raises(E, match='float32'):
        _mix.DiagFitLoop(x, r0, weights=w.double())
    with pytest.raises(E, match='finite'):
        _mix.DiagFitLoop(x, r0, weights=torch.full((N,), float('nan')))
    with pytest.raises(E, match='>= 0'):
        _mix.DiagFitLoop(x, r0, weights=-w)
    with pytest.raises(E, match='zero'):
        _mix.DiagFitLoop(x, r0, weights=0 * w)
    for kw in (dict(miss=miss), dict(weights=w), dict(miss=miss, weights=w)):
        with pytest.raises(E, match='cpu'):
            _mix.DiagFitLoop(x, r0, **kw)
    with pytest.raises(E, match='masked wide rows'):
        _mix.DiagFitLoop.from_seed(x, K, 0, weights=w, miss=miss)
    with pytest.raises(E, match='masked wide rows'):
        gmm.inference_diag_weighted(x, w, K, 0, miss=miss, init='kmeans++')
    with pytest.raises(E, match='cpu'):
        _mix.DiagFitLoop.from_seed(x, K, 0, weights=w)
    with pytest.raises(E, match='cpu'):
        gmm.inference_diag_missing(x, miss, K, 0)
    with pytest.raises(E, match='cpu'):
        gmm.inference_diag_weighted(x, w, K, 0)
    with pytest.raises(E, match='needs the missing-data mask'):
        gmm.inference_diag_missing(x, None, K, 0)
    # the pass and its pack
    pack = torch.zeros(K, 3 * D + 1)
    with pytest.raises(E, match='no masked-fit diagonal pack'):
        _mix.mixture_diag_mfit_pass(x, torch.zeros(K, 2 * D + 1), miss=miss)
    with pytest.raises(E, match='no output'):
        _mix.mixture_diag_mfit_pass(x, pack, miss=miss, want_r=False, want_stats=False)
    with pytest.raises(E, match='needs want_r'):
        _mix.mixture_diag_mfit_pass(x, pack, miss=miss, want_r=False, want_logr=True)
    with pytest.raises(E, match='want_fill needs miss'):
        _mix.mixture_diag_mfit_pass(x, pack, weights=w, want_fill=True)
    with pytest.raises(E, match='mask must be'):
        _mix.mixture_diag_mfit_pass(x, pack, miss=miss[:3])
    with pytest.raises(E, match='weights have shape'):
        _mix.mixture_diag_mfit_pass(x, pack, weights=w[:3])
    with pytest.raises(E, match='cpu'):
        _mix.mixture_diag_mfit_pass(x, pack, miss=miss, weights=w)
    prior = _mix.default_diag_prior(x, K)
    with pytest.raises(E, match='b has shape'):
        _mix.diag_mfit_pack(prior[0], prior[1], prior[2], prior[3], prior[4][:, :2])
    with pytest.raises(E, match='cpu'):
        _mix.diag_mfit_pack(*prior)
    for kw in (dict(miss=miss), dict(weights=w)):
        with pytest.raises(E, match='cpu'):
            gmm.lower_bound_diag(x, *prior, **kw)
    with pytest.raises(E, match='mask must be'):
        gmm.lower_bound_diag(x, *prior, miss=miss[:3])
    # the observed column means: dead entries are selected out, a column without an observed entry gets 0
    xm = torch.tensor([[1.0, float('nan'), 5.0], [3.0, float('nan'), float('nan')], [float('nan'), 2.0, 9.0]])
    mm = torch.tensor([[0, 1, 0], [0, 1, 1], [0, 0, 0]], dtype=torch.bool)
    p = _mix.default_diag_prior(xm, 2, miss=mm, weights=torch.tensor([1.0, 3.0, 0.0]))
    assert p[2].tolist() == [[2.5, 0.0, 5.0]] * 2


def test_dmfit_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..64 x (K <= 16 | K > 16) x (masked | not)) and the two K-sized kernels:
    private segment size 0 in the shipped code object (profiles/NOTES_mix_diagmfit.md lists the registers)"""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    from test_mix_diag_abi import _readelf
    readelf = _readelf(E.OBJDUMP)
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S*dmfit_(?:cell|gather|prep)_kernel\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 64 * 2 * 2 + 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
