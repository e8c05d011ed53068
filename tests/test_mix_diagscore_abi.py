"""Host side of the diagonal mixture's scoring pass (csrc/vmp_diagscore.hip; include/vmp_hip.h "Diagonal-covariance mixture: scoring and
filling wide rows"): the exports exist and agree with the ctypes table, the size queries are host arithmetic, every argument refusal
happens before any launch (a negative code: VMP_E_BADARG = -1, VMP_E_DIM = -2, VMP_E_WS = -3; a call that reached a launch on a
machine without a GPU would return a positive HIP code), the Python layer refuses what it cannot do before it touches a device, and no
instantiation of the new kernels uses private memory."""
import ctypes
import os
import re

import pytest
import torch

import test_mix_diag_abi as A

ROOT = A.ROOT
P = A.P
BADARG, DIM, WS = -1, -2, -3
NAMES = ('vmp_mixture_diag_score_pack_words', 'vmp_mixture_diag_score_pack', 'vmp_mixture_diag_score_workspace_bytes',
         'vmp_mixture_diag_score')


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_exports_exist_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    assert 'Diagonal-covariance mixture: scoring and filling wide rows' in header
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in V._lib._SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, header), n
    assert _lib().vmp_abi_version() == 1


def test_size_queries_are_host_arithmetic():
    lib = _lib()
    for D in (1, 9, 17, 64):
        assert lib.vmp_mixture_diag_score_pack_words(D) == 3 * D + 3
    assert lib.vmp_mixture_diag_score_pack_words(0) == 0 and lib.vmp_mixture_diag_score_pack_words(65) == 0
    for D, K in ((1, 1), (16, 16), (64, 64)):
        prev = 0
        for N in (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4099, 10 ** 6, 2048 * 1024 - 1, 2048 * 1024, 2048 * 1024 + 1, 2 ** 31, 2 ** 40):
            b = lib.vmp_mixture_diag_score_workspace_bytes(N, D, K)
            assert b == 8 * min(2048, max(1, -(-N // 1024))), (N, D, K, b)   # the header's formula: one fp64 partial per block
            assert b % 8 == 0 and b >= prev
            prev = b
    for D, K in ((0, 4), (65, 4), (3, 0), (3, 65)):
        assert lib.vmp_mixture_diag_score_workspace_bytes(1000, D, K) == 0


#           x  mask N    D   K   pack logp resp x_out sum ws ws_bytes stream
SCORE_OK = [P, P, 100, 33, 16, P, P, P, P, P, P, 1 << 20, None]
IDX = dict(x=0, mask=1, N=2, D=3, K=4, pack=5, logp=6, resp=7, x_out=8, sum=9, ws=10, ws_bytes=11)


def _call(**kw):
    args = list(SCORE_OK)
    for k, v in kw.items():
        args[IDX[k]] = v
    lib = _lib()
    return lib.vmp_mixture_diag_score(*args), lib.vmp_last_error()


@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=65), DIM, b'D=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(K=65), DIM, b'K=65'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(x=None), BADARG, b'(x)'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(logp=None, resp=None, x_out=None, sum=None), BADARG, b'no output'),
    (dict(mask=None), BADARG, b'x_out needs a mask'),
    (dict(ws=ctypes.c_void_p(68)), BADARG, b'aligned'),
    (dict(ws=None), WS, b'workspace'),
    (dict(ws_bytes=4), WS, b'workspace'),
])
def test_score_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _call(**kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_diag_score' in msg and word in msg, (kw, msg)


def test_workspace_bound_is_exact_and_only_the_sum_needs_it():
    need = _lib().vmp_mixture_diag_score_workspace_bytes(10 ** 6, 33, 16)
    rc, msg = _call(N=10 ** 6, ws_bytes=need - 1)
    assert rc == WS, (rc, msg)
    # without sum_out the workspace is not looked at: the next refusal in line is reached instead
    rc, msg = _call(sum=None, ws=None, ws_bytes=0, mask=None)
    assert rc == BADARG and b'x_out needs a mask' in msg, (rc, msg)


def test_pack_builder_refuses_on_the_host():
    lib = _lib()
    ok = [33, 16, P, P, P, P, P, P, None]
    fn = lib.vmp_mixture_diag_score_pack
    for at, v in ((0, 0), (0, 65), (1, 0), (1, 65)):
        assert fn(*[v if j == at else a for j, a in enumerate(ok)]) == DIM and b'vmp_mixture_diag_score_pack' in lib.vmp_last_error(), (at, v)
    for i in range(2, 8):
        assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == BADARG
        assert b'vmp_mixture_diag_score_pack' in lib.vmp_last_error() and b'null pointer' in lib.vmp_last_error(), i


def test_python_refusals_come_before_the_device():
    """CPU tensors throughout: each call is refused for the stated reason, not for being on the CPU"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _diag, _mix, gmm
    E = V._lib.VmpError
    N, D, K = 7, 12, 3
    x, pack = torch.zeros(N, D), torch.zeros(K, 3 * D + 3)
    miss = torch.zeros(N, D, dtype=torch.bool)
    assert _mix.mixture_diag_score is _diag.mixture_diag_score and _mix.diag_score_pack is _diag.diag_score_pack
    with pytest.raises(E, match='no diagonal score pack'):
        _mix.mixture_diag_score(x, torch.zeros(K, 2 * D + 1))               # a fit pack does not do
    with pytest.raises(E, match='K=65'):
        _mix.mixture_diag_score(x, torch.zeros(65, 3 * D + 3))
    with pytest.raises(E, match='x must be'):
        _mix.mixture_diag_score(torch.zeros(N), pack)
    with pytest.raises(E, match='no output'):
        _mix.mixture_diag_score(x, pack, want_logp=False)
    with pytest.raises(E, match='want_fill needs miss'):
        _mix.mixture_diag_score(x, pack, want_fill=True)
    with pytest.raises(E, match='mask must be'):
        _mix.mixture_diag_score(x, pack, miss=miss[:3])
    with pytest.raises(E, match='inplace=True needs want_fill'):
        _mix.mixture_diag_score(x, pack, miss=miss, inplace=True)
    with pytest.raises(E, match='cpu'):
        _mix.mixture_diag_score(x, pack)
    with pytest.raises(E, match='float32'):
        _mix.mixture_diag_score(x.double(), pack)
    prior = _mix.default_diag_prior(x, K)
    with pytest.raises(E, match='b has shape'):
        _mix.diag_score_pack(prior[0], prior[1], prior[2], prior[3], prior[4][:, :2])
    with pytest.raises(E, match='cpu'):
        _mix.diag_score_pack(*prior)
    with pytest.raises(E, match='cpu'):
        gmm.predictive_logprob_diag(x, *prior)
    with pytest.raises(E, match='mask must be'):
        gmm.predictive_impute_diag(x, miss[:3], *prior)
    with pytest.raises(E, match='columns'):
        gmm.predictive_logprob_diag(torch.zeros(N, D + 1), *prior)
    with pytest.raises(E, match='cpu'):
        gmm.predictive_impute_diag(x, miss, *prior)


def test_the_old_names_still_refuse():
    """score / impute / sample of the diagonal loop keep raising with `not built` (tests/test_mix_diag_gpu.py pins it on a device);
    the messages now say where to go"""
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    loop = object.__new__(_mix.DiagLoop)                                     # the refusals look at nothing
    for name, word in (('score', 'heldout'), ('impute', 'fill'), ('sample', 'sampling'), ('impute_draws', 'sampling')):
        with pytest.raises(V._lib.VmpError, match='not built') as e:
            getattr(loop, name)()
        assert word in str(e.value)
    loop.iterations = 0
    for call in (lambda: loop.heldout(torch.zeros(3, 2)), lambda: loop.fill(torch.zeros(3, 2), None), lambda: loop.predictive_pack(),
                 lambda: loop.heldout_logprob(torch.zeros(3, 2))):
        with pytest.raises(V._lib.VmpError, match='at least one iteration'):
            call()


def test_dscore_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..64 x (masked | not)), the pack kernel and the one-wave sum: 130 kernels,
    private segment size 0 in the shipped code object (profiles/NOTES_mix_diagscore.md lists the registers)"""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    readelf = A._readelf(E.OBJDUMP)
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S*dscore_(?:pass|pack|rowsum)_kernel\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 64 * 2 + 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}


def test_the_fit_kernels_still_count_132():
    A.test_diag_kernels_use_no_scratch()
