"""Host side of mixture sampling (csrc/vmp_sample.hip; include/vmp_hip.h "Mixture sampling"): the export exists and agrees with the
ctypes table, every argument refusal of vmp_mixture_sample happens before any launch (a negative code: VMP_E_BADARG = -1,
VMP_E_DIM = -2; a call that reached a launch on a machine without a GPU would return a positive HIP code), the Python surface exists
and refuses wrong shapes, wrong pack widths and operands on the wrong device before it touches a device, and no instantiation of the
kernel uses private memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)          # non-NULL, never dereferenced: every call below is refused on the host
BADARG, DIM = -1, -2


def _lib():
    import vmp_for_svae_amd as V
    return V._lib.lib()


def test_the_export_exists_in_library_header_and_table():
    import vmp_for_svae_amd as V
    raw = ctypes.CDLL(V._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'vmp_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert hasattr(raw, 'vmp_mixture_sample') and 'vmp_mixture_sample' in V._lib._SIGNATURES
    assert re.search(r'\bvmp_mixture_sample\s*\(', header)


#            x  mask N    D  K   pack seed row0 draws x_out z_out stream
SAMPLE_OK = [P, P, 100, 8, 16, P, 7, 0, 2, P, P, None]


def _sample(**kw):
    idx = dict(x=0, mask=1, N=2, D=3, K=4, pack=5, seed=6, row0=7, draws=8, x_out=9, z_out=10)
    args = list(SAMPLE_OK)
    for k, v in kw.items():
        args[idx[k]] = v
    lib = _lib()
    return lib.vmp_mixture_sample(*args), lib.vmp_last_error()


@pytest.mark.parametrize('kw,code,word', [
    (dict(D=0), DIM, b'D=0'),
    (dict(D=9), DIM, b'D=9'),
    (dict(K=65), DIM, b'K=65'),
    (dict(K=0), DIM, b'K=0'),
    (dict(N=0), BADARG, b'N must be positive'),
    (dict(N=-3), BADARG, b'N must be positive'),
    (dict(draws=0), BADARG, b'draws must be positive'),
    (dict(draws=-1), BADARG, b'draws must be positive'),
    (dict(row0=-1), BADARG, b'row0'),
    (dict(x=None), BADARG, b'x is NULL'),
    (dict(mask=None), BADARG, b'mask is NULL'),
    (dict(pack=None), BADARG, b'(pack)'),
    (dict(x_out=None), BADARG, b'(x_out)'),
    (dict(x=None, mask=None, x_out=None), BADARG, b'(x_out)'),
    (dict(x=None, mask=None, z_out=None, N=0), BADARG, b'N must be positive'),      # the plain form without z_out passes the pointer checks
])
def test_sample_argument_checks_happen_on_the_host(kw, code, word):
    rc, msg = _sample(**kw)
    assert rc == code, (kw, rc, msg)
    assert b'vmp_mixture_sample' in msg and word in msg, (kw, msg)


def _theta(K, D):
    return (torch.ones(K), torch.ones(K), torch.zeros(K, D), torch.eye(D).expand(K, D, D).contiguous(), torch.full((K,), D + 2.0))


def test_the_surface_exists():
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import _mix, gmm, smm
    for mod, names in ((_mix, ('mixture_sample', 'mixture_draw')), (gmm, ('predictive_sample', 'predictive_impute_draws')),
                       (smm, ('heldout_sample', 'heldout_impute_draws')), (student_t, ('mixture_sample',)),
                       (_mix.VMPLoop, ('sample', 'impute_draws'))):
        for n in names:
            assert callable(getattr(mod, n)), (mod, n)


def test_wrappers_refuse_shapes_pack_widths_and_devices_before_a_device_is_touched():
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.distributions import student_t
    from vmp_for_svae_amd.models import _mix, gmm, smm
    E = V._lib.VmpError
    N, D, K = 7, 3, 4
    x, miss = torch.zeros(N, D), torch.zeros(N, D, dtype=torch.uint8)
    words = lambda d: 2 * d + d * (d + 1) // 2 + 5
    pack = torch.zeros(K, words(D))
    # pack widths: a score pack (D + D(D+1)/2 + 4) and a fit pack (D + D(D+1)/2 + 1) of the same D are no impute packs
    for bad in (torch.zeros(K, D + D * (D + 1) // 2 + 4), torch.zeros(K, D + D * (D + 1) // 2 + 1), torch.zeros(K, words(D) + 1),
                torch.zeros(words(D)), None):
        with pytest.raises(E, match='impute pack|impute_pack'):
            _mix.mixture_sample(x, miss, bad, 1)
        with pytest.raises(E, match='impute pack|impute_pack'):
            _mix.mixture_draw(5, bad, 1)
    # shapes
    for xb, mb in ((torch.zeros(N, D + 1), miss), (torch.zeros(N), miss), (None, miss)):
        with pytest.raises(E, match='shape|must be'):
            _mix.mixture_sample(xb, mb, pack, 1)
    # counts
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(draws=0), dict(row0=-1)):
        args = dict(seed=1, draws=1, row0=0)
        args.update(kw)
        with pytest.raises(E, match='seed|draws|row0'):
            _mix.mixture_sample(x, miss, pack, **args)
    with pytest.raises(E, match='n must be'):
        _mix.mixture_draw(0, pack, 1)
    with pytest.raises(E, match='row0'):
        _mix.mixture_draw(3, pack, 1, row0=-2)
    with pytest.raises(E, match='compiled range'):
        _mix.mixture_draw(3, torch.zeros(65, words(D)), 1)
    # well-formed operands on the CPU: refused by the operand check, nothing is evaluated in torch
    with pytest.raises(E, match='cpu'):
        _mix.mixture_sample(x, miss, pack, 1)
    with pytest.raises(E, match='cpu'):
        _mix.mixture_draw(5, pack, 1)
    al, be, m, C, v = _theta(K, D)
    kap = torch.full((K,), 5.0)
    with pytest.raises(E, match='cpu'):
        gmm.predictive_sample(5, 1, al, be, m, C, v)
    with pytest.raises(E, match='cpu'):
        gmm.predictive_impute_draws(x, miss, 2, 1, al, be, m, C, v)
    with pytest.raises(E, match='cpu'):
        smm.heldout_sample(5, 1, al, be, m, C, v, kap)
    with pytest.raises(E, match='cpu'):
        smm.heldout_impute_draws(x, miss, 2, 1, al, be, m, C, v, kap)
    with pytest.raises(E, match='cpu'):
        student_t.mixture_sample(5, 1, m, C, v, torch.zeros(K))
    # mismatched shapes in the model wrappers
    for args in ((torch.zeros(N, D + 1), miss, 2, 1, al, be, m, C, v), (x, miss[:, :2], 2, 1, al, be, m, C, v), (x, None, 2, 1, al, be, m, C, v),
                 (x, miss, 2, 1, al[:3], be, m, C, v), (x, miss, 2, 1, al, be, m, C[:, :2], v)):
        with pytest.raises(E, match='shape|must be'):
            gmm.predictive_impute_draws(*args)
        with pytest.raises(E, match='shape|must be'):
            smm.heldout_impute_draws(*args, kap)
    with pytest.raises(E, match='kappa_k has shape'):
        smm.heldout_sample(5, 1, al, be, m, C, v, kap[:2])
    with pytest.raises(E, match='shape|must be'):
        gmm.predictive_sample(5, 1, al, be[:2], m, C, v)
    with pytest.raises(E, match='shape|must be'):
        student_t.mixture_sample(5, 1, m, C[:2], v, torch.zeros(K))


def test_sample_kernels_use_no_scratch():
    """every instantiation of the streaming kernel (D = 1..8 x (K <= 16 | K > 16)): private segment size 0 in the shipped code object
    (profiles/NOTES_mix_sample.md lists the registers)"""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import erratum_scan as E
    from test_mix_impute_abi import _readelf
    readelf = _readelf(E.OBJDUMP)
    blob = open(os.path.join(ROOT, 'vmp-for-svae_amd', 'lib', 'libvmp_hip.so'), 'rb').read()
    seen = {}
    for img in E.code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'\.name:\s+(\S*13sample_kernelILi\S*).*?\.private_segment_fixed_size:\s+(\d+)', txt, re.S):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 8 * 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
