#!/usr/bin/env python3
"""Bitwise A/B of the fit-pack and impute-pack kernels between two builds of the library.

    VMP_LIB_PATH=/path/to/libvmp_hip.so python tools/fit_family_dump.py dump OUT.npz     (on the GPU; one fresh process per build)
    python tools/fit_family_dump.py compare A.npz B.npz                                  (CPU: numpy.array_equal on the raw bits)

`dump` writes, for every shape of SHAPES on fixed seeded data with 25 % of the entries missing: fit_pack; every output of
mixture_fit_pass; every output of mixture_wfit_pass with and without a mask, and its bound-only form; mixture_bound with and without a
mask, with want_rows; mixture_impute (all four outputs) and mixture_sample (3 draws and their components) with a fixed seed.
`compare` exits 1 if an array is missing on either side or differs in dtype, shape or any bit (a NaN equals the same NaN)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, D, K): D = 1; K > 16 at odd D; the odd-D log-pivot branch with three component tiles; D = 8 at K = 16; a wave's second chunk
# and waves without rows (tests/test_mix_missfit_gpu.py::test_second_chunk_of_a_wave_and_waves_without_rows)
SHAPES = ((257, 1, 3), (65, 3, 17), (513, 5, 33), (1031, 8, 16), (270371, 3, 17))
SEED = 20240607


def dump(out):
    import torch
    if not torch.cuda.is_available():
        sys.exit('fit_family_dump.py dump needs a GPU')
    sys.path.insert(0, ROOT)
    import vmp_for_svae_amd as V
    from vmp_for_svae_amd.models import _mix
    V._lib.lib()
    arrays = {}

    def keep(tag, names, values):
        for n, v in zip(names, values):
            assert v is not None, (tag, n)
            arrays['%s/%s' % (tag, n)] = v.detach().cpu().numpy()

    for N, D, K in SHAPES:
        rng = np.random.Generator(np.random.PCG64(N * 1000 + D * 100 + K))
        f32 = lambda v: torch.as_tensor(np.asarray(v, np.float32)).cuda()
        centres = rng.standard_normal((K, D)) * 4
        x = f32(centres[rng.integers(0, K, N)] + rng.standard_normal((N, D)))
        miss = torch.as_tensor((rng.random((N, D)) < 0.25).astype(np.uint8)).cuda()
        w = f32(rng.choice(np.array([0.0, 0.25, 1.0, 3.0, 7.5]), size=N))
        A = rng.standard_normal((K, D, D))
        v = D + 2 + 5 * rng.random(K)
        C = (A @ A.transpose(0, 2, 1) / D + np.eye(D)) * v[:, None, None]          # v C^-1 of order one
        theta = [f32(t) for t in (1 + 5 * rng.random(K), 0.5 + 3 * rng.random(K), centres + 0.3 * rng.standard_normal((K, D)), C, v)]
        tag = 'N%d_D%d_K%d' % (N, D, K)
        pack = _mix.fit_pack(*theta)
        keep(tag, ('fit_pack',), (pack,))
        keep(tag + '/fit_pass', ('r', 'logr', 'x_fill', 'stats'), _mix.mixture_fit_pass(x, miss, pack, want_logr=True, want_fill=True))
        names = ('r', 'logr', 'x_fill', 'stats', 'bound')
        keep(tag + '/wfit_masked', names,
             _mix.mixture_wfit_pass(x, w, pack, miss=miss, want_logr=True, want_fill=True, want_stats=True, want_bound=True))
        full = _mix.mixture_wfit_pass(x, w, pack, want_logr=True, want_stats=True, want_bound=True)
        keep(tag + '/wfit_full', ('r', 'logr', 'stats', 'bound'), full[:2] + full[3:])
        for sub, m in (('wfit_bound_only_masked', miss), ('wfit_bound_only_full', None)):
            keep(tag + '/' + sub, ('bound',), _mix.mixture_wfit_pass(x, w, pack, miss=m, want_r=False, want_stats=False, want_bound=True)[4:])
        keep(tag + '/bound_masked', ('data', 'lse'), _mix.mixture_bound(x, miss, pack, want_rows=True))
        keep(tag + '/bound_full', ('data', 'lse'), _mix.mixture_bound(x, None, pack, want_rows=True))
        ipack = _mix.impute_pack_niw(*theta)
        keep(tag, ('impute_pack',), (ipack,))
        keep(tag + '/impute', ('x_out', 'logp', 'resp', 'sum'),
             _mix.mixture_impute(x, miss, ipack, want_x=True, want_logp=True, want_resp=True, want_sum=True))
        keep(tag + '/sample', ('x_draws', 'z'), _mix.mixture_sample(x, miss, ipack, SEED, draws=3, want_z=True))
    torch.cuda.synchronize()
    np.savez(out, **arrays)
    print('%d arrays -> %s' % (len(arrays), out))


def compare(a, b):
    with np.load(a) as fa, np.load(b) as fb:
        only = sorted(set(fa.files) ^ set(fb.files))
        differ = []
        for n in sorted(set(fa.files) & set(fb.files)):
            u, v = fa[n], fb[n]
            same = u.dtype == v.dtype and u.shape == v.shape and np.array_equal(np.ascontiguousarray(u).reshape(-1).view(np.uint8),
                                                                               np.ascontiguousarray(v).reshape(-1).view(np.uint8))
            if not same:
                differ.append(n)
        print('%d arrays compared on the raw bits: %d equal, %d differ, %d on one side only'
              % (len(set(fa.files) & set(fb.files)), len(set(fa.files) & set(fb.files)) - len(differ), len(differ), len(only)))
        for n in differ:
            print('  differs: ' + n)
        for n in only:
            print('  one side only: ' + n)
    return 1 if differ or only else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'dump':
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
