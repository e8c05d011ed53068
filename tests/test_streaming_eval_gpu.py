"""Streaming test-time evaluation on the GPU (losses.streaming_metrics / streaming_imputation_losses, vmp_decoder_eval_fwd, the row
offset of the in-kernel noise) against the fp64 oracle: oracle.svae_ref.inference fed oracle.philox.cell_noise for the same cells,
then oracle.metrics.*.

The bar is not invented: the existing materialised path (svae.inference on PhiloxNoise.materialise, then losses.*) is measured against
the same oracle on the same inputs; streaming differs from it in reduction order only, so it may be off by 2x that measured error, and
not less than the 1e-5 relative of test_eval_metrics_golden.  MEASURED holds the materialised path's errors as measured on an MI355X
(every test prints both paths' figures before it asserts)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOOR = 1e-5
# materialised path vs the fp64 oracle, relative (scalars: |a-b|/|b|; tensors: max|a-b| / max|b|), measured on an MI355X
MEASURED = {
    'auto':   {'mse': 1.413e-07, 'loli': 4.753e-10, 'mse_n': 3.644e-07, 'loli_n': 1.839e-07, 'log_z': 2.553e-07, 'entropy': 1.062e-07, 'purity': 8.727e-08, 'loli_masked': 1.217e-07, 'mse_masked': 1.383e-07},
    'c5':     {'mse': 5.064e-08, 'loli': 5.589e-08, 'mse_n': 4.484e-07, 'loli_n': 1.859e-07, 'log_z': 2.337e-07, 'entropy': 6.422e-08, 'purity': 2.245e-08, 'loli_masked': 1.044e-07, 'mse_masked': 1.063e-07},
    'c5_s10': {'mse': 4.675e-08, 'loli': 3.061e-08, 'mse_n': 2.597e-07, 'loli_n': 2.359e-07, 'log_z': 2.337e-07, 'entropy': 6.422e-08, 'purity': 2.245e-08, 'loli_masked': 7.738e-08, 'mse_masked': 7.629e-08},
    'l2':     {'mse': 8.414e-09, 'loli': 4.795e-08, 'mse_n': 4.187e-07, 'loli_n': 3.395e-07, 'log_z': 2.487e-07, 'entropy': 7.418e-08, 'purity': 6.097e-09, 'loli_masked': 6.987e-08, 'mse_masked': 8.437e-08},
    'imputation': {'imp_mse': 3.113e-08, 'imp_logprob': 3.305e-09},
}
# (streaming, same run: the same figures except c5 loli 2.8e-8, c5 loli_n 2.0e-7, c5_s10 entropy
# 3.0e-8, l2 mse_masked 3.9e-9 - every entry below 4.5e-7, so every bar is the 1e-5 floor)
SHAPES = {'auto': (120, 10, 6, 50, 7, 100), 'c5': (300, 16, 8, 50, 8, 100), 'c5_s10': (300, 16, 8, 50, 8, 10), 'l2': (150, 10, 2, 50, 2, 100)}


def _bar(name, key):
    return max(2.0 * MEASURED[name][key], FLOOR)


def _rel(a, b):
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _model(N, K, Ld, U, Dy, seed=5, std=0.3):
    """Data, labels, non-trivial MLP weights (stddev 0.3: mean and var vary) and a recognition GMM, on the GPU and as fp64 copies."""
    from vmp_for_svae_amd.models import svae, vae
    from oracle import nets
    rng = np.random.Generator(np.random.PCG64(seed))
    cen = rng.standard_normal((4, Dy)) * 1.5
    lab = rng.integers(0, 4, N)
    y = (cen[lab] + 0.5 * rng.standard_normal((N, Dy))).astype(np.float32)
    w = {}
    for scope, din, dout in (('encoder_net', Dy, Ld), ('decoder_net', Ld, Dy)):
        shapes = {'layer_0/kernel': (din, U), 'layer_0/bias': (U,), 'layer_1/kernel': (U, U), 'layer_1/bias': (U,),
                  'gaussian_output/kernel': (U, 2 * dout), 'gaussian_output/bias': (2 * dout,), 'shortcut/b1': (dout,),
                  'shortcut/b2': (dout,)}
        for n_, shp in shapes.items():
            w[scope + '/' + n_] = (rng.standard_normal(shp) * std).astype(np.float32)
        w[scope + '/shortcut/W'] = nets.rand_partial_isometry(din, dout, 1., 0).astype(np.float32)
    vae.reset_variables()
    for n_, v in w.items():
        vae.VARIABLES[n_] = torch.nn.Parameter(torch.as_tensor(v).cuda())
    _, theta = svae.init_mm(K, Ld, seed=0, param_device='cuda')
    phi = [p.detach() for p in svae.init_recognition_params(theta, K, seed=0, param_device='cuda')]
    enc = [(U, torch.tanh), (U, torch.tanh), (Ld, 'natparam')]
    dec = [(U, torch.tanh), (U, torch.tanh), (Dy, 'standard')]
    T = lambda a: torch.as_tensor(a).double()
    ora = dict(y=T(y), phi=[p.double().cpu() for p in phi], enc={n_: T(w['encoder_net/' + n_]) for n_ in nets.NET_VARS},
               dec={n_: T(w['decoder_net/' + n_]) for n_ in nets.NET_VARS})
    labels = torch.nn.functional.one_hot(torch.as_tensor(lab), 4).float()
    return torch.as_tensor(y).cuda(), labels.cuda(), phi, enc, dec, ora


def _oracle_cells(ora, y_in, K, Ld, S, seed):
    """fp64: (mean, var (N,K,S,Dy), log_z (N,K)) of the oracle's inference on the Philox stream of cells n K + k"""
    from oracle import philox, svae_ref
    N = y_in.shape[0]
    noise = torch.as_tensor(philox.cell_noise(seed, np.arange(N * K), Ld, S)).double().reshape(N, K, Ld, S)
    (mean, var), _, _, _, log_z, _, _ = svae_ref.inference(y_in, ora['phi'], ora['enc'], ora['dec'], noise, torch.zeros(N, S, dtype=torch.long))
    return mean, var, log_z


def _oracle_metrics(ora, K, Ld, S, seed, labels, mask):
    from oracle import metrics
    y = ora['y']
    mean, var, log_z = _oracle_cells(ora, y, K, Ld, S, seed)
    r = torch.exp(log_z)
    sq = (y[:, None, None, :] - mean) ** 2
    lp = -0.5 * (sq / var + torch.log(var) + np.log(2 * np.pi))
    out = {'mse': metrics.weighted_mse(y, mean, r), 'loli': metrics.diagonal_gaussian_logprob(y, mean, var, log_z),
           'mse_n': (sq.sum(3).mean(2) * r).sum(1),
           'loli_n': torch.logsumexp(torch.logsumexp(lp.sum(3), dim=2) - np.log(S) + log_z, dim=1), 'log_z': log_z}
    out['entropy'], out['purity'] = metrics.purity(r, labels.double().cpu())
    m = mask.double().cpu()
    out['loli_masked'] = metrics.diagonal_gaussian_logprob(y, mean, var, log_z, mask=mask.cpu())
    out['mse_masked'] = ((sq * m[:, None, None, :]).sum(3).mean(2) * r).sum(1).mean()
    return out


def _materialised_metrics(y, labels, phi, enc, dec, K, Ld, S, seed, mask):
    from vmp_for_svae_amd import losses
    from vmp_for_svae_amd.models import svae, _svae_ops
    N = y.shape[0]
    with torch.no_grad():
        noise = _svae_ops.PhiloxNoise(seed, S).materialise(N, K, Ld, 'cuda')
        (mean, var), _, _, _, log_z, _, _ = svae.inference(y, phi, enc, dec, S, stddev_init_nn=0.3, seed=seed, noise=noise)
        r = torch.exp(log_z)
        mse_nk, lse_nk = losses._cell_metrics(y, mean, var, log_z, None, True, True)
        out = {'mse': losses.weighted_mse(y, mean, r), 'loli': losses.diagonal_gaussian_logprob(y, mean, var, log_z),
               'mse_n': (mse_nk * r).sum(1), 'loli_n': torch.logsumexp(lse_nk, dim=1), 'log_z': log_z}
        out['entropy'], out['purity'] = losses.purity(r, labels)
        out['loli_masked'] = losses.diagonal_gaussian_logprob(y, mean, var, log_z, mask=mask)
        out['mse_masked'] = losses.imputation_mse(y, mean, r, mask)
    return out


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_streaming_metrics_against_the_oracle(name):
    from vmp_for_svae_amd import losses
    N, K, Ld, U, Dy, S = SHAPES[name]
    seed = 1234
    y, labels, phi, enc, dec, ora = _model(N, K, Ld, U, Dy)
    mask = losses.generate_missing_data_mask(y, 0.25, seed=3)
    want = _oracle_metrics(ora, K, Ld, S, seed, labels, mask)
    mat = _materialised_metrics(y, labels, phi, enc, dec, K, Ld, S, seed, mask)
    kw = dict(stddev_init_nn=0.3, seed=seed, max_workspace_bytes=(N // 3 + 1) * 4 * (K * S * (2 * Ld + 2) + 2 * Ld + 6 * K))   # ~3 chunks
    got = losses.streaming_metrics(y, phi, enc, dec, S, labels=labels, **kw)
    gm = losses.streaming_metrics(y, phi, enc, dec, S, missing_data_mask=mask, mask_mse=True, **kw)
    got['loli_masked'], got['mse_masked'] = gm['loli'], gm['mse']
    assert torch.equal(gm['log_z'], got['log_z'])
    fails = []
    for key in sorted(MEASURED[name]):
        e_mat, e_str = _rel(mat[key], want[key]), _rel(got[key], want[key])
        print('%-7s %-12s materialised %.3e   streaming %.3e   bar %.3e' % (name, key, e_mat, e_str, _bar(name, key)))
        if not e_str <= _bar(name, key):
            fails.append((key, e_str, _bar(name, key)))
    assert not fails, fails


def test_streaming_imputation_against_the_oracle():
    """P = 3 perturbations (injected draws), S = 7, a 25 % mask, the C5 widths."""
    from vmp_for_svae_amd import losses
    from vmp_for_svae_amd.models import svae, _svae_ops
    from oracle import metrics
    N, K, Ld, U, Dy, S, P, seed = 200, 16, 8, 50, 8, 7, 3, 77
    y, labels, phi, enc, dec, ora = _model(N, K, Ld, U, Dy, seed=9)
    mask = losses.generate_missing_data_mask(y, 0.25, seed=1)
    pert = torch.randn(P, N, Dy, generator=torch.Generator().manual_seed(4))

    def ora_impute(y_pert):
        return _oracle_cells(ora, y_pert, K, Ld, S, seed)
    w_mse, w_ll = metrics.imputation_losses(ora['y'], mask.cpu(), ora_impute, pert.double(), S)

    def impute(y_pert):
        noise = _svae_ops.PhiloxNoise(seed, S).materialise(N, K, Ld, 'cuda')
        (mean, var), _, _, _, log_r, _, _ = svae.inference(y_pert.contiguous(), phi, enc, dec, S, stddev_init_nn=0.3, seed=seed, noise=noise)
        return mean, var, log_r
    with torch.no_grad():
        m_mse, m_ll = losses.imputation_losses(y, mask, impute, P, S, seed=seed, noise=pert.cuda())
    budget = (N // 3 + 1) * 4 * (K * S * (2 * Ld + 2) + 2 * Ld + 6 * K)
    s_mse, s_ll = losses.streaming_imputation_losses(y, mask, phi, enc, dec, P, S, stddev_init_nn=0.3, seed=seed, max_workspace_bytes=budget,
                                                     noise=pert.cuda())
    fails = []
    for key, w_, m_, s_ in (('imp_mse', w_mse, m_mse, s_mse), ('imp_logprob', w_ll, m_ll, s_ll)):
        e_mat, e_str = _rel(m_, w_), _rel(s_, w_)
        print('imputation %-12s materialised %.3e   streaming %.3e   bar %.3e' % (key, e_mat, e_str, _bar('imputation', key)))
        if not e_str <= _bar('imputation', key):
            fails.append((key, e_str))
    assert not fails, fails


@pytest.mark.parametrize('K,Ld,U,Dy,S', [(16, 8, 50, 8, 100), (10, 6, 50, 7, 10), (10, 3, 20, 5, 7)])
def test_chunk_invariance(K, Ld, U, Dy, S):
    """The same call under budgets that force 1, 3 and 7 chunks (ragged last chunk, N = 211): per-row results bit-identical."""
    from vmp_for_svae_amd import losses
    N = 211
    y, labels, phi, enc, dec, _ = _model(N, K, Ld, U, Dy, seed=2)
    in_kernel = bool(losses._rng_in_kernel(K, Ld, S))
    assert in_kernel == ((K, Ld, S) != (10, 3, 7))                     # the third shape takes the noise workspace
    per_row = losses._eval_row_bytes(K, S, Ld, Dy, in_kernel, True)
    res = []
    for chunks in (1, 3, 7):
        rows = -(-N // chunks)
        assert -(-N // rows) == chunks and N % rows != 0 or chunks == 1
        assert losses.plan_eval_chunks(N, K, S, Ld, Dy, rows * per_row) == rows
        res.append(losses.streaming_metrics(y, phi, enc, dec, S, labels=labels, stddev_init_nn=0.3, seed=11, max_workspace_bytes=rows * per_row))
    for other in res[1:]:
        for key in ('mse_n', 'loli_n', 'log_z'):
            assert torch.equal(res[0][key], other[key]), key
        assert res[0]['mse'] == other['mse'] and res[0]['loli'] == other['loli']
        for key in ('entropy', 'purity'):
            assert abs(res[0][key] - other[key]) <= 1e-6 * abs(res[0][key]), key
    assert np.isfinite([res[0][k] for k in ('mse', 'loli', 'entropy', 'purity')]).all()


def test_decoder_eval_equals_the_materialised_cell_metrics():
    """vmp_decoder_eval_fwd against vmp_decoder_loglike_fwd's (mean, var) + vmp_eval_cell_metrics on the same samples: the same
    per-row mean / var, another order of the sums over d and s (1e-5: the bar of test_eval_metrics_golden)."""
    from vmp_for_svae_amd import losses
    from vmp_for_svae_amd.models import vae, _svae_ops
    N, K, Ld, U, Dy, S = 77, 5, 5, 33, 6, 13
    y, _, _, _, dec, _ = _model(N, K, Ld, U, Dy, seed=4)
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(N, K, S, Ld, device='cuda', generator=g)
    logw = torch.log_softmax(torch.randn(N, K, device='cuda', generator=g), 1)
    mask = losses.generate_missing_data_mask(y, 0.3, seed=2)
    ps = vae.decoder_variables(Ld, dec, 0.3, 0, 'cuda')
    mean, var = _svae_ops.decoder_outputs(x, ps)
    for mk, mm in ((None, False), (mask, False), (mask, True)):
        mse0, lse0 = losses._cell_metrics(y, mean, var, logw, mk, True, True, mask_mse=mm)
        mse1, lse1 = _svae_ops.decoder_eval(x, y, ps, logw=logw, mask=mk, mask_mse=mm)
        assert _rel(mse1, mse0) < 1e-5 and _rel(lse1, lse0) < 1e-5
    only_mse, none = _svae_ops.decoder_eval(x, y, ps, want_lse=False)
    assert none is None and _rel(only_mse, losses._cell_metrics(y, mean, None, None, None, True, False)[0]) < 1e-5


@pytest.mark.parametrize('N,K,Ld,S', [(1500, 16, 8, 10), (400, 16, 8, 100), (300, 10, 3, 7)])
def test_row_offset_of_the_noise_and_the_estep(N, K, Ld, S):
    """_at(row0) == rows [row0, row0 + n) of the whole launch, bit for bit: the noise tensor (also against the oracle on the offset
    cells) and x, lz, T' of the E-step - in-kernel shapes (streaming kernels: N above the minibatch form's 256 tiles, or S > 16) and
    one noise_ws shape."""
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import svae, _svae_ops
    from oracle import philox
    seed, row0, n = 0xC0FFEE12345, 137, 101
    whole = _svae_ops.PhiloxNoise(seed, S).materialise(N, K, Ld, 'cuda')
    part = _svae_ops.PhiloxNoise(seed, S, row0=row0).materialise(n, K, Ld, 'cuda')
    assert torch.equal(part, whole[row0:row0 + n])
    cells = np.arange(row0 * K, (row0 + 8) * K)
    want = torch.as_tensor(philox.cell_noise(seed, cells, Ld, S)).reshape(8, K, Ld, S)
    assert (part[:8].double().cpu() - want).abs().max().item() < 2e-5            # v_log / v_sqrt / v_sin / v_cos vs libm (test_philox)
    assert bool(L.lib().vmp_svae_rng_in_kernel(K, Ld, S)) == ((K, Ld, S) != (10, 3, 7))
    g = torch.Generator(device='cuda').manual_seed(13)
    eta1 = torch.randn(N, Ld, device='cuda', generator=g)
    eta2d = -0.5 * torch.nn.functional.softplus(torch.randn(N, Ld, device='cuda', generator=g))
    _, theta = svae.init_mm(K, Ld, seed=0, param_device='cuda')
    phi = list(svae.init_recognition_params(theta, K, seed=0, param_device='cuda'))
    with torch.no_grad():
        xw, lzw, ptw, _ = svae.e_step((eta1, eta2d), phi, S, noise=_svae_ops.PhiloxNoise(seed, S), theta=theta)          # vmp_svae_estep_fwd_rng
        xa, lza, pta, _ = svae.e_step((eta1, eta2d), phi, S, noise=_svae_ops.PhiloxNoise(seed, S, at=True), theta=theta)  # _at, row0 = 0
        for r0, cnt in ((row0, n), (N - 33, 33), (0, 64)):
            xs, lzs, pts, _ = svae.e_step((eta1[r0:r0 + cnt].contiguous(), eta2d[r0:r0 + cnt].contiguous()), phi, S,
                                          noise=_svae_ops.PhiloxNoise(seed, S, row0=r0, at=True), theta=theta)
            assert torch.equal(xs, xw[r0:r0 + cnt]) and torch.equal(lzs, lzw[r0:r0 + cnt]) and torch.equal(pts.T_prime, ptw.T_prime[r0:r0 + cnt])
    assert torch.equal(xa, xw) and torch.equal(lza, lzw) and torch.equal(pta.T_prime, ptw.T_prime)


def test_streaming_memory_stays_within_the_budget():
    """C5, S = 100, N = 40 000 (materialised: ~8 GB, not run) under the default 256 MiB budget: the rise of the peak allocation stays
    within the budget plus the N-sized tensors - three (N,K) outputs, one (N,K) product, the (N,) vectors, the uint8 copy of no mask (0)
    - and a 2 MiB allowance for the allocator's rounding of the chunk's ~10 buffers and the K-sized tensors."""
    from vmp_for_svae_amd import losses
    N, K, Ld, U, Dy, S = 40_000, 16, 8, 50, 8, 100
    y, labels, phi, enc, dec, _ = _model(N, K, Ld, U, Dy, seed=6)
    budget = 256 << 20
    assert losses.plan_eval_chunks(N, K, S, Ld, Dy, budget) < N // 5
    losses.streaming_metrics(y[:64].contiguous(), phi, enc, dec, S, stddev_init_nn=0.3)          # module / kernel set-up outside the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = losses.streaming_metrics(y, phi, enc, dec, S, labels=labels, stddev_init_nn=0.3, max_workspace_bytes=budget)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    n_sized = 4 * N * (3 * K + 2 * K + 4) + 4 * N * Dy                  # outputs (N,K) x 3, exp / product temporaries (N,K) x 2, (N,) vectors; a y-sized slack
    print('peak rise %.1f MiB, budget %.1f MiB, N-sized allowance %.1f MiB' % (rise / 2 ** 20, budget / 2 ** 20, n_sized / 2 ** 20))
    assert rise <= budget + n_sized + (2 << 20), (rise, budget, n_sized)
    assert torch.isfinite(out['mse_n']).all() and torch.isfinite(out['loli_n']).all() and torch.isfinite(out['log_z']).all()
    assert np.isfinite([out['mse'], out['loli'], out['entropy'], out['purity']]).all()


def test_driver_streaming_mode():
    """experiments.run(eval_mode='streaming'): same history keys; purity / entropy (functions of log z alone, not of the noise) equal
    to the default mode's; the trained parameters bit-identical (evaluation does not touch the trainer); evaluate_imputation(streaming)
    finite and positive on the trained model."""
    from vmp_for_svae_amd import experiments, losses
    cfg = {'dataset': 'pinwheel', 'method': 'svae-cvi', 'lr': 0.01, 'lrcvi': 0.1, 'K': 10, 'L': 2, 'U': 50, 'seed': 0}
    res = {}
    for mode in ('materialised', 'streaming'):
        tr, hist, _ = experiments.run(cfg, nb_iters=21, measurement_freq=10, verbose=False, eval_mode=mode, imputation_freq=20,
                                      nb_samples_pert=3, nb_samples_te=20, max_workspace_bytes=1 << 18)     # 150 test rows: two chunks
        res[mode] = (hist, [p.detach().clone() for p in tr.trainables()[1]] + [t.clone() for t in tr.theta], tr)
    (h0, p0, _), (h1, p1, tr) = res['materialised'], res['streaming']
    assert len(h0) == len(h1) and [sorted(a) for a in h0] == [sorted(b) for b in h1]
    assert 'imp_mse' in h1[0] and 'purity' in h1[0]
    for a, b in zip(h0, h1):
        assert np.isfinite(list(b.values())).all()
        assert abs(a['purity'] - b['purity']) <= 1e-6 and abs(a['entropy'] - b['entropy']) <= 1e-6
        assert a['neg_normed_elbo'] == b['neg_normed_elbo']
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    from vmp_for_svae_amd import data as data_mod
    X, lab = data_mod.load_dataset('pinwheel', None)
    _, _, X_te, _ = data_mod.split_and_scale('pinwheel', X, lab, ratio_tr=0.7, seed_split=0, noise_level=0.1)
    Xte = torch.as_tensor(X_te).cuda()
    mask = losses.generate_missing_data_mask(Xte, 0.25, seed=0)
    imp = experiments.evaluate_imputation(tr, Xte, mask, nb_samples_pert=4, nb_samples_te=20, streaming=True, max_workspace_bytes=1 << 20)
    assert np.isfinite(imp['imp_mse']) and imp['imp_mse'] > 0 and np.isfinite(imp['imp_logprob'])
    with pytest.raises(ValueError):
        experiments.run(cfg, nb_iters=1, eval_mode='lazy', verbose=False)


def test_unfused_standard_decoder_streams_per_chunk():
    """A 'standard' decoder outside the fused kernels' range (U = 100) runs the materialised computation per chunk (torch MLP +
    vmp_eval_cell_metrics) under the same budget, the MLP's hidden activations counted.  Against the materialised path on the same
    Philox stream and between 1 / 3 / 7 chunks: 1e-5 relative (the floor of the oracle tests) - not bit for bit, torch's GEMM may pick
    another kernel for another row count; log z comes from the fused encoder and the E-step and IS bit-identical.  The peak allocation
    stays within the budget plus the N-sized tensors."""
    from vmp_for_svae_amd import losses
    from vmp_for_svae_amd.models import svae, vae, _svae_ops
    N, K, Ld, U, Dy, S, seed = 211, 6, 4, 100, 5, 12, 21
    y, labels, phi, enc, dec, _ = _model(N, K, Ld, 50, Dy, seed=8)
    dec = [(U, torch.tanh), (U, torch.tanh), (Dy, 'standard')]
    assert not vae.fused_decoder_eligible(Ld, dec)
    with torch.no_grad():
        for n_ in [n_ for n_ in vae.VARIABLES if n_.startswith('decoder_net/')]:
            del vae.VARIABLES[n_]
        vae.make_decoder(torch.zeros(1, 1, 1, Ld, device='cuda'), layerspecs=dec, stddev_init=0.3, seed=3)       # creates the U = 100 variables
        noise = _svae_ops.PhiloxNoise(seed, S).materialise(N, K, Ld, 'cuda')
        (mean, var), _, _, _, log_z, _, _ = svae.inference(y, phi, enc, dec, S, stddev_init_nn=0.3, seed=seed, noise=noise)
        mse_nk, lse_nk = losses._cell_metrics(y, mean, var, log_z, None, True, True)
        want = {'mse_n': (mse_nk * torch.exp(log_z)).sum(1), 'loli_n': torch.logsumexp(lse_nk, dim=1), 'log_z': log_z}
    assert mean.std().item() > 0.05 and var.std().item() > 1e-3
    per_row = losses._eval_row_bytes(K, S, Ld, Dy, True, False, hidden=(U, U))
    assert per_row > 4 * K * S * 3 * U
    res = []
    for chunks in (1, 3, 7):
        rows = -(-N // chunks)
        budget = rows * per_row
        assert losses.plan_eval_chunks(N, K, S, Ld, Dy, budget, fused=False, hidden=(U, U)) == rows
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = losses.streaming_metrics(y, phi, enc, dec, S, labels=labels, stddev_init_nn=0.3, seed=seed, max_workspace_bytes=budget)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        n_sized = 4 * N * (5 * K + 4 + Dy)
        print('unfused, %d chunk(s): peak rise %.2f MiB, budget %.2f MiB' % (chunks, rise / 2 ** 20, budget / 2 ** 20))
        assert rise <= budget + n_sized + (2 << 20), (chunks, rise, budget)
        res.append(out)
        assert torch.equal(out['log_z'], want['log_z'])
        for key in ('mse_n', 'loli_n'):
            assert _rel(out[key], want[key]) < 1e-5, (chunks, key, _rel(out[key], want[key]))
    for other in res[1:]:
        for key in ('mse_n', 'loli_n'):
            assert _rel(other[key], res[0][key]) < 1e-5
        assert abs(other['purity'] - res[0]['purity']) <= 1e-6 * abs(res[0]['purity'])
