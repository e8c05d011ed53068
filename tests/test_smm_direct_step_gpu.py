"""The six-launch direct minibatch step of the Student-t mixture SVAE (SVAETrainer(smm=True); BASELINE config 5's model,
experiments.py:154-176, 196-267): launch 1 packs the Student-t theta (vmp_mlp_gauss_head_fwd_prep_smm), launch 4 writes the theta
half of the partial rows (vmp_svae_estep_bwd_tail_t), launch 6 differentiates the packing, runs Adam on the 23 tensors and the N_k-only
M-step + CVI of alpha (vmp_svae_step_final_smm / vmp_svae_step_pack_smm).  Checked against the autograd SMM step (direct_step=False),
against itself replayed from HIP graphs (one and four steps per replay, experiments.run) and in a two-rank data-parallel step."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
C5 = (64, 16, 8, 50, 8, 10)                          # (N, K, L, U, Dy, S): experiments.py:26, 154-176
SHAPES = [C5, (64, 10, 8, 50, 6, 16), (512, 8, 6, 50, 6, 10), (40, 20, 4, 32, 4, 6), (30, 33, 2, 16, 2, 4), (8, 64, 8, 64, 8, 10),
          (1, 1, 1, 1, 1, 4)]


def _trainer(N, K, Ld, U, Dy, S, **kw):
    from vmp_for_svae_amd.models import vae
    from vmp_for_svae_amd.training import SVAETrainer
    vae.reset_variables()
    return SVAETrainer(K, Ld, U, Dy, nb_samples=S, lr=3e-3, lrcvi=0.2, decay_rate=0.95, stddev_init_nn=0.1, seed=3, smm=True, dof=5.0, **kw)


def _minibatches(N, Dy, n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [torch.randn(N, Dy, device='cuda', generator=g) * 2 for _ in range(n)]


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize('N,K,Ld,U,Dy,S', [C5] + SHAPES[1:])
def test_smm_trainer_takes_the_direct_step(N, K, Ld, U, Dy, S):
    """The direct step covers the SMM trainer under the GMM trainer's conditions, and nothing else changes its answer."""
    y = torch.randn(N, Dy, device='cuda')
    tr = _trainer(N, K, Ld, U, Dy, S)
    assert tr._direct_ok(y, None, None, None, None)
    assert not tr._direct_ok(y, torch.zeros(N, K, Ld, S, device='cuda'), None, None, None)          # injected noise
    assert not tr._direct_ok(y, None, torch.zeros(N, S, dtype=torch.int64, device='cuda'), None, None)
    assert not _trainer(N, K, Ld, U, Dy, S, direct_step=False)._direct_ok(y, None, None, None, None)
    assert not _trainer(N, K, Ld, U, Dy, S, rng='torch')._direct_ok(y, None, None, None, None)
    assert not tr._direct_ok(torch.randn(513, Dy, device='cuda'), None, None, None, None)


@pytest.mark.parametrize('N,K,Ld,U,Dy,S', SHAPES)
def test_smm_direct_step_equals_the_autograd_step(N, K, Ld, U, Dy, S):
    """4 direct steps against 4 autograd steps from the same seed: step 1's log z, samples and sub-sample bit-identical (they do
    not depend on theta); ELBO scalars to 2e-5, the 23 gradients, alpha*, parameters, alpha and Adam slots to 1e-4 of each
    tensor's max-abs (the Student-t theta packing moves from torch to the kernel: other roundings)."""
    ys = _minibatches(N, Dy, 4, N + K)

    def run(direct):
        tr = _trainer(N, K, Ld, U, Dy, S, direct_step=direct)
        assert tr._direct_ok(ys[0], None, None, None, None) == direct
        outs = []
        for y in ys:
            o = tr.step(y)
            outs.append(dict(elbo=[float(o[k]) for k in ('elbo', 'neg_rec_err', 'regulariser')],
                             grads={k: v.detach().clone() for k, v in o['grads'].items()}, star=[t.clone() for t in o['theta_star']],
                             log_z=o['log_z'].clone(), x_k=o['x_k'].clone(), xs=o['x_samples'].clone()))
        assert tr.global_step == 4 and tr.opt.t == 4
        names = tr.trainables()[0]
        state = [p.detach().clone() for p in tr.trainables()[1]] + [tr.theta[0].clone()] + [t.clone() for t in tr.opt.m] + \
                [t.clone() for t in tr.opt.v]
        return names, outs, state
    names_a, want_o, want_s = run(False)
    names_d, got_o, got_s = run(True)
    assert names_d == names_a and len(names_d) == 23
    assert torch.equal(got_o[0]['log_z'], want_o[0]['log_z'])
    assert torch.equal(got_o[0]['x_k'], want_o[0]['x_k'])
    assert torch.equal(got_o[0]['xs'], want_o[0]['xs'])
    for i, (a, b) in enumerate(zip(got_o, want_o)):
        scale = max(abs(b['elbo'][1]), abs(b['elbo'][2]))
        for x, y_ in zip(a['elbo'], b['elbo']):
            assert abs(x - y_) <= 2e-5 * scale, (i, a['elbo'], b['elbo'])
        assert sorted(a['grads']) == sorted(b['grads'])
        for k in b['grads']:
            assert _rel(a['grads'][k], b['grads'][k]) <= 1e-4, (i, k, _rel(a['grads'][k], b['grads'][k]))
        assert len(a['star']) == len(b['star']) == 1 and _rel(a['star'][0], b['star'][0]) <= 1e-4
    # parameters: 1e-4 of max-abs - except elements whose gradient is NEAR ZERO (Adam RMS sqrt(v) below 1 % of the tensor's largest):
    # Adam divides every gradient element by its own RMS, so the rounding difference of such an element (within the 1e-4 max-abs
    # gradient bar above) reaches the parameter at the scale of lr, not of the gradient.  Those elements get 1 % of the Adam movement
    # of 4 steps (4 lr); seen: phi_gmm/log_pi_k at K = 64, N = 8 (8 rows over 64 components) differed by 1.2e-5 = 4e-3 lr.
    npar = len(names_d)
    for j, (a, b) in enumerate(zip(got_s, want_s)):
        if j < npar:
            rms = want_s[2 * npar + 1 + j].double().sqrt()                 # Adam v of parameter j (autograd run)
            tiny = rms < 1e-2 * rms.max()
            bar = torch.where(tiny, torch.full_like(rms, 1e-2 * 4 * 3e-3), torch.full_like(rms, 1e-4 * b.abs().max().item()))
            d = (a.double() - b.double()).abs()
            assert bool((d <= bar).all()), (j, names_d[j], _rel(a, b), int((d > bar).sum()))
        else:
            assert _rel(a, b) <= 1e-4, (j, _rel(a, b))


def test_smm_direct_step_vs_fp64_oracle():
    """One direct SMM step at the C5 minibatch against the oracle's literal restatement of experiments.py:196-267 for the Student-t model
    (oracle.train_ref.train_step(State(..., smm=True))), fed the device's own draws: the in-kernel Philox noise of the step's key
    (oracle.philox.cell_noise) and the categorical picks the oracle forms from ITS r by inverse CDF of the same uniforms
    (oracle.philox.subsample_uniforms) - which must equal the device's picks.  ELBO, the 23 gradients, alpha after the CVI update and
    the 23 parameters after Adam, each to max(1e-5, 3 |oracle fp64 - oracle fp32|) of its max-abs (the golden tests' clause)."""
    from oracle import philox, svae_ref, train_ref
    N, K, Ld, U, Dy, S = C5
    rng = np.random.Generator(np.random.PCG64(55))
    tr = _trainer(*C5)
    with torch.no_grad():                                   # the reference starts every Student-t component at the prior mean:
        tr.theta[1].add_(torch.as_tensor(rng.standard_normal((K, Ld)) * 1.5, dtype=torch.float32).cuda())        # spread them out
        tr.theta[2].add_(torch.as_tensor(np.tril(rng.standard_normal((K, Ld, Ld)) * 0.3), dtype=torch.float32).cuda())
        tr.phi_gmm[1].add_(torch.as_tensor(np.tril(rng.standard_normal((K, Ld, Ld)) * 0.2, -1), dtype=torch.float32).cuda())
    c = rng.standard_normal((K, Dy)) * 2.0
    y = torch.as_tensor((c[rng.integers(0, K, N)] + 0.5 * rng.standard_normal((N, Dy))).astype(np.float32)).cuda()
    names, params = tr.trainables()
    init = dict(zip(names, [p.detach().cpu().double() for p in params]))
    theta0 = [t.cpu().double() for t in tr.theta]
    prior0 = tr.gmm_prior.cpu().double()
    seed = tr._step_seed_at(0) & 0xFFFFFFFFFFFFFFFF
    assert tr._direct_ok(y, None, None, None, None)
    out = tr.step(y)
    torch.cuda.synchronize()
    noise = torch.as_tensor(philox.cell_noise(seed, np.arange(N * K), Ld, S)).reshape(N, K, Ld, S)
    u = torch.as_tensor(philox.subsample_uniforms(seed, N, 1)[:, 0]).double()
    # the device's picks: the component whose first sample x_samples[n] is
    xk, xs = out['x_k'].cpu(), out['x_samples'].cpu()
    hit = (xk[:, :, 0, :] == xs[:, None, :]).all(-1)
    assert bool((hit.sum(1) >= 1).all())
    z_dev = hit.float().argmax(1)
    nets_w = lambda scope, dt: {v: init[scope + '/' + v].to(dt) for v in ('layer_0/kernel', 'layer_0/bias', 'layer_1/kernel', 'layer_1/bias',
                                                                            'gaussian_output/kernel', 'gaussian_output/bias', 'shortcut/W',
                                                                            'shortcut/b1', 'shortcut/b2')}

    def oracle(dt):
        phi = [init['phi_gmm/' + n_].to(dt) for n_ in ('mu_k', 'L_k', 'log_pi_k')]
        theta = [theta0[0].to(dt), init['theta/mu_k'].to(dt), init['theta/L_k'].to(dt), theta0[3].to(dt)]
        enc, dec = nets_w('encoder_net', dt), nets_w('decoder_net', dt)
        yo, no = y.cpu().to(dt), noise.to(dt)
        with torch.no_grad():                               # the oracle's r -> its picks (inverse CDF of the device's uniforms)
            lz = svae_ref.inference(yo, phi, enc, dec, no, torch.zeros(N, S, dtype=torch.int64))[4]
        cdf = torch.cumsum(torch.exp(lz.double()), dim=1)
        z = (cdf[:, :K - 1] <= u[:, None]).sum(1)
        st = train_ref.State(phi, enc, dec, theta, prior0.to(dt), smm=True)
        ref = train_ref.train_step(st, yo, no, z[:, None].expand(N, S).contiguous(), tr.lr, tr.lrcvi0, tr.decay_rate)
        ns, ps = st.trainables()
        return z, ref, dict(zip(ns, [p.detach().double() for p in ps])), st.theta[0].double()
    z64, ref64, par64, a64 = oracle(torch.float64)
    z32, ref32, par32, a32 = oracle(torch.float32)
    assert torch.equal(z64, z_dev), (z64 != z_dev).nonzero()

    def check(what, got, want64, want32):
        got, want64, want32 = [torch.as_tensor(t).double().cpu() for t in (got, want64, want32)]
        scale = want64.abs().max().clamp_min(1e-300)
        bar = max(1e-5, 3 * ((want64 - want32).abs().max() / scale).item())
        err = ((got - want64).abs().max() / scale).item()
        assert err <= bar, (what, err, bar)
    check('elbo', out['elbo'], ref64['elbo'], ref32['elbo'])
    assert len(ref64['grads']) == 23 and sorted(ref64['grads']) == sorted(out['grads'])
    for n_ in ref64['grads']:
        check('grad ' + n_, out['grads'][n_], ref64['grads'][n_], ref32['grads'][n_])
    check('alpha*', out['theta_star'][0], ref64['theta_star'][0], ref32['theta_star'][0])
    check('alpha after CVI', tr.theta[0], a64, a32)
    for n_, p in zip(*tr.trainables()):
        check('param ' + n_, p.detach(), par64[n_], par32[n_])


def _direct_shapes():
    import svae_estep_truth as T
    return T.DIRECT_SHAPES


@pytest.mark.parametrize('smm', [False, True], ids=['gmm', 'smm'])
@pytest.mark.parametrize('shape', _direct_shapes(), ids=lambda s: 'x'.join(map(str, s)))
def test_direct_step_vs_fp64_oracle_at_generic_parameters(shape, smm):
    """The comparison above over the minibatch shapes, for the Gaussian (vmp_svae_estep_bwd_tail: its first fp64 truth) and the
    Student-t model, with theta and phi_gmm moved to generic values first (svae_estep_truth.generic_params: no component is a multiple
    of the identity, no two are alike) - the Student-t theta set to generic values rather than perturbed, so that every input is
    known on the CPU, where tests/test_svae_estep_truth.py checks that the oracle's fp64 and fp32 picks agree for these seeds.
    ELBO, every gradient, theta* and theta after CVI, the parameters after Adam: max(1e-5, 3 |oracle fp64 - oracle fp32|) of max-abs;
    parameters whose gradient element is near zero by the Adam-RMS rule of test_smm_direct_step_equals_the_autograd_step."""
    import ctypes
    import svae_estep_truth as T
    import parity_log
    from oracle import philox, svae_ref, train_ref
    from vmp_for_svae_amd import _lib as L
    from vmp_for_svae_amd.models import vae
    from vmp_for_svae_amd.training import SVAETrainer
    N, K, Ld, U, Dy, S = shape
    out8 = (ctypes.c_int64 * 8)()
    L.check(L.lib().vmp_svae_launch_plan(0, N, K, Ld, S, 1, 1, 0, 1, out8), 'vmp_svae_launch_plan')
    assert T.FWD_FORMS[out8[0]] == 'fwd1'
    L.check(L.lib().vmp_svae_launch_plan(1, N, K, Ld, S, int(smm), 1, 0, 0, out8), 'vmp_svae_launch_plan')
    assert out8[2] == 1                                       # the backward with the ELBO tail inside covers the shape
    su = T.direct_setup(shape, smm)
    lr, lrcvi, decay = 3e-3, 0.2, 0.95
    vae.reset_variables()
    for n_, v in su['w'].items():
        vae.VARIABLES[n_] = torch.nn.Parameter(torch.as_tensor(v).cuda())
    tr = SVAETrainer(K, Ld, U, Dy, nb_samples=S, lr=lr, lrcvi=lrcvi, decay_rate=decay, seed=su['model_seed'], smm=smm, dof=5.0,
                     m_uniform=torch.as_tensor(su['m_unif']).cuda(), pi_normal=torch.as_tensor(su['pi_norm']).cuda())
    phi32, th32 = su['params'].as_torch(torch.float32)
    with torch.no_grad():
        for p, v in zip(tr.phi_gmm, phi32):
            p.copy_(v.cuda())
        for t, v in zip(tr.theta, th32):
            t.copy_(v.cuda())
    y = torch.as_tensor(su['y']).cuda()
    names, params = tr.trainables()
    init = dict(zip(names, [p.detach().cpu().double() for p in params]))
    for n_, v in su['w'].items():
        assert torch.equal(init[n_].float(), torch.as_tensor(v)), n_
    theta0 = [t.detach().cpu().double() for t in tr.theta]
    prior0 = [p.cpu().double() for p in tr.gmm_prior] if not smm else tr.gmm_prior.cpu().double()
    seed = tr._step_seed_at(0) & 0xFFFFFFFFFFFFFFFF
    assert seed == su['model_seed'] and tr._direct_ok(y, None, None, None, None)
    out = tr.step(y)
    torch.cuda.synchronize()
    noise = torch.as_tensor(philox.cell_noise(seed, np.arange(N * K), Ld, S)).reshape(N, K, Ld, S)
    xk, xs = out['x_k'].cpu(), out['x_samples'].cpu()
    hit = (xk[:, :, 0, :] == xs[:, None, :]).all(-1)
    assert bool((hit.sum(1) >= 1).all())

    def oracle(dt):
        phi = [init['phi_gmm/' + n_].to(dt) for n_ in ('mu_k', 'L_k', 'log_pi_k')]
        theta = [t.to(dt) for t in theta0]
        enc = {v: init['encoder_net/' + v].to(dt) for v in T.NET_VARS}
        dec = {v: init['decoder_net/' + v].to(dt) for v in T.NET_VARS}
        yo, no = y.cpu().to(dt), noise.to(dt)
        lz = T.direct_oracle_logz(su, shape, seed, dt)
        z = T.picks(torch.exp(lz.double()), seed)
        pri = prior0.to(dt) if smm else [p.to(dt) for p in prior0]
        st = train_ref.State(phi, enc, dec, theta, pri, smm=smm)
        ref = train_ref.train_step(st, yo, no, z[:, None].expand(N, S).contiguous(), lr, lrcvi, decay)
        ns, ps = st.trainables()
        return z, ref, dict(zip(ns, [p.detach().double() for p in ps])), [t.detach().double() for t in st.theta]
    z64, ref64, par64, th64 = oracle(torch.float64)
    z32, ref32, par32, th32_ = oracle(torch.float32)
    assert torch.equal(z64, z32)
    assert bool(hit[torch.arange(N), z64].all()), (~hit[torch.arange(N), z64]).nonzero()       # the device's picks are the oracle's
    tag = '%s direct %s' % ('smm' if smm else 'gmm', shape)

    def check(what, got, want64, want32, tiny=None):
        got, want64, want32 = [torch.as_tensor(t).detach().double().cpu() for t in (got, want64, want32)]
        scale = want64.abs().max().clamp_min(1e-300)
        o32 = ((want64 - want32).abs().max() / scale).item()
        bar = max(1e-5, 3 * o32)
        d = (got - want64).abs()
        if tiny is not None and bool(tiny.any()):
            # elements whose gradient is near zero: Adam divides by their own RMS, so their rounding reaches the parameter at the scale
            # of lr - they may meet 1 % of the Adam movement of the step INSTEAD of the clause (whichever allows more: at generic
            # parameters most components hold no mass, their log_pi_k gradient is pi_k times a sum that is zero but for rounding, and
            # the fp32 oracle's own parameters move by ~lr there, which the clause measures)
            ok = tiny & (d <= 1e-2 * lr)
            d = torch.where(ok, torch.zeros_like(d), d)
        err = (d.max() / scale).item()
        parity_log.record('rel', err, bar, what)
        print('FORMS|%s|%s|err=%.3e|bar=%.3e|oracle32=%.3e' % (tag, what, err, bar, o32))
        assert err <= bar, (tag, what, err, bar)
    check('elbo', out['elbo'], ref64['elbo'], ref32['elbo'])
    assert len(ref64['grads']) == (23 if smm else 21) and sorted(ref64['grads']) == sorted(out['grads'])
    for n_ in ref64['grads']:
        check('grad ' + n_, out['grads'][n_], ref64['grads'][n_], ref32['grads'][n_])
    assert len(out['theta_star']) == len(ref64['theta_star']) == (1 if smm else 5)
    for i, (g, a, b) in enumerate(zip(out['theta_star'], ref64['theta_star'], ref32['theta_star'])):
        check('theta* %d' % i, g, a, b)
    for i in range(1 if smm else 5):
        check('theta after CVI %d' % i, tr.theta[i], th64[i], th32_[i])
    for n_, p in zip(*tr.trainables()):
        g = ref64['grads'][n_].double().abs()
        rms = (0.001 ** 0.5) * g                                # Adam's sqrt(v) after one step
        check('param ' + n_, p.detach(), par64[n_], par32[n_], tiny=rms < 1e-2 * rms.max())


def test_graphed_smm_direct_step_is_bit_identical_to_eager():
    """GraphedSVAEStep on an SMM trainer is in table mode, with one and with four steps per replay; 3 replays of 4 steps leave ELBOs,
    parameters, alpha and Adam slots bit-identical to 12 eager direct steps."""
    from vmp_for_svae_amd.training import GraphedSVAEStep
    N, K, Ld, U, Dy, S = C5
    ys = _minibatches(N, Dy, 12, 7)
    tr = _trainer(*C5)
    want_elbo = [float(tr.step(y)['elbo']) for y in ys]
    want = [p.detach().clone() for p in tr.trainables()[1]] + [tr.theta[0].clone()] + list(tr.opt.m) + list(tr.opt.v)
    tr1 = _trainer(*C5)
    assert GraphedSVAEStep(tr1, ys[0], steps_per_replay=1).table_mode
    tr4 = _trainer(*C5)
    gs = GraphedSVAEStep(tr4, ys[0], steps_per_replay=4)
    assert gs.table_mode
    got_elbo = []
    for c in range(3):
        outs = gs(torch.stack(ys[4 * c:4 * c + 4]))
        got_elbo += [float(o['elbo']) for o in outs]
    assert tr4.global_step == 12 and tr4.opt.t == 12
    assert got_elbo == want_elbo
    got = [p.detach() for p in tr4.trainables()[1]] + [tr4.theta[0]] + list(tr4.opt.m) + list(tr4.opt.v)
    for j, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), j


def test_experiments_run_smm_steps_per_replay():
    """experiments.run on an SMM config (the Student-t model of BASELINE config 5): steps_per_replay=4 gives the history and the
    parameters of steps_per_replay=1 bit for bit (it raised before: the multi-step graph needs the direct step)."""
    from vmp_for_svae_amd import experiments
    cfg = {'dataset': 'pinwheel', 'method': 'svae-cvi-smm', 'lr': 0.01, 'lrcvi': 0.1, 'K': 10, 'L': 2, 'U': 50, 'seed': 0, 'DoF': 5}
    res = []
    for n in (1, 4):
        tr, hist, _ = experiments.run(cfg, nb_iters=23, measurement_freq=10, verbose=False, steps_per_replay=n)
        assert tr.smm
        res.append((hist, [p.detach().clone() for p in tr.trainables()[1]] + [t.clone() for t in tr.theta]))
    (h1, p1), (h4, p4) = res
    assert [sorted(h.items()) for h in h1] == [sorted(h.items()) for h in h4]
    for a, b in zip(p1, p4):
        assert torch.equal(a, b)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_data_parallel_smm_direct_step(tmp_path):
    """Two ranks on one GPU (tests/smm_direct_worker.py): the direct step covers both shards; 3 direct (packed exchange buffer) steps
    match 3 autograd steps to the bars above; the graph='dp' replay matches the eager data-parallel direct steps bit for bit in the ELBOs
    and to 2e-5 in the parameters - a departure from bit-identity that is not the direct step's: _step_back's SMM branch (shared by the
    eager and the captured data-parallel step, unchanged here) updates alpha with update_gmm_params and a Python step size eagerly and
    with mul_ / add_ and the device word when captured, which round differently (the GMM data-parallel graph test uses the same bar)."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), WORLD_SIZE='2')
    procs = []
    for r in range(2):
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'smm_direct_worker.py'), str(tmp_path)],
                                      env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0].decode(errors='replace'))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    ranks = [np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r)) for r in range(2)]
    for r in ranks:
        assert 'error' not in r.files, str(r['error'])
        assert int(r['direct_ok']) == 1
        scale = np.maximum(np.abs(r['elbo_autograd'][:, 1]), np.abs(r['elbo_autograd'][:, 2]))
        assert np.all(np.abs(r['elbo_direct'] - r['elbo_autograd']) <= 2e-5 * scale[:, None]), (r['elbo_direct'], r['elbo_autograd'])
        assert float(r['grad_err'].max()) <= 1e-4, r['grad_err']
        assert float(r['param_err'].max()) <= 1e-4, r['param_err']
        assert int(r['graph_back']) == 1
        # graph='dp' against the eager data-parallel direct steps: the ELBOs bit for bit; the parameters to 2e-5 as for the GMM step
        # (tests/test_multirank_gpu.py) - _step_back's SMM branch updates alpha with a Python step size eagerly and with the device word
        # when captured, which round differently
        assert np.array_equal(r['elbo_graphed'], r['elbo_direct'][:, 0])
        assert float(r['graph_param_err'].max()) <= 2e-5, r['graph_param_err']
    assert np.array_equal(ranks[0]['params_direct'], ranks[1]['params_direct'])
