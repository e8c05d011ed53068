"""One rank of tests/test_smm_direct_step_gpu.py::test_data_parallel_smm_direct_step (WORLD_SIZE child processes on one GPU, gloo
rendezvous): the SMM-SVAE's data-parallel direct step (SVAETrainer._step_direct(pack=True) -> vmp_svae_step_pack_smm, the one
all-reduce, _step_back) on this rank's half of each minibatch, against the autograd step and against its graph='dp' replay.  Writes
<out>/rank<r>.npz.  Not a test module itself (no test_ prefix)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from vmp_for_svae_amd.models import vae
    from vmp_for_svae_amd.training import SVAETrainer, GraphedSVAEStep
    N, K, Ld, U, Dy, S = 64, 16, 8, 50, 8, 10
    res = {}
    try:
        g = torch.Generator(device='cuda').manual_seed(17)
        ys = [torch.randn(N, Dy, device='cuda', generator=g) * 2 for _ in range(3)]
        shard = [y[rank * N // world:(rank + 1) * N // world].contiguous() for y in ys]

        def fresh(direct=True):
            vae.reset_variables()
            return SVAETrainer(K, Ld, U, Dy, nb_samples=S, lr=3e-3, lrcvi=0.2, decay_rate=0.95, stddev_init_nn=0.1, seed=3, smm=True,
                               dof=5.0, direct_step=direct)

        def run(tr, step):
            el, grads = [], []
            for y in shard:
                o = step(y)
                el.append([float(o[k]) for k in ('elbo', 'neg_rec_err', 'regulariser')])
                grads.append([v.detach().clone() for v in o['grads'].values()])
            state = [p.detach().clone() for p in tr.trainables()[1]] + [tr.theta[0].clone()] + [t.clone() for t in tr.opt.m + tr.opt.v]
            return np.array(el), grads, state
        tr_d = fresh()
        res['direct_ok'] = np.int64(tr_d._direct_ok(shard[0], None, None, None, None))
        el_d, g_d, s_d = run(tr_d, tr_d.step)
        tr_a = fresh(False)
        el_a, g_a, s_a = run(tr_a, tr_a.step)
        rel = lambda a, b: ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()
        res['elbo_direct'], res['elbo_autograd'] = el_d, el_a
        res['grad_err'] = np.array([rel(a, b) for ga, gb in zip(g_d, g_a) for a, b in zip(ga, gb)])
        res['param_err'] = np.array([rel(a, b) for a, b in zip(s_d, s_a)])
        res['params_direct'] = np.concatenate([t.cpu().numpy().reshape(-1) for t in s_d])
        tr_g = fresh()
        gs = GraphedSVAEStep(tr_g, shard[0], warmup=2)
        res['graph_back'] = np.int64(gs.graph_back is not None)
        el_g, _, s_g = run(tr_g, gs)
        res['elbo_graphed'] = el_g[:, 0]
        res['params_graphed'] = np.concatenate([t.cpu().numpy().reshape(-1) for t in s_g])
        res['graph_param_err'] = np.array([rel(a, b) for a, b in zip(s_g, s_d)])
    except Exception:
        import traceback
        res['error'] = np.array(traceback.format_exc())
    dist.barrier()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), **res)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
