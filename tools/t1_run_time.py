"""Wall time of VMPLoop.run(n) called again and again, as run_until / run_until_bound call it (default check_every = 5), per iteration.
usage: [N=1000000 D=8 K=16 FLAV=gmm NRUN=5 CALLS=200] python tools/t1_run_time.py   (VMP_LIB_PATH selects an A/B library)"""
import os
import sys
import time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vmp_for_svae_amd as V
from vmp_for_svae_amd.models import _mix
L = V._lib
N = int(os.environ.get('N', 1000000)); D = int(os.environ.get('D', 8)); K = int(os.environ.get('K', 16))
nrun = int(os.environ.get('NRUN', 5)); calls = int(os.environ.get('CALLS', 200))
flav = L.VMP_SMM if os.environ.get('FLAV', 'gmm') == 'smm' else L.VMP_GMM
g = torch.Generator(device='cuda').manual_seed(0)
c = torch.randn(K, D, device='cuda', generator=g) * 5
x = c[torch.randint(0, K, (N,), device='cuda', generator=g)] + torch.randn(N, D, device='cuda', generator=g)
r0 = torch.softmax(3 * torch.randn(N, K, device='cuda', generator=g), 1)
loop = _mix.VMPLoop(x, r0, flav, kappa=torch.full((K,), 5.0, device='cuda') if flav == L.VMP_SMM else None)
for _ in range(20):
    loop.run(nrun)
out = []
for rep in range(7):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        loop.run(nrun)
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / (calls * nrun) * 1e6)
out.sort()
print('run(%d) x %d, N=%d %s: us per iteration min / median / max  %.2f / %.2f / %.2f' % (nrun, calls, N, os.environ.get('FLAV', 'gmm'), out[0], out[3], out[-1]))
