"""Where the fixed cost of the T1 pass kernel goes: clock64 stamps of every wave of blocks 0 and 100 (debug hook)."""
# needs a library built with: make -C vmp-for-svae_amd/csrc EXTRA=-DVMP_DEBUG_TS
# usage: tools/pass_ts.py [smm] [N ...]
import os, sys, ctypes, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vmp_for_svae_amd as V
from vmp_for_svae_amd.models import _mix
L = V._lib
D, K = 8, 16
h = ctypes.CDLL(L.LIB_PATH)
args = sys.argv[1:]
smm = bool(args) and args[0] == 'smm'
if smm:
    args = args[1:]
# slot 6: the XDL form (K == 16) stamps the end of its whole-tile loop there; what follows up to "loop end" is the wave's tail
ORDER = (0, 1, 6, 2, 3, 4, 5)
for N in [int(a) for a in args] or (2048, 1000000):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(N, D, device='cuda', generator=g) * 3
    r0 = torch.softmax(3 * torch.randn(N, K, device='cuda', generator=g), 1)
    loop = _mix.VMPLoop(x, r0, L.VMP_SMM if smm else L.VMP_GMM, kappa=torch.full((K,), 5.0, device='cuda') if smm else None)
    for _ in range(5): loop.step()
    ts = torch.zeros(128, dtype=torch.int64, device='cuda')
    h.vmp_debug_set_pass_timestamps(ctypes.c_void_p(ts.data_ptr()))
    loop.step(); torch.cuda.synchronize()
    t = ts.cpu().view(2, 8, 8)
    for b in range(2):
        t0 = int(t[b, :, 0].min())
        print('%s N=%d block %d: per wave [entry | params+rows | whole tiles done | loop end | after block sync | slabs reduced | partials written] '
              'relative to the first entry, then the tail = loop end - whole tiles done' % ('smm' if smm else 'gmm', N, (0, 100)[b]))
        for w in range(8):
            whole = int(t[b, w, 6])
            print('   wave %d: ' % w + ' '.join('%7d' % ((int(t[b, w, i]) - t0) if int(t[b, w, i]) else 0) for i in ORDER)
                  + '   tail %6d' % ((int(t[b, w, 2]) - whole) if whole else 0))
    h.vmp_debug_set_pass_timestamps(None)
