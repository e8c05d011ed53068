"""The streaming loop of the XDL mixture pass (csrc/vmp_mix.hip, pass_xdl_body) runs whole 64-row tiles of K == 16 as straight-line
code (four-wide DPP reductions, stores counted apart from the prefetched rows) and everything else - the ragged last tile, every tile
of K < 16 - through the general form.  One fused step (VMPLoop.step) of both flavours against oracle.mixtures in fp64 at the bars of
tests/test_mix_gpu.py.

The plan (pass_plan) gives every wave at least 64 rows and uses up to 256 x 8 waves, so below 131 072 rows a wave runs ONE tile:
the small shapes reach each form of a tile on its own - N = 64 (a whole tile), 65 and 127 (a whole tile in one wave, a ragged one in
the next), 63 (ragged only), 1 041 with K = 16 and with K = 10 (never the straight-line form), D in {2, 5, 8}, and 65 573 rows (the
2-term moment instance).  What only a wave with SEVERAL tiles shows - the prefetched rows carried from one whole tile to the next
under the counted wait, row0 and the prefetch handed from the straight-line loop to the general one, the fp64 flush every second
tile - is reached by the large shapes: 200 037 rows (104 rows per wave: one whole tile, then 40 rows) and 400 037 rows (split plan,
240 / 152 rows per wave: three or two whole tiles with a flush between them, then a ragged tail), the latter in both flavours with
D in {2, 5, 8} and once with want_logr."""
import numpy as np
import pytest
import torch

import parity_log
import test_mix_gpu as T
from mix_pass_truth import loop as _loop, one_step as _one_step, truth as _truth      # shared with tests/test_mix_tiled_pass_gpu.py

pytestmark = pytest.mark.gpu

SHAPES = [(64, 16), (65, 16), (127, 16), (63, 16), (1024 + 17, 16), (1024 + 17, 10)]


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('D', [2, 5, 8])
@pytest.mark.parametrize('N,K', SHAPES)
def test_one_fused_step_vs_oracle(N, K, D, flavour):
    _one_step(N, D, K, flavour)


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
def test_one_fused_step_vs_oracle_two_term_moments(flavour):
    _one_step(65536 + 37, 8, 16, flavour)


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
def test_one_fused_step_vs_oracle_one_whole_tile_then_a_ragged_one_per_wave(flavour):
    _one_step(200000 + 37, 8, 16, flavour)


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('D', [2, 5, 8])
def test_one_fused_step_vs_oracle_several_whole_tiles_per_wave(D, flavour):
    _one_step(400000 + 37, D, 16, flavour)


@pytest.mark.parametrize('flavour', ['gmm', 'smm'])
@pytest.mark.parametrize('N', [129, 400000 + 37])
def test_logr_is_the_logarithm_of_r(N, flavour):
    """want_logr adds one store per r store to the straight-line tiles: N = 129 (two waves with a whole tile, one with one row) and
    400 037 (whole tiles in a row per wave: the stores of a tile stay in flight across the next staging).  logr is logf of the stored
    fp32 r: held to 4 ulp of fp32 at the magnitude of the logarithm (the device logf is good to 2), exactly -inf where r is 0."""
    smm = flavour == 'smm'
    D, K = 8, 16
    x, r0, r1, _, _, ref32 = _truth(N, D, K, smm)
    loop = _loop(x, r0, smm, K)
    r = loop.step(want_logr=True)
    bar_r = max(1e-5, ref32)
    assert T.abserr(r, r1, flavour + ' want_logr r_nk', bar_r) <= bar_r
    rd, lg = r.double().cpu(), loop.logr.double().cpu()
    pos = rd > 0
    assert pos.any() and torch.equal(lg[~pos], torch.full_like(lg[~pos], -np.inf))
    want = torch.log(rd[pos])
    err = ((lg[pos] - want).abs() / want.abs().clamp_min(1.0)).max().item()
    parity_log.record('rel', err, 4 * 2.0 ** -24, flavour + ' logr vs log(r)')
    assert err <= 4 * 2.0 ** -24
