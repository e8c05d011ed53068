"""The one stop loop behind VMPLoop.run_until / run_until_bound and DiagLoop.run_until / run_until_bound (_lib.check_until) and the one
missing-data mask normalisation (_lib.mask_u8), on the host: no GPU, no library load.  A stub loop's run(n) advances `iterations`
and records n; its measure follows a scripted sequence.  Every expectation below is worked out by hand from the rule the four methods
had written out each: stop at the first check (not the very first) whose gain over the previous check is below tol (run_until:
absolute) or below tol * max(1, |value|) (run_until_bound)."""
import math

import pytest
import torch

import vmp_for_svae_amd as V
from vmp_for_svae_amd.models import _diag, _mix

L = V._lib


class _Script(object):
    def __init__(self, values, iterations=0):
        self.values, self.iterations, self.runs = list(values), iterations, []

    def run(self, n):
        self.runs.append(n)
        self.iterations += n

    def measure(self):
        return self.values[len(self.runs) - 1]


def _absolute(tol):
    return lambda v, prev: v - prev < tol


def _relative(tol):
    return lambda v, prev: v - prev < tol * max(1.0, abs(v))


def test_absolute_rule_history_and_stop():
    # gains 1.0, 0.5 (not below 0.5: goes on), 0.25 (stops); the 9.0 is never measured.  The loop had done 7 iterations before.
    loop = _Script([1.0, 2.0, 2.5, 2.75, 9.0], iterations=7)
    hist = L.check_until(loop, loop.measure, _absolute(0.5), 3, 100)
    assert hist == [(10, 1.0), (13, 2.0), (16, 2.5), (19, 2.75)]
    assert loop.runs == [3, 3, 3, 3] and loop.iterations == 19
    # a value that falls stops at once, whatever the (positive) tolerance
    loop = _Script([5.0, 4.0, 6.0])
    assert L.check_until(loop, loop.measure, _absolute(1e-9), 2, 100) == [(2, 5.0), (4, 4.0)]


def test_relative_rule_history_and_stop():
    # tol 1e-2: check 2 gains 20 >= 1e-2 * 980 = 9.8, goes on; check 3 gains 5 < 1e-2 * 975 = 9.75, stops
    values = [-1000.0, -980.0, -975.0, -974.0]
    loop = _Script(values)
    assert L.check_until(loop, loop.measure, _relative(1e-2), 5, 1000) == [(5, -1000.0), (10, -980.0), (15, -975.0)]
    # the absolute rule with the same tol does not stop there: 5 and 1 are both >= 1e-2, the script runs out at max_iterations
    loop = _Script(values)
    assert L.check_until(loop, loop.measure, _absolute(1e-2), 5, 20) == [(5, -1000.0), (10, -980.0), (15, -975.0), (20, -974.0)]
    # the floor max(1, |v|): a gain of 0.005 at |v| = 0.105 is below 1e-2 * 1 and stops (1e-2 * 0.105 would not have stopped it)
    loop = _Script([0.1, 0.105, 7.0])
    assert L.check_until(loop, loop.measure, _relative(1e-2), 1, 1000) == [(1, 0.1), (2, 0.105)]


def test_short_last_run():
    loop = _Script([1.0, 2.0, 3.0, 4.0])
    assert L.check_until(loop, loop.measure, _absolute(0.5), 3, 7) == [(3, 1.0), (6, 2.0), (7, 3.0)]
    assert loop.runs == [3, 3, 1]
    loop = _Script([1.0])
    assert L.check_until(loop, loop.measure, _absolute(0.5), 5, 2) == [(2, 1.0)] and loop.runs == [2]
    loop = _Script([])
    assert L.check_until(loop, loop.measure, _absolute(0.5), 5, 0) == [] and loop.runs == []


@pytest.mark.parametrize('check_every', [0, -2, 0.9])
def test_check_every_below_one_is_refused(check_every):
    loop = _Script([1.0])
    with pytest.raises(L.VmpError, match='^check_every must be >= 1$'):
        L.check_until(loop, loop.measure, _absolute(0.5), check_every, 10)
    assert loop.runs == []


@pytest.mark.parametrize('value', [-math.inf, math.nan, 0.0])
def test_one_check_never_stops_early(value):
    # nothing to compare the first check with: a rule that calls everything stalled still lets it happen, and is not asked
    asked = []
    loop = _Script([value, 1.0])
    hist = L.check_until(loop, loop.measure, lambda v, prev: asked.append((v, prev)) or True, 4, 4)
    assert len(hist) == 1 and hist[0][0] == 4 and loop.runs == [4] and asked == []
    loop = _Script([value, 1.0])
    hist = L.check_until(loop, loop.measure, lambda v, prev: asked.append((v, prev)) or True, 4, 8)
    assert len(hist) == 2 and loop.runs == [4, 4] and len(asked) == 1


def _stub(cls, values, **attrs):
    """a loop object of the real class that owns nothing: run() and the measured method are the script's"""
    script = _Script(values)

    class Stub(cls):
        iterations = property(lambda self: script.iterations)
        run = lambda self, n: script.run(n)
        score = heldout = lambda self, x_val: script.measure()
        lower_bound = lambda self: script.measure()
    loop = object.__new__(Stub)
    for k, v in attrs.items():
        setattr(loop, k, v)
    return loop, script


@pytest.mark.parametrize('cls', [_mix.VMPLoop, _diag.DiagLoop])
def test_the_four_methods_apply_their_rule(cls):
    values = [-1000.0, -980.0, -975.0, -974.0]
    loop, script = _stub(cls, values, flavour=L.VMP_GMM)
    assert loop.run_until_bound(1e-2, check_every=5, max_iterations=1000) == [(5, -1000.0), (10, -980.0), (15, -975.0)]
    loop, script = _stub(cls, values)
    assert loop.run_until(None, 1e-2, check_every=5, max_iterations=17) == [(5, -1000.0), (10, -980.0), (15, -975.0), (17, -974.0)]
    assert script.runs == [5, 5, 5, 2]
    loop, script = _stub(cls, values, flavour=L.VMP_GMM)
    for call in (lambda: loop.run_until(None, 1.0, check_every=0), lambda: loop.run_until_bound(1.0, check_every=0)):
        with pytest.raises(L.VmpError, match='^check_every must be >= 1$'):
            call()
    assert script.runs == []


def test_run_until_bound_still_refuses_the_student_t_loop_first():
    loop, script = _stub(_mix.VMPLoop, [1.0], flavour=L.VMP_SMM)
    with pytest.raises(L.VmpError, match='Gaussian mixture'):
        loop.run_until_bound(1e-6, check_every=0)
    assert script.runs == []


def test_one_mask_normalisation():
    assert _diag._mask_u8 is _mix._mask_u8 is L.mask_u8
    rows = [[0, 1, 0], [1, 1, 0]]
    b = torch.tensor(rows, dtype=torch.bool)
    out = L.mask_u8(b)
    assert out.dtype == torch.uint8 and out.tolist() == rows and out.data_ptr() == b.data_ptr()       # a view of the bool bytes
    bt = torch.tensor([[0, 1], [1, 1], [0, 0]], dtype=torch.bool).t()                                  # (2,3), not contiguous
    out = L.mask_u8(bt)
    assert out.is_contiguous() and out.dtype == torch.uint8 and out.tolist() == rows
    u = torch.tensor([[0, 7, 0], [255, 1, 0]], dtype=torch.uint8)                                      # uint8 passes as it is
    out = L.mask_u8(u)
    assert out.data_ptr() == u.data_ptr() and out.tolist() == [[0, 7, 0], [255, 1, 0]]
    for dtype in (torch.float32, torch.float64, torch.int64):
        f = torch.tensor([[0, 2, 0], [-1, 1, 0]]).to(dtype)
        out = L.mask_u8(f)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.tolist() == rows
    out = L.mask_u8(torch.tensor([[0.0, math.nan, -0.0], [0.5, math.inf, 0.0]]))                       # NaN != 0: missing
    assert out.tolist() == rows
