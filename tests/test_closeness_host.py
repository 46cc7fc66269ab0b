"""tests/closeness.py on synthetic float64 tensors, no GPU: the bar, the zero-scale substitutions, each ``beyond`` policy's allowance,
the 20-bar cap, both ``nonfinite`` modes.  The floor is a power of two and the references lie on a grid of 1 / 1024: all is exact."""
import math

import pytest
import torch

from closeness import GRAD_FLOOR, OP_FLOOR, close, grad_close, kp_close

FLOOR = 2.0 ** -10
BAR = FLOOR * 4.0          # of reference(n): scale 4, oracle exact
vec = lambda *v: torch.tensor(v, dtype=torch.float64)


def reference(n):
    """(want, want32): ``n`` entries, element n // 2 zero, the two ends -+4; the fp32 oracle is exact."""
    want = (torch.arange(n) - n // 2).double() / 1024
    want[0], want[-1] = -4.0, 4.0
    return want, want.clone()


def off_by(want, excess, count=1):
    """A copy of ``want`` with ``count`` elements ``excess`` away, the zero element first."""
    got = want.clone()
    got[(want.numel() // 2 + torch.arange(count)) % want.numel()] += excess
    return got


def fails(*args, **kwargs):
    with pytest.raises(AssertionError):
        close(*args, **kwargs)
    return True


def test_an_element_at_the_bar_passes_and_the_next_float64_fails():
    assert OP_FLOOR == 2e-5 and GRAD_FLOOR == 5e-3
    want, want32 = reference(3)
    assert close(off_by(want, BAR), want, want32, "at the bar", FLOOR) == 1.0
    assert close(off_by(want, -BAR), want, want32, "at the bar, from below", FLOOR) == 1.0
    assert fails(off_by(want, math.nextafter(BAR, 1.0)), want, want32, "one ulp beyond", FLOOR)
    assert close(want.float(), want, want32, "exact, fp32 input, the default floor") == 0.0
    assert fails(torch.zeros(3), torch.zeros(4), torch.zeros(4), "shapes differ")


def test_the_floor_governs_an_exact_oracle_and_the_oracle_governs_when_it_is_far():
    want = vec(4.0, 0.0, 0.0)
    for want32 in (want.clone(), want + vec(0.0, 0.0, FLOOR / 2)):           # 4 x (FLOOR / 2) / 4 = FLOOR / 2 of scale, below FLOOR
        assert close(vec(4.0, BAR, 0.0), want, want32, "floor", FLOOR) == 1.0
        assert fails(vec(4.0, 2 * BAR, 0.0), want, want32, "floor", FLOOR)
    want32 = want + vec(0.0, 0.0, 0.25)                                       # the bar is 4 x 0.25 = 1, in whichever element the error lies
    assert close(vec(4.0, -1.0, 0.0), want, want32, "oracle", FLOOR) == 1.0
    assert kp_close(vec(4.0, -1.0, 0.0), want, want32, "oracle, through kp_close", FLOOR) == 1.0
    assert fails(vec(4.0, -math.nextafter(1.0, 2.0), 0.0), want, want32, "oracle", FLOOR)


def test_zero_scale_and_gmax():
    zero, hit = torch.zeros(3, dtype=torch.float64), lambda v: vec(0.0, v, 0.0)
    assert close(hit(FLOOR), zero, zero, "all zero: scale 1", FLOOR) == 1.0
    assert fails(hit(2 * FLOOR), zero, zero, "all zero: scale 1", FLOOR)
    assert close(hit(8 * FLOOR), zero, zero, "all zero: scale gmax", FLOOR, gmax=8.0) == 1.0
    assert fails(hit(16 * FLOOR), zero, zero, "all zero: scale gmax", FLOOR, gmax=8.0)
    tiny, small = vec(2.0 ** -40, 0.0, 0.0), vec(2.0 ** -20, 0.0, 0.0)       # 9.1e-13 < 1e-9 x 8 <= 9.5e-7
    assert close(tiny + hit(8 * FLOOR), tiny, tiny, "below 1e-9 gmax: scale gmax", FLOOR, gmax=8.0) == 1.0
    assert kp_close(tiny + hit(8 * FLOOR), tiny, tiny, "the same through kp_close", FLOOR, gmax=8.0) == 1.0
    assert close(small + hit(2.0 ** -20 * FLOOR), small, small, "above it: its own scale", FLOOR, gmax=8.0) == 1.0
    assert fails(small + hit(8 * FLOOR), small, small, "above it: its own scale", FLOOR, gmax=8.0)


@pytest.mark.parametrize("beyond,n,allowed", [("relu", 399, 1), ("relu", 400, 2), ("relu", 1000, 5), ("network", 100, 2), ("network", 1000, 5), ("network", 1199, 5)])
def test_how_many_elements_may_lie_beyond_the_bar(beyond, n, allowed):
    want, want32 = reference(n)
    assert close(off_by(want, 2 * BAR, allowed), want, want32, f"{beyond} {n}", FLOOR, beyond=beyond) == 2.0
    assert fails(off_by(want, 2 * BAR, allowed + 1), want, want32, f"{beyond} {n}", FLOOR, beyond=beyond)
    assert fails(off_by(want, 2 * BAR), want, want32, f"none {n}", FLOOR)
    assert close(off_by(want, BAR, n), want, want32, f"{beyond} {n}: at the bar is not beyond it", FLOOR, beyond=beyond) == 1.0
    # the 20-bar cap, and the two wrappers
    assert close(off_by(want, 20 * BAR), want, want32, "twenty bars", FLOOR, beyond=beyond) == 20.0
    assert fails(off_by(want, math.nextafter(20 * BAR, 1.0)), want, want32, "beyond twenty bars", FLOOR, beyond=beyond)
    wrapper = grad_close if beyond == "network" else lambda *a: kp_close(*a, relu=True)
    wrapper(off_by(want, 2 * BAR, allowed), want, want32, "wrapper", FLOOR)
    with pytest.raises(AssertionError):
        wrapper(off_by(want, 2 * BAR, allowed + 1), want, want32, "wrapper", FLOOR)


def test_nonfinite_refuse_and_match():
    clean, clean32 = reference(10)
    want = clean.clone()
    want[3], want[4] = float("nan"), float("inf")
    got = off_by(want, BAR)
    got[4] = float("nan")                                                     # not finite where the reference is not: a NaN for an inf will do
    assert close(got, want, want, "match", FLOOR, nonfinite="match") == 1.0
    assert fails(got, want, want, "refuse", FLOOR)
    assert fails(off_by(got, BAR), want, want, "match: the bar holds for the rest", FLOOR, nonfinite="match")
    for i, v in ((3, 0.0), (7, float("nan"))):                                # finite where the reference is not; a NaN of its own
        bad = got.clone()
        bad[i] = v
        with pytest.raises(AssertionError, match="finite entries differ"):
            close(bad, want, want, "match", FLOOR, nonfinite="match")
    nothing = torch.full((4,), float("nan"), dtype=torch.float64)
    assert close(nothing, nothing, nothing, "match: nothing finite", FLOOR, nonfinite="match") == 0.0
    for v in (float("nan"), float("inf")):
        bad = clean.clone()
        bad[7] = v
        assert fails(bad, clean, clean32, "refuse: a finite reference", FLOOR)
