"""The project's closeness rule, in one place: one tensor against its float64 reference ``want``, with ``want32`` = the same
computation by the oracle (ATen, or the plain-torch reference) in fp32 from identical fp32-rounded inputs.  Per tensor, relative to
its largest reference entry, the bar is

    max(4 |want32 - want|_max, floor x scale),        scale = |want|_max

-- four times what fp32 arithmetic in another summation order costs on this very input, and never below a floor.  Every accuracy
claim in DESIGN.md rests on it; tests/test_closeness_host.py pins it on synthetic tensors.

``beyond``: how many elements may lie beyond the bar.  "none"; "network", the whole-network gradient rule (a ReLU or max-pool decision
flipped by rounding moves a few elements): at most max(2, n // 200), none beyond 20 bars; "relu", the key-point detectors' rule behind
ReLUs: the same, but one element where n < 400.  ``nonfinite="match"``: a reference may hold entries that are not finite (a window of
one pixel has the grid 0 / 0); ``got`` is then not finite exactly there, and the bar applies to the rest.  No pytest hooks, no fixtures."""
import torch

OP_FLOOR = 2e-5      # operators, forward taps, loss values: two fp32 summation orders differ by this much
GRAD_FLOOR = 5e-3    # a gradient through a whole network: one ReLU flipped by rounding moves it by about 1.6e-3 of scale


def close(got, want, want32, what, floor=OP_FLOOR, *, gmax=None, beyond="none", nonfinite="refuse"):
    """Assert the rule above and print one line.  ``gmax``: the scale to use for a reference that is zero by construction -- all
    zeros, or below 1e-9 of ``gmax``, the largest tensor's scale (a convolution bias in front of batch statistics).  Returns
    err / bar."""
    assert beyond in ("none", "network", "relu") and nonfinite in ("refuse", "match"), (beyond, nonfinite)
    got, want, want32 = (t.detach().cpu().double().reshape(-1) for t in (got, want, want32))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if nonfinite == "refuse":
        assert bool(torch.isfinite(got).all()), what
    else:
        fin = torch.isfinite(want)
        assert bool((torch.isfinite(got) == fin).all()), (what, "finite entries differ")
        if not bool(fin.any()):
            return 0.0
        got, want, want32 = got[fin], want[fin], want32[fin]
    scale = float(want.abs().max())
    if scale == 0.0 or (gmax is not None and scale < 1e-9 * gmax):
        scale = gmax if gmax else 1.0
    oracle = float((want32 - want).abs().max()) / scale
    bar = max(4.0 * oracle, floor) * scale
    diff = (got - want).abs()
    err, n, over = float(diff.max()), diff.numel(), int((diff > bar).sum())
    print(f"  {what:48s} err/scale {err / scale:.2e}  ATen fp32 {oracle:.2e}  bar/scale {bar / scale:.2e}"
          + ("" if beyond == "none" else f"  beyond {over}/{n}"))
    if beyond == "none":
        assert err <= bar, (what, err, bar)
    else:
        allowed = 1 if beyond == "relu" and n < 400 else max(2, n // 200)
        assert over <= allowed, (what, over, allowed, err, bar)
        assert err <= 20 * bar, (what, err, bar)
    return err / bar


def grad_close(got, want, want32, what, floor=GRAD_FLOOR):       # the whole-network gradient rule
    return close(got, want, want32, what, floor, beyond="network")


def kp_close(got, want, want32, what, floor, relu=False, gmax=None, nonfinite="refuse"):       # relu: a ReLU lies between it and the loss
    return close(got, want, want32, what, floor, gmax=gmax, beyond="relu" if relu else "none", nonfinite=nonfinite)
