"""Every row of calling.OPERATORS called the ways a training script calls an operator, not only the one way the operator tests do:
operands that are strided views or start off a 16-byte boundary, an upstream gradient that is strided, offset or expanded, an operand of
the wrong dtype or on the wrong device, a gradient asked of some inputs or through some outputs only, and a side stream.

Every varied or spoilt call runs inside ``calling.checked()``: whatever the binding does with the operand, the library is never handed a
tensor that is strided, misaligned, of another dtype or on another device -- the test fails there, before the launch.

* canonical   forward and every gradient against float64 (tests/closeness.py; OP_FLOOR, the floor of the operators' own tests).  The
              baseline of everything below: it is computed once per row and left unchanged, as is the reference.
* layout      each tensor operand in turn, and each upstream gradient, as an equal-valued (a) non-contiguous view of permuted storage,
              (b) contiguous view 4 bytes past a 16-byte boundary, the gradients also (c) expanded with stride 0: the same bits as the
              canonical call.  ``relu_pool`` documents that it needs a contiguous tensor: there (a) is its named ValueError.
* refusal     each tensor operand in turn as float64 and float16 on the GPU and as float32 on the CPU: RuntimeError or ValueError that
              names the operator, with no tensor converted for the library.
* subsets     each differentiable input alone and each output alone: the same bits as the gradient of the all-inputs run through the
              same outputs, which itself meets the float64 reference of that loss; an input that requires no gradient has none.
* side stream forward and backward under ``torch.cuda.stream(side)`` with inputs that exist in that stream's order only
              (tests/guarded.py ``Late``): the same bits.

Gradients that tests/guarded.py lists as ``unstable`` (float atomics: the warp's feature gradient, motion_front's image gradient) are
held to the canonical bar where the others are held to bits."""
import functools

import pytest
import torch

import guarded
from calling import DEV, OPERATORS, checked
from closeness import OP_FLOOR, close

pytestmark = pytest.mark.gpu
ROWS = list(OPERATORS)


# ---- the float64 / float32 reference of a row, once -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """(host operands, one upstream gradient per output, {dtype: (leaves, outputs)}); nothing in it is written to afterwards."""
    row = OPERATORS[name]
    host = row.make()
    runs = {}
    for dt in (torch.float64, torch.float32):
        leaves = {k: v.to(dt).clone().requires_grad_(k in row.diff) for k, v in host.items()}
        runs[dt] = (leaves, row.ref(leaves))
    g = torch.Generator().manual_seed(1234)
    upstream = [None if o is None else torch.randn(o.shape, generator=g) for o in runs[torch.float64][1]]
    return host, upstream, runs


def reference_grads(name, use=None, upstream=None):
    """{dtype: {input: gradient of sum over the used outputs of (output * upstream).sum()}}; an input the loss does not reach gets zeros."""
    row = OPERATORS[name]
    _, default, runs = reference(name)
    upstream = default if upstream is None else upstream
    res = {}
    for dt, (leaves, outs) in runs.items():
        loss = sum((o * g.to(dt)).sum() for i, (o, g) in enumerate(zip(outs, upstream)) if o is not None and (use is None or i in use))
        grads = torch.autograd.grad(loss, [leaves[k] for k in row.diff], retain_graph=True, allow_unused=True)
        res[dt] = {k: torch.zeros_like(leaves[k]) if g is None else g for k, g in zip(row.diff, grads)}
    return res


# ---- one call of a row ----------------------------------------------------------------------------------------------------------------
class _Relayout(torch.autograd.Function):
    """The identity, onto storage of another layout.  A Function of its own, and ``set_`` instead of view operations, because what those
    return is a VIEW to autograd, and an operator that writes in place and has two outputs (relu_pool) may not be given one; this
    returns a plain tensor that merely has strides, or a storage offset."""

    @staticmethod
    def forward(ctx, t, kind):
        new = lambda base, offset, strides=None: t.new_empty(0).set_(base.untyped_storage(), base.storage_offset() + offset, t.shape, strides)
        if kind == "strided":       # a copy whose storage is permuted, seen through the inverse permutation
            if t.dim() >= 2:
                base = t.permute(tuple(reversed(range(t.dim())))).contiguous()
                return new(base, 0, tuple(reversed(base.stride())))
            return new(torch.stack([t, t], dim=1), 0, (2,))
        return new(torch.cat([t.new_zeros(1), t.reshape(-1)]), 1)      # contiguous, 4 bytes past a 16-byte boundary

    @staticmethod
    def backward(ctx, g):
        return g, None


def variant(t, kind):
    """An equal-valued tensor of the asked layout, differentiable in ``t``."""
    if kind == "plain":
        return t
    assert kind in ("strided", "offset"), kind
    v = _Relayout.apply(t, kind)
    if kind == "strided":
        assert not v.is_contiguous(), tuple(t.shape)
    else:
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
    assert torch.equal(v.detach(), t.detach())
    return v


def can_be(t, kind):
    return kind != "strided" or (t.numel() > 1 and (t.dim() == 1 or sum(s > 1 for s in t.shape) >= 2))


def run(name, need=None, vary=None, upstream=None, use=None, place=None):
    """The row's forward (and, where ``need`` names inputs, backward through the outputs ``use``) inside ``checked()``.
    -> (outputs, {input: gradient or None}, what checked() saw)."""
    row = OPERATORS[name]
    host, default, _ = reference(name)
    need = row.diff if need is None else need
    vary = vary or {}
    place = place or (lambda t: t.to(DEV))
    module = row.prepare() if row.prepare is not None else None       # (before the first operand is placed: see test_side_stream)
    leaves, operands = {}, {}
    for k, v in host.items():
        leaf = place(v)
        if k in need:
            leaf.requires_grad_()
        t = variant(leaf, vary.get(k, "plain"))
        leaves[k], operands[k] = leaf, (t.clone() if (k in row.inplace and t is leaf) else t)
    if row.prepare is not None:
        operands["module"] = module
    grads = [None if g is None else (g if g.device.type == "cuda" else place(g)) for g in (default if upstream is None else upstream)]
    with checked() as seen:
        outs = row.call(operands)
        assert len(outs) == len(row.outputs), name
        if need:
            used = [(o, g) for i, (o, g) in enumerate(zip(outs, grads)) if o is not None and (use is None or i in use)]
            torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    torch.cuda.synchronize()
    if row.after is not None:
        row.after()
    return [None if o is None else o.detach() for o in outs], {k: leaves[k].grad for k in row.diff}, seen


@functools.lru_cache(maxsize=None)
def canonical(name):
    return run(name)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


def compare(name, got, want, what, use=None, upstream=None, inputs=None):
    """Outputs and gradients of a varied call against the canonical call's: bits, or the canonical bar for an ``unstable`` gradient."""
    row = OPERATORS[name]
    for label, g, w in zip(row.outputs, got[0], want[0]):
        assert (g is None) == (w is None), (name, what, label)
        assert g is None or same_bits(g, w), (name, what, f"output {label} differs from the canonical call")
    ref = None
    for k in (row.diff if inputs is None else inputs):
        g, w = got[1][k], want[1][k]
        assert (g is None) == (w is None), (name, what, f"gradient of {k}", "missing" if g is None else "unexpected")
        if g is None:
            continue
        if k in row.unstable:
            ref = ref or reference_grads(name, use, upstream)
            close(g, ref[torch.float64][k], ref[torch.float32][k], f"{name} {what} d {k} (atomics)", row.grad_floor)
        else:
            assert same_bits(g, w), (name, what, f"gradient of {k} differs from the canonical call")


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_canonical(name):
    row = OPERATORS[name]
    outs, grads, seen = canonical(name)
    assert seen.reached > 0, "the call converted no tensor: checked() saw nothing"
    _, _, runs = reference(name)
    for label, got, w64, w32 in zip(row.outputs, outs, runs[torch.float64][1], runs[torch.float32][1]):
        assert (got is None) == (w64 is None), (name, label)
        if got is not None:
            close(got, w64, w32, f"{name} {label}", OP_FLOOR)
    ref = reference_grads(name) if row.diff else None
    for k in row.diff:
        assert grads[k] is not None, (name, k)
        close(grads[k], ref[torch.float64][k], ref[torch.float32][k], f"{name} d {k}", row.grad_floor)


@pytest.mark.parametrize("name", ROWS)
def test_operand_layout(name):
    row = OPERATORS[name]
    host, upstream, _ = reference(name)
    want = canonical(name)
    for k, v in host.items():
        for kind in ("strided", "offset"):
            if not can_be(v, kind):
                continue
            if kind == "strided" and row.contiguous_only and k in row.inplace:
                with pytest.raises(ValueError, match=row.contiguous_only):
                    run(name, vary={k: kind})
                continue
            compare(name, run(name, vary={k: kind}), want, f"{k} {kind}")
    if not row.diff:
        return
    for i, g in enumerate(upstream):
        if g is None:
            continue
        for kind in ("strided", "offset"):
            if can_be(g, kind):
                varied = [variant(u.to(DEV), kind) if j == i else u for j, u in enumerate(upstream)]
                compare(name, run(name, upstream=varied), want, f"upstream gradient of {row.outputs[i]} {kind}")
    # (c) what out.sum().backward() delivers: one element, expanded with stride 0 -- against the same gradient as a dense tensor of ones
    ones = [None if g is None else torch.ones(g.shape, device=DEV) for g in upstream]
    expanded = [None if g is None else torch.ones((), device=DEV).expand(g.shape) for g in upstream]
    assert all(g is None or g.dim() == 0 or all(s == 0 for s in g.stride()) for g in expanded)
    compare(name, run(name, upstream=expanded), run(name, upstream=ones), "upstream gradients expanded", upstream=[None if g is None else g.cpu() for g in ones])


@pytest.mark.parametrize("name", ROWS)
def test_wrong_dtype_or_device_is_refused_by_name(name):
    row = OPERATORS[name]
    host, _, _ = reference(name)
    spoil = {"float64": lambda t: t.double(), "float16": lambda t: t.half(), "cpu": lambda t: t.cpu()}
    for k in host:
        for how, fn in spoil.items():
            operands = {a: v.to(DEV) for a, v in host.items()}
            operands[k] = fn(operands[k])
            if row.prepare is not None:
                operands["module"] = row.prepare()
            with checked() as seen:
                with pytest.raises((RuntimeError, ValueError)) as e:
                    row.call(operands)
            torch.cuda.synchronize()
            assert seen.reached == 0, (name, k, how, "the library was reached", seen.converted[:3])
            assert row.op in str(e.value), (name, k, how, "the refusal does not name the operator", str(e.value))


@pytest.mark.parametrize("name", [n for n in ROWS if OPERATORS[n].diff])
def test_gradient_subsets(name):
    row = OPERATORS[name]
    outs, _, _ = canonical(name)
    present = [i for i, o in enumerate(outs) if o is not None]
    uses = [None] + ([(i,) for i in present] if len(present) > 1 else [])
    for use in uses:
        what = "all outputs" if use is None else f"output {row.outputs[use[0]]} alone"
        everything = canonical(name) if use is None else run(name, use=use)
        if use is not None:       # a loss that reads this output only, against its own float64 reference
            compare(name, everything, canonical(name), what, inputs=())
            ref = reference_grads(name, use)
            for k in row.diff:
                w64, w32 = ref[torch.float64][k], ref[torch.float32][k]
                got = everything[1][k]
                if got is None:      # an output this input does not reach: no gradient, where the reference has exact zeros
                    assert not bool(w64.any()), (name, what, k)
                    continue
                close(got, w64, w32, f"{name} {what} d {k}", row.grad_floor)
        if len(row.diff) > 1:
            for k in row.diff:
                alone = run(name, need=(k,), use=use)
                compare(name, alone, everything, f"{what}, {k} alone", use=use, inputs=(k,))
                assert all(alone[1][other] is None for other in row.diff if other != k), (name, what, k, "an input that requires no gradient got one")
    nothing = run(name, need=())
    compare(name, nothing, canonical(name), "no gradient required", inputs=())
    assert all(g is None for g in nothing[1].values())


@pytest.mark.parametrize("name", ROWS)
def test_side_stream(name):
    row = OPERATORS[name]
    want = canonical(name)
    side = guarded.side_stream(DEV)
    late = guarded.Late(DEV, side)
    with guarded.watching(late) as watch, torch.cuda.stream(side):
        got = run(name, place=lambda t: late.place(t, "in"))
    assert watch.calls and watch.calls[0][1], (name, "the delay was over at the first library call: the run proves nothing", watch.calls[:1])
    compare(name, got, want, "side stream")
