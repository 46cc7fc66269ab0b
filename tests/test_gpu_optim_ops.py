"""The multi-tensor Adam entry (eamm_optim_adam, csrc/optim.hip) through ``eamm_amd.adam_step`` on ONE list that holds every path of the
kernel, against torch's single-tensor Adam on the CPU (tests/optim_common.py) at ``closeness.close``'s bar with OP_FLOOR, on p,
exp_avg, exp_avg_sq and the update p - p0 of every tensor.

The list (``optim_common.lengths``; E = elements per workgroup, T = tensors per launch, both read from the library): lengths 1..5 around
the float4 width, E - 1, E, E + 1 and 2 E + 3 around one and two chunks, a zero-length tensor, one view that starts 4 bytes off a
16-byte boundary in p only and one in g only (the scalar path), and 7-element tensors up to T + 1 tensors, so that the list needs a
second launch; the step numbers 1, 2 and 1000 are mixed over the list.  Well under a million elements.

The eamm_optim_ family is not in the guard-band registry's family list, so it makes its guard-band runs here: every p, g, m, v between
NaN bands at skews 0 and 16."""
import ctypes

import pytest
import torch

import guarded
import optim_common as oc
from eamm_amd import _lib, adam_step, optim_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_cache = {}


def the_list():
    """(numels, tensors, steps), drawn once."""
    if "list" not in _cache:
        numels = oc.lengths(optim_ops.block_elems(), optim_ops.table_capacity())
        _cache["list"] = (numels,) + oc.draw_list(numels)
    return _cache["list"]


def reference(weight_decay):
    """(want, want32) of the list, computed once per weight_decay and never changed."""
    if weight_decay not in _cache:
        _, tensors, steps = the_list()
        _cache[weight_decay] = tuple(oc.oracle_step(tensors, steps, weight_decay, dtype) for dtype in (torch.float64, torch.float32))
    return _cache[weight_decay]


def place_list(place):
    """Every tensor's p, g, m, v through ``place`` (tests/guarded.py: Plain, Arena, Late), p / m / v as "inout", g as "in".  The
    operand that is to start 4 bytes off a 16-byte boundary is placed one float longer and handed on without its first element."""
    _, tensors, _ = the_list()
    lists = ([], [], [], [])
    for i, quad in enumerate(tensors):
        for k, (name, t) in enumerate(zip("pgmv", quad)):
            off = (i == oc.OFF_P and name == "p") or (i == oc.OFF_G and name == "g")
            if t.numel() == 0:                        # (an empty tensor has no address to place)
                lists[k].append(torch.empty(0, device=place.device))
                continue
            host = torch.cat([torch.full((1,), float(i)), t]) if off else t
            view = place(host, "in" if name == "g" else "inout", name=f"{name}{i}")
            view = view[1:] if off else view
            assert view.data_ptr() % 16 == (4 if off else 0), (name, i)
            lists[k].append(view)
    return lists


def run(lists, weight_decay):
    _, _, steps = the_list()
    adam_step(*lists, steps, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=weight_decay)


def check_values(lists, weight_decay):
    _, tensors, _ = the_list()
    want, want32 = reference(weight_decay)
    torch.cuda.synchronize()
    for i, quad in enumerate(tensors):
        got = tuple(lists[k][i] for k in (0, 2, 3))
        oc.compare(got, quad[0], want[i], want32[i], f"[{i}] n={quad[0].numel()} wd={weight_decay}")
        assert torch.equal(lists[1][i].cpu(), quad[1]), (i, "the gradient was written to")
        if weight_decay == 0:
            oc.assert_dead_channels_stand_still(got[0], quad[0], quad[2], i)
    # the float in front of an offset view is not the entry's to touch
    for i, k in ((oc.OFF_P, 0), (oc.OFF_G, 1)):
        whole = lists[k][i].as_strided((1,), (1,), lists[k][i].storage_offset() - 1)
        assert float(whole) == float(i)


def test_the_list_holds_every_path():
    numels, tensors, steps = the_list()
    E, T = optim_ops.block_elems(), optim_ops.table_capacity()
    assert len(numels) == T + 1 and sum(numels) < 1_000_000
    assert set(numels) >= {0, 1, 2, 3, 4, 5, E - 1, E, E + 1, 2 * E + 3, 7}
    assert set(steps) == {1, 2, 1000} and len(optim_ops.plan(numels)[0]) == 2
    def regime_of(q):                                   # 0..3 for the gradient scales 1e-8, 1e-3, 1, 1e4
        top = float(q[1].abs().max())
        return 3 if top > 1e3 else 2 if top > 1e-2 else 1 if top > 1e-6 else 0

    sevens = [(regime_of(q), s) for q, s, n in zip(tensors, steps, numels) if n == oc.SEVEN]
    assert {r for r, _ in sevens} == {0, 1, 2, 3} and {s for _, s in sevens} == {1, 2, 1000}
    long = [(regime_of(q), s) for q, s, n in zip(tensors, steps, numels) if n >= E - 1]
    assert len({r for r, _ in long}) >= 3 and {s for _, s in long} == {1, 2, 1000}
    g = torch.cat([q[1] for q in tensors])
    assert float((g == 0).float().mean()) > 0.1 and float(g[g != 0].abs().min()) >= 1e-15


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_against_torch_adam_and_twice_the_same_bits(weight_decay):
    first, second = guarded.Plain(DEV), guarded.Plain(DEV)
    a, b = place_list(first), place_list(second)
    run(a, weight_decay)
    run(b, weight_decay)
    check_values(a, weight_decay)
    assert guarded.same_outputs(first, second) == []


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("skew", guarded.SKEWS)
def test_between_guard_bands(skew, weight_decay):
    plain, arena = guarded.Plain(DEV), guarded.Arena(DEV, skew=skew)
    a, b = place_list(plain), place_list(arena)
    run(a, weight_decay)
    run(b, weight_decay)
    torch.cuda.synchronize()
    arena.check()                                       # bands intact, every g bit-unchanged
    assert all(not bool(torch.isnan(v).any()) for _, v in arena.outs)
    check_values(b, weight_decay)
    assert guarded.same_outputs(plain, arena) == []     # neither the neighbourhood nor the alignment changes a bit


def test_operands_that_exist_in_a_side_streams_order_only():
    """Every operand is NaN until a copy on the side stream, queued behind a delay, brings its data: the entry must enqueue on the
    stream it is given, and neither wait nor read anything back."""
    plain = guarded.Plain(DEV)
    a = place_list(plain)
    run(a, 0.01)
    torch.cuda.synchronize()
    side = guarded.side_stream(DEV)
    late = guarded.Late(DEV, side)
    b = place_list(late)
    with torch.cuda.stream(side):
        run(b, 0.01)
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream
    pending = not late.started.query()
    torch.cuda.synchronize()
    print(f"  the side stream's delay was {'still pending' if pending else 'over'} when the call returned")
    assert all(not bool(torch.isnan(v).any()) for _, v in late.outs)
    assert guarded.same_outputs(plain, late) == []


def test_a_plain_side_stream_gives_the_default_streams_bits():
    """The plain ``torch.cuda.stream`` form, with ONE copy behind the delay, so that the delay is certainly pending at the call: the
    list's operands are views of one buffer, NaN-filled on the default stream and filled on the side stream."""
    _, tensors, steps = the_list()
    plain = guarded.Plain(DEV)
    a = place_list(plain)
    run(a, 0.0)
    torch.cuda.synchronize()
    flat = torch.cat([torch.cat([t, torch.zeros(-t.numel() % 4)]) for quad in tensors for t in quad]).pin_memory()
    dev = torch.full((flat.numel(),), float("nan"), device=DEV)
    torch.cuda.synchronize()
    side = guarded.side_stream(DEV)
    lists, at = ([], [], [], []), 0
    for quad in tensors:
        for k, t in enumerate(quad):
            lists[k].append(dev[at:at + t.numel()])
            at += t.numel() + (-t.numel() % 4)
    guarded._delay(side)
    started = torch.cuda.Event()
    started.record(side)
    with torch.cuda.stream(side):
        dev.copy_(flat, non_blocking=True)
        run(lists, 0.0)
    assert not started.query(), "the delay was over when the call returned: the run proves nothing"
    torch.cuda.synchronize()
    for i in range(len(tensors)):
        for k in (0, 2, 3):
            assert torch.equal(lists[k][i], a[k][i]), (i, "pgmv"[k])
    assert not bool(torch.isnan(dev).any())


def test_misaligned_and_mistyped_operands_are_refused_before_any_launch():
    n = 8
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    before = [t.clone() for t in (p, g, m, v)]
    L = _lib.lib()
    arr = lambda *ts: (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])
    numel, ss, bc = (ctypes.c_longlong * 1)(n - 1), (ctypes.c_float * 1)(1e-3), (ctypes.c_float * 1)(0.5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for which in range(4):                               # an address 2 bytes off, in each of the four arrays
        lists = [arr(t.data_ptr() + 2) if k == which else arr(t) for k, t in enumerate((p, g, m, v))]
        assert L.eamm_optim_adam(0, 1, *lists, numel, ss, bc, 0.5, 0.999, 1e-8, 0.0, stream) == _lib.ERR_ARG
        assert "eamm_optim_adam: tensor 0 has an address that is not 4-byte aligned" in L.eamm_last_error(None).decode()
    for bad in (torch.zeros(n, device=DEV, dtype=torch.float64), torch.zeros(n, device=DEV, dtype=torch.float16),
                torch.zeros(n, device=DEV, dtype=torch.int32)):
        for which in range(4):
            lists = [[bad] if k == which else [t] for k, t in enumerate((p, g, m, v))]
            with pytest.raises(RuntimeError, match="adam_step: float32 tensors only"):
                adam_step(*lists, [1], lr=1e-3)
    with pytest.raises(RuntimeError, match=r"optim_ops.adam_step runs only on a ROCm GPU"):
        adam_step([p], [g.cpu()], [m], [v], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r"adam_step: exp_avgs\[0\] / exp_avg_sqs\[0\] must share the strides"):
        q = torch.zeros(2, 3, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last)
        adam_step([q], [torch.zeros_like(q)], [torch.zeros(2, 3, 4, 5, device=DEV)], [torch.zeros_like(q)], [1], lr=1e-3)
    with pytest.raises(ValueError, match=r"adam_step: params\[0\] is not a dense tensor"):
        q = torch.zeros(4, 6, device=DEV)[:, ::2]
        adam_step([q], [torch.zeros(4, 3, device=DEV)], [torch.zeros_like(q)], [torch.zeros_like(q)], [1], lr=1e-3)
    torch.cuda.synchronize()
    assert all(torch.equal(t, b) for t, b in zip((p, g, m, v), before))
