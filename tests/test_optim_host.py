"""The optimiser without a GPU: the binding's table, the all-zero refusal, the launch planner (``eamm_optim_adam_plan`` is the function
the launching entry uses, exported so that it can be checked here), and ``eamm_amd.Adam`` on CPU parameters, where it hands the step to
torch's single-tensor Adam and must equal ``torch.optim.Adam(foreach=False)`` to the bit -- state layout, ``state_dict`` interchange in
both directions, schedulers, parameters without a gradient, every refusal by name."""
import copy
import ctypes
import os
import random
import re

import pytest
import torch

import optim_common as oc
from conftest import ROOT
from eamm_amd import Adam, _lib, adam_step, optim_ops

ENTRIES = ["eamm_optim_adam", "eamm_optim_adam_plan", "eamm_optim_adam_table_capacity", "eamm_optim_adam_block_elems"]


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_the_entries_are_bound_as_the_header_declares_them():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        declared = 0 if m.group(1).strip() == "void" else m.group(1).count(",") + 1
        assert res is ctypes.c_int and len(args) == declared, name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("eamm_optim_")) == sorted(ENTRIES)
    args = _lib.SIGNATURES["eamm_optim_adam"][1]
    assert args[0] is ctypes.c_int and args[-1] is ctypes.c_void_p            # device first, stream last
    assert _lib.ABI_VERSION == 6 and _lib.lib().eamm_abi_version() == 6
    assert "#define EAMM_ABI_VERSION 6" in header


def test_an_all_zero_call_is_refused_under_the_entrys_own_name():
    L = _lib.lib()
    zeros = [0.0 if t is ctypes.c_double else 0 if t is ctypes.c_int else None for t in _lib.SIGNATURES["eamm_optim_adam"][1]]
    assert L.eamm_optim_adam(*zeros) == _lib.ERR_ARG
    assert L.eamm_last_error(None).decode().startswith("eamm_optim_adam:")
    assert L.eamm_optim_adam_plan(0, None, 0, None, None, None, None) == _lib.ERR_ARG
    assert L.eamm_last_error(None).decode().startswith("eamm_optim_adam_plan:")


def _host_arrays(n, numel=8, address=0x1000):
    ptrs = (ctypes.c_void_p * n)(*[address] * n)
    return ptrs, (ctypes.c_longlong * n)(*[numel] * n), (ctypes.c_float * n)(*[1e-3] * n), (ctypes.c_float * n)(*[0.5] * n)


@pytest.mark.parametrize("spoil,text", [
    ("n", "n = -1 tensors"), ("numel", "numel[1] = -5"), ("null", "tensor 1 has a null address"), ("align2", "not 4-byte aligned"),
    ("beta1", "not finite"), ("eps", "not finite"), ("beta2", r"in \[0, 1\)"), ("step_size", "step_size[1]"), ("bc2", "bc2_sqrt[1]"),
])
def test_the_entry_refuses_by_name_before_it_touches_a_device(spoil, text):
    """Every check comes before the device is made current, so the refusals run here.  The addresses are never dereferenced."""
    L = _lib.lib()
    ptrs, numel, ss, bc = _host_arrays(2)
    bad = (ctypes.c_void_p * 2)(0x1000, None if spoil == "null" else 0x1002 if spoil == "align2" else 0x1000)
    n = -1 if spoil == "n" else 2
    if spoil == "numel":
        numel[1] = -5
    if spoil == "step_size":
        ss[1] = float("inf")
    if spoil == "bc2":
        bc[1] = 0.0
    beta1 = float("nan") if spoil == "beta1" else 0.5
    beta2 = 1.0 if spoil == "beta2" else 0.999
    eps = float("inf") if spoil == "eps" else 1e-8
    assert L.eamm_optim_adam(0, n, ptrs, ptrs, bad, ptrs, numel, ss, bc, beta1, beta2, eps, 0.0, None) == _lib.ERR_ARG
    msg = L.eamm_last_error(None).decode()
    assert msg.startswith("eamm_optim_adam:") and re.search(text if spoil == "beta2" else re.escape(text), msg), msg


# ---- the planner ----------------------------------------------------------------------------------------------------------------
def _check_plan(numels):
    E, T = optim_ops.block_elems(), optim_ops.table_capacity()
    launches, per_block = optim_ops.plan(numels)
    assert len(per_block) == len(numels)
    nxt = 0
    for first, count, blocks in launches:
        assert first == nxt and 1 <= count <= T, (first, count)                 # list order, no gap, within the table
        nxt = first + count
        want = 0
        for i in range(first, nxt):
            n, per = numels[i], per_block[i]
            if n == 0:
                assert per == 0                                                 # no workgroup
                continue
            assert per >= E and per % E == 0, (i, per)
            # workgroup j of the tensor covers [j per, min((j + 1) per, n)): ceil(n / per) of them cover every element exactly once
            want += -(-n // per)
        assert blocks == want, (first, blocks, want)
        assert len({per_block[i] for i in range(first, nxt) if numels[i]}) <= 1  # one chunk size per launch
    assert nxt == len(numels)
    return launches, per_block


def test_the_plan_of_the_operator_tests_list():
    E, T = optim_ops.block_elems(), optim_ops.table_capacity()
    assert E % 4 == 0 and E >= 1024 and 16 <= T <= 72          # float4 chunks; the table fits the 4 KiB of kernel arguments
    numels = oc.lengths(E, T)
    assert len(numels) == T + 1
    launches, per_block = _check_plan(numels)
    assert [(f, c) for f, c, _ in launches] == [(0, T), (T, 1)]
    # 1..5, E - 1, E: one workgroup each; E + 1: two; 2 E + 3: three; 0: none; the two views and every 7-element tensor: one each
    assert launches[0][2] == 7 + 2 + 3 + 0 + 2 + (T - 12) and launches[1][2] == 1
    assert all(per == E for n, per in zip(numels, per_block) if n)


def test_the_plan_of_edge_lists():
    E, T = optim_ops.block_elems(), optim_ops.table_capacity()
    assert _check_plan([])[0] == []
    assert _check_plan([0])[0] == [(0, 1, 0)]
    assert _check_plan([0] * (T + 2))[0] == [(0, T, 0), (T, 2, 0)]
    assert _check_plan([E] * T)[0] == [(0, T, T)]
    assert _check_plan([E] * (2 * T))[0] == [(0, T, T), (T, T, T)]
    # a launch of very many chunks takes larger ones: still every element once, the grid bounded
    launches, per_block = _check_plan([25_000_000, 1, 4 * E + 1] + [3_000_000] * 40)
    assert per_block[0] > E and launches[0][2] <= 2 * 8192
    with pytest.raises(_lib.EammError, match="eamm_optim_adam_plan: numel"):
        optim_ops.plan([5, -1])


def test_the_plan_of_500_random_lengths():
    rng = random.Random(20240)
    E = optim_ops.block_elems()
    numels = []
    for _ in range(500):
        kind = rng.random()
        numels.append(0 if kind < 0.05 else rng.randint(1, 9) if kind < 0.2 else rng.choice((E - 1, E, E + 1, 2 * E, 3 * E + 2)) if kind < 0.3
                      else int(2 ** rng.uniform(0, 24.6)))
    _check_plan(numels)
    assert max(numels) > 4_000_000 and 0 in numels


# ---- the class on CPU parameters ------------------------------------------------------------------------------------------------
def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(5, 3), (7,), (2, 3, 4, 5), (1,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g) * 0.01) for s in shapes]
    ps[2].data = ps[2].data.contiguous(memory_format=torch.channels_last)
    return ps


def _grads(ps, step, seed=100):
    g = torch.Generator().manual_seed(seed + step)
    return [torch.randn(p.shape, generator=g) for p in ps]


def _groups(ps):
    return [{"params": ps[:2], "lr": 2e-4}, {"params": ps[2:], "lr": 1e-3, "weight_decay": 0.01}]


def _run(opt, ps, steps, skip=(), sched=None, first=1):
    for step in range(first, first + steps):
        for i, (p, g) in enumerate(zip(ps, _grads(ps, step))):
            p.grad = None if (i == 1 and step in skip) else g.clone()
        opt.step()
        if sched is not None:
            sched.step()


def _same_state(a, pa, b, pb):
    for x, y in zip(pa, pb):
        assert torch.equal(x, y) and x.stride() == y.stride()
        sa, sb = a.state[x], b.state[y]
        assert sorted(sa) == sorted(sb) == ["exp_avg", "exp_avg_sq", "step"]
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device and torch.equal(sa[k], sb[k]), k
        assert sa["exp_avg"].stride() == x.stride() and sa["step"].dim() == 0 and sa["step"].dtype == torch.float32


def test_cpu_parameters_equal_torch_adam_to_the_bit():
    """Two groups with their own lr and weight_decay, a parameter without a gradient in steps 2 and 3, MultiStepLR with a milestone
    inside the run."""
    pa, pb = _params(), _params()
    a = Adam(_groups(pa), betas=(0.5, 0.999))
    b = torch.optim.Adam(_groups(pb), betas=(0.5, 0.999), foreach=False)
    assert isinstance(a, torch.optim.Optimizer) and isinstance(a, torch.optim.Adam)
    sa = torch.optim.lr_scheduler.MultiStepLR(a, milestones=[2], gamma=0.1)
    sb = torch.optim.lr_scheduler.MultiStepLR(b, milestones=[2], gamma=0.1)
    _run(a, pa, 5, skip=(2, 3), sched=sa)
    _run(b, pb, 5, skip=(2, 3), sched=sb)
    _same_state(a, pa, b, pb)
    assert float(a.state[pa[0]]["step"]) == 5 and float(a.state[pa[1]]["step"]) == 3       # no gradient, no step
    assert [g["lr"] for g in a.param_groups] == [g["lr"] for g in b.param_groups] == pytest.approx([2e-5, 1e-4])


def test_step_returns_the_closures_loss_and_runs_without_a_graph():
    ps = _params()
    opt = Adam(ps, lr=2e-4, betas=(0.5, 0.999))

    def closure():
        assert torch.is_grad_enabled()
        loss = sum((p * p).sum() for p in ps)
        loss.backward()
        return loss

    loss = opt.step(closure)
    assert loss.requires_grad and float(loss.detach()) > 0
    assert all(not p.grad_fn and p.is_leaf for p in ps)
    opt.zero_grad()
    assert all(p.grad is None for p in ps)


@pytest.mark.parametrize("ours_first", [True, False])
def test_state_dict_round_trips_with_torch_adam(ours_first):
    make = [lambda ps: Adam(_groups(ps), betas=(0.5, 0.999)), lambda ps: torch.optim.Adam(_groups(ps), betas=(0.5, 0.999), foreach=False)]
    if not ours_first:
        make.reverse()
    pa = _params()
    a = make[0](pa)
    _run(a, pa, 2)
    sd = copy.deepcopy(a.state_dict())
    pb = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in pa]
    b = make[1](pb)
    b.load_state_dict(sd)
    _run(a, pa, 2, first=3)
    _run(b, pb, 2, first=3)
    _same_state(a, pa, b, pb)
    assert sorted(a.state_dict()["param_groups"][0]) == sorted(b.state_dict()["param_groups"][0])


def test_a_checkpoint_whose_step_is_a_python_int_loads():
    pa, pb = _params(), _params()
    a, b = Adam(pa, lr=2e-4, betas=(0.5, 0.999)), torch.optim.Adam(pb, lr=2e-4, betas=(0.5, 0.999), foreach=False)
    _run(b, pb, 2)
    sd = copy.deepcopy(b.state_dict())
    for s in sd["state"].values():
        s["step"] = int(s["step"])
    with torch.no_grad():
        for x, y in zip(pa, pb):
            x.copy_(y)
    a.load_state_dict(sd)
    assert all(torch.is_tensor(a.state[p]["step"]) and a.state[p]["step"].device.type == "cpu" for p in pa)
    _run(a, pa, 1, first=3)
    _run(b, pb, 1, first=3)
    _same_state(a, pa, b, pb)


def test_foreach_and_fused_are_accepted_and_ignored():
    for kw in ({"foreach": True}, {"foreach": False}, {"fused": True}, {"fused": False}):
        pa, pb = _params(), _params()
        a, b = Adam(pa, lr=2e-4, **kw), torch.optim.Adam(pb, lr=2e-4, foreach=False)
        assert a.param_groups[0]["foreach"] is None and a.param_groups[0]["fused"] is None
        _run(a, pa, 2)
        _run(b, pb, 2)
        _same_state(a, pa, b, pb)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"])
def test_unsupported_flags_are_refused_by_name(flag):
    with pytest.raises(ValueError, match=f"eamm_amd.Adam: {flag}=True is not supported"):
        Adam(_params(), lr=2e-4, **{flag: True})
    opt = Adam(_params(), lr=2e-4)
    opt.param_groups[0][flag] = True            # as a loaded state_dict may set it
    with pytest.raises(ValueError, match=f"eamm_amd.Adam: {flag}=True is not supported"):
        opt.step()


def test_a_tensor_lr_and_sparse_gradients_are_refused_by_name():
    with pytest.raises(ValueError, match="eamm_amd.Adam: lr as a tensor is not supported"):
        Adam(_params(), lr=torch.tensor(2e-4))
    emb = torch.nn.Parameter(torch.zeros(4, 3))
    opt = Adam([emb], lr=2e-4)
    emb.grad = torch.sparse_coo_tensor([[1], [2]], [1.0], (4, 3))
    with pytest.raises(ValueError, match="eamm_amd.Adam: sparse gradients are not supported"):
        opt.step()
    # torch's own constructor checks stay
    with pytest.raises(ValueError, match="Invalid beta parameter at index 0"):
        Adam(_params(), betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="Invalid learning rate"):
        Adam(_params(), lr=-1.0)


def test_the_operator_refuses_cpu_tensors_and_mismatched_lists_by_name():
    t = [torch.zeros(4)]
    with pytest.raises(RuntimeError, match=r"optim_ops.adam_step runs only on a ROCm GPU \(there is no CPU fallback\)"):
        adam_step(t, t, t, t, [1], lr=2e-4)
    with pytest.raises(ValueError, match="adam_step: params, grads, exp_avgs, exp_avg_sqs and steps must be lists of one length"):
        adam_step(t, t, t, t, [1, 2], lr=2e-4)
    with pytest.raises(ValueError, match="adam_step: lr must be a Python number"):
        adam_step(t, t, t, t, [1], lr=torch.tensor(1.0))
    adam_step([], [], [], [], [], lr=2e-4)        # an empty list is no call
