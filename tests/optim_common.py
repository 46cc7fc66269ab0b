"""What the optimiser's tests share (test_optim_host.py, test_gpu_optim_ops.py, test_gpu_optim.py).  Plain helper module: no pytest hooks,
no fixtures.

The oracle is torch's own Adam on the CPU, the single-tensor form (``foreach=False``): in float64 (``want``) and in float32
(``want32``) from identical fp32-rounded inputs, compared with ``closeness.close`` at ``OP_FLOOR`` with no element beyond the bar, on
``p``, ``exp_avg``, ``exp_avg_sq`` AND on the update ``p - p0``.

The rule scales per tensor, so the inputs keep every regime in a tensor of its own (a twelve-decade gradient in one tensor would hide
its small entries): a tensor's gradient scale is one of 1e-8 (``eps`` decides the update), 1e-3, 1, 1e4; every seventh entry is a dead
channel (gradient, and both moments, exactly zero: the update must be exactly zero); parameters are drawn at about 10 x lr, so that the
update is comparable to ``p``; no gradient magnitude lies between 0 and 1e-15, so the squares stay normal numbers."""
import inspect

import torch
from torch.optim import adam as torch_adam

from closeness import OP_FLOOR, close

LR, BETAS, EPS = 2e-4, (0.5, 0.999), 1e-8          # train.py's optimisers
SCALES = (1e-8, 1e-3, 1.0, 1e4)
STEPS = (1, 2, 1000)
DEAD = 3                                           # entries DEAD, DEAD + 7, ... of every tensor are dead channels
SEVEN = 7                                          # the length of the tensors that fill the list up


def lengths(E, T):
    """The operator tests' list: around the float4 width, around one and two chunks of E, a zero-length tensor, the two views that start
    off a 16-byte boundary (OFF_P, OFF_G), and 7-element tensors up to T + 1 in all."""
    head = [1, 2, 3, 4, 5, E - 1, E, E + 1, 2 * E + 3, 0, 37, 41]
    return head + [SEVEN] * (T + 1 - len(head))


OFF_P, OFF_G = 10, 11                              # indices into lengths(): the view 4 bytes off a 16-byte boundary in p only / in g only


def regime(n, scale, step, seed):
    """(p, g, m, v) of one tensor, fp32 on the CPU, at gradient scale ``scale`` entering step number ``step``."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, generator=gen) * scale
    g = torch.where(g.abs() < 1e-15, torch.full_like(g, 1e-15), g)
    p = torch.randn(n, generator=gen) * (10 * LR)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:      # moments of the size step - 1 updates leave behind, so that the update stays about lr
        m = torch.randn(n, generator=gen) * (0.5 * scale)
        v = (torch.rand(n, generator=gen) + 0.5) * (scale * scale * (1 - BETAS[1] ** (step - 1)))
    for t in (g, m, v):
        t[DEAD::7] = 0
    return p, g, m, v


def draw_list(numels, seed=0):
    """Per tensor (p, g, m, v) and its step number; scales and steps cycle through SCALES and STEPS with different periods."""
    tensors, steps = [], []
    for i, n in enumerate(numels):
        step = STEPS[i % len(STEPS)]
        tensors.append(regime(n, SCALES[(i // 2 + i) % len(SCALES)], step, seed + 17 * i))
        steps.append(step)
    return tensors, steps


def oracle_step(tensors, steps, weight_decay, dtype, lr=LR):
    """One step of torch's single-tensor Adam on copies in ``dtype``: ``steps`` are the numbers AFTER the increment.  -> [(p, m, v)]"""
    p, g, m, v = ([t[k].to(dtype).clone() for t in tensors] for k in range(4))
    state_steps = [torch.tensor(float(s - 1)) for s in steps]
    extra = {"decoupled_weight_decay": False} if "decoupled_weight_decay" in inspect.signature(torch_adam.adam).parameters else {}
    torch_adam.adam(p, g, m, v, [], state_steps, foreach=False, capturable=False, differentiable=False, fused=False, grad_scale=None,
                    found_inf=None, has_complex=False, amsgrad=False, beta1=BETAS[0], beta2=BETAS[1], lr=lr, weight_decay=weight_decay, eps=EPS,
                    maximize=False, **extra)
    assert [float(s) for s in state_steps] == [float(s) for s in steps]
    return list(zip(p, m, v))


def compare(got, p0, want, want32, what, floor=OP_FLOOR):
    """``got`` / ``want`` / ``want32``: (p, m, v) of one tensor; ``p0`` the parameter before the step."""
    if p0.numel() == 0:
        assert all(t.numel() == 0 for t in got)
        return
    for name, k in (("p", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
        close(got[k], want[k], want32[k], f"{what} {name}", floor)
    base = p0.detach().cpu().double().reshape(-1)
    update = [t[0].detach().cpu().double().reshape(-1) - base for t in (got, want, want32)]
    close(update[0], update[1], update[2], f"{what} update", floor)


def assert_dead_channels_stand_still(got_p, p0, m, what):
    """Where the gradient and exp_avg are exactly zero (and there is no weight decay) the update is exactly zero."""
    dead = torch.zeros(p0.numel(), dtype=torch.bool)
    dead[DEAD::7] = True
    dead &= m.reshape(-1) == 0
    assert torch.equal(got_p.detach().cpu().reshape(-1)[dead], p0.reshape(-1)[dead]), what
