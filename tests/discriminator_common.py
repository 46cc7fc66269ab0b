"""What the discriminator tests share: a plain-torch discriminator (nn.Conv2d, torch.nn.utils.spectral_norm, F.instance_norm /
leaky_relu / avg_pool2d) as oracle -- run on the CPU in float64 and in float32 from identical fp32-rounded values -- and the seeded
recipe of its parameters.  The tolerance rule is tests/closeness.py's: no element beyond max(4 |ATen fp32 - fp64|_max,
OP_FLOOR x scale)."""
import torch
import torch.nn.functional as F
from torch import nn

from closeness import close, grad_close


def heatmaps(value, size, variance):
    """Gaussian heat maps [B,K,H,W] of key points [B,K,2] = (x, y) in [-1,1] on the pixel-centre grid -1 .. 1."""
    h, w = size
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h, dtype=value.dtype), torch.linspace(-1, 1, w, dtype=value.dtype), indexing="ij")
    grid = torch.stack([xs, ys], dim=-1)                                  # [H,W,2]
    d = grid[None, None] - value[:, :, None, None, :]
    return torch.exp(-0.5 * (d ** 2).sum(-1) / variance)


class TorchBlock(nn.Module):
    def __init__(self, cin, cout, norm, pool, sn):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=4)
        if sn:
            self.conv = nn.utils.spectral_norm(self.conv)
        self.norm = nn.InstanceNorm2d(cout, affine=True) if norm else None
        self.pool = pool

    def forward(self, x):
        x = self.conv(x)
        if self.norm is not None:
            x = F.instance_norm(x, weight=self.norm.weight, bias=self.norm.bias, eps=1e-5)
        x = F.leaky_relu(x, 0.2)
        return F.avg_pool2d(x, 2) if self.pool else x


class TorchDiscriminator(nn.Module):
    def __init__(self, num_channels=3, block_expansion=64, num_blocks=4, max_features=512, sn=False, use_kp=False, num_kp=10,
                 kp_variance=0.01):
        super().__init__()
        widths = [num_channels + num_kp * use_kp] + [min(max_features, block_expansion * 2 ** (i + 1)) for i in range(num_blocks)]
        self.down_blocks = nn.ModuleList(TorchBlock(widths[i], widths[i + 1], i != 0, i != num_blocks - 1, sn) for i in range(num_blocks))
        self.conv = nn.Conv2d(widths[-1], 1, kernel_size=1)
        if sn:
            self.conv = nn.utils.spectral_norm(self.conv)
        self.use_kp, self.kp_variance = use_kp, kp_variance

    def forward(self, x, kp=None):
        if self.use_kp:
            x = torch.cat([x, heatmaps(kp["value"], x.shape[2:], self.kp_variance)], dim=1)
        maps = []
        for block in self.down_blocks:
            x = block(x)
            maps.append(x)
        return maps, self.conv(x)


class TorchMultiScale(nn.Module):
    def __init__(self, scales=(), **kwargs):
        super().__init__()
        self.discs = nn.ModuleDict({str(s).replace(".", "-"): TorchDiscriminator(**kwargs) for s in scales})

    def forward(self, x, kp=None):
        out = {}
        for name, disc in self.discs.items():
            scale = name.replace("-", ".")
            out["feature_maps_" + scale], out["prediction_map_" + scale] = disc(x["prediction_" + scale], kp)
        return out


def seeded_state(seed=3, **kwargs):
    """The fp32 state dict of a TorchDiscriminator(**kwargs) built under ``seed``: torch's own initialisation, InstanceNorm weights
    uniform in 0.5 .. 1.5 and biases 0.2 randn."""
    torch.manual_seed(seed)
    net = TorchDiscriminator(**kwargs)
    g = torch.Generator().manual_seed(seed + 1)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for k in sd:
        if ".norm.weight" in k:
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
        elif ".norm.bias" in k:
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
    return sd


def oracle(sd, dtype, **kwargs):
    """A TorchDiscriminator holding ``sd`` in ``dtype`` (a fresh module: the spectral-norm hook's attribute does not deep-copy)."""
    net = TorchDiscriminator(**kwargs)
    net.load_state_dict(sd, strict=True)
    return net.to(dtype)


def module_loss(maps, prediction):
    """((1 - p)^2).mean() + sum_i |f_i|.mean()"""
    return ((1 - prediction) ** 2).mean() + sum(f.abs().mean() for f in maps)


SHIPPED = dict(scales=[1], block_expansion=32, max_features=512, num_blocks=4, sn=True)     # the reference configs' discriminator_params


def fixture_state(seed):
    """The state dict behind tests/golden/disc_tiny.npz (11 MB at the shipped widths, so the fixture holds the seed): in the key order
    of the module, filters and biases uniform in +-1 / sqrt(fan_in), InstanceNorm weights uniform in 0.5 .. 1.5 and biases 0.2 randn,
    u and v normalised randn -- all from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    shapes = {k: tuple(v.shape) for k, v in TorchMultiScale(**SHIPPED).state_dict().items()}
    sd = {}
    for k, shape in shapes.items():
        if k.endswith(("weight_u", "weight_v")):
            sd[k] = F.normalize(torch.randn(shape, generator=g), dim=0)
        elif ".norm.weight" in k:
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif ".norm.bias" in k:
            sd[k] = 0.2 * torch.randn(shape, generator=g)
        else:
            w = shapes[k[:-len("bias")] + "weight_orig"] if k.endswith("bias") else shape
            sd[k] = (2 * torch.rand(shape, generator=g) - 1) / (w[1] * w[2] * w[3]) ** 0.5
    return sd


def state_checksum(sd):
    """sum over the tensors (in key order) of (k + 1) * sum|t| in float64: equal only if fixture_state's generator stream is the
    recording's (a changed torch stream is then reported as that, not as a kernel mismatch)."""
    return float(sum((i + 1) * float(v.double().abs().sum()) for i, (_, v) in enumerate(sorted(sd.items()))))


def decisions_differing(maps, maps64):
    """Per feature map, the units whose sign is not float64's: where |f| lies within rounding of zero, the term |f|.mean() of
    module_loss has two equally valid subgradients (+-1 / N), and every gradient UPSTREAM of that unit moves with the choice."""
    return [int((torch.sign(m.detach().cpu().double()) != torch.sign(w.double())).sum()) for m, w in zip(maps, maps64)]


def gradient_check(deepest_flip, block, got, want, want32, what):
    """``close`` -- unless a unit of feature map ``deepest_flip`` or deeper... precisely: a gradient that belongs to block ``block``
    (the image: block 0) lies upstream of every feature map j >= block; if one of those took a sign decision differently from
    float64 (``deepest_flip >= block``) the float64 gradient is one of two valid answers there and the project's whole-network
    gradient rule ``grad_close`` applies instead.  Gradients downstream of every differing unit stay at ``close``."""
    if deepest_flip >= block:
        grad_close(got, want, want32, what + " [a decision upstream differs: grad_close]")
    else:
        close(got, want, want32, what)
