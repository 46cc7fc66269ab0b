"""CPU-side checks of the discriminator: the modules keep the reference's state-dict layout (that of the plain-torch module built
with the same arguments) and load it strictly, unsupported widths are refused by name, and nothing computes without a GPU.  (The
entries' guarded cases and all-zero refusals: tests/test_guarded_host.py, tests/test_op_entries_host.py.)"""
import pytest
import torch

from eamm_amd import Discriminator, MultiScaleDiscriminator, conv4_valid, norm_act_pool
from eamm_amd.disc_ops import thin_channels
from discriminator_common import TorchMultiScale, seeded_state

SHIPPED = dict(scales=[1], block_expansion=32, max_features=512, num_blocks=4, sn=True)


@pytest.mark.parametrize("kwargs", [SHIPPED, dict(scales=[1, 0.5], block_expansion=32, num_blocks=3, sn=False),
                                    dict(scales=[1], block_expansion=64, num_blocks=2, sn=True, use_kp=True, num_kp=10)])
def test_state_dict_layout_is_the_plain_torch_modules(kwargs):
    torch.manual_seed(0)
    ours, theirs = MultiScaleDiscriminator(**kwargs), TorchMultiScale(**kwargs)
    assert list(ours.state_dict().keys()) == list(theirs.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in theirs.state_dict().items()}
    sd = theirs.state_dict()
    ours.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in ours.state_dict().items())
    assert [k for k, _ in ours.named_parameters()] == [k for k, _ in theirs.named_parameters()]


def test_shipped_layout_names():
    keys = set(MultiScaleDiscriminator(**SHIPPED).state_dict())
    assert {"discs.1.down_blocks.0.conv.weight_orig", "discs.1.down_blocks.0.conv.weight_u", "discs.1.down_blocks.0.conv.weight_v",
            "discs.1.down_blocks.0.conv.bias", "discs.1.down_blocks.3.norm.weight", "discs.1.down_blocks.3.norm.bias",
            "discs.1.conv.weight_orig", "discs.1.conv.bias"} <= keys
    assert "discs.1.down_blocks.0.norm.weight" not in keys and "discs.1.down_blocks.0.conv.weight" not in keys
    plain = set(MultiScaleDiscriminator(scales=[0.5], block_expansion=32).state_dict())
    assert {"discs.0-5.down_blocks.1.conv.weight", "discs.0-5.conv.weight"} <= plain


def test_a_missing_or_misshaped_key_is_refused_by_name():
    net = Discriminator(block_expansion=32, num_blocks=2, sn=True)
    sd = seeded_state(block_expansion=32, num_blocks=2, sn=True)
    net.load_state_dict(sd, strict=True)
    missing = {k: v for k, v in sd.items() if k != "down_blocks.1.conv.weight_u"}
    with pytest.raises(RuntimeError, match="down_blocks.1.conv.weight_u"):
        net.load_state_dict(missing, strict=True)
    bad = dict(sd)
    bad["down_blocks.1.norm.weight"] = torch.ones(7)
    with pytest.raises(RuntimeError, match="down_blocks.1.norm.weight"):
        net.load_state_dict(bad, strict=True)
    with pytest.raises(RuntimeError, match="conv.weight_q"):
        net.load_state_dict({**sd, "conv.weight_q": torch.ones(1)}, strict=True)


def test_unsupported_widths_are_refused_by_name():
    with pytest.raises(ValueError, match=r"down_blocks\.0 has 48 output channels"):
        Discriminator(block_expansion=24)
    with pytest.raises(ValueError, match=r"down_blocks\.2 has 100 output channels"):
        Discriminator(block_expansion=16, max_features=100, num_blocks=3)
    with pytest.raises(ValueError, match="kernel_size must be 4"):
        from eamm_amd.discriminator import DownBlock2d
        DownBlock2d(32, 64, kernel_size=3)
    assert [thin_channels(n) for n in (3, 13, 17)] == [4, 16, 32]


def test_defaults_are_the_references():
    net = Discriminator()
    assert [b.conv.out_channels for b in net.down_blocks] == [128, 256, 512, 512] and net.down_blocks[0].conv.in_channels == 3
    assert [b.norm is not None for b in net.down_blocks] == [False, True, True, True]
    assert [b.pool for b in net.down_blocks] == [True, True, True, False]
    assert not net.use_kp and net.kp_variance == 0.01 and "weight" in dict(net.conv.named_parameters())
    assert Discriminator(use_kp=True).down_blocks[0].conv.in_channels == 13
    assert list(MultiScaleDiscriminator().discs) == [] and Discriminator(anything_else=1) is not None


def test_no_cpu_fallback():
    net = Discriminator(block_expansion=32, num_blocks=1)
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        conv4_valid(torch.zeros(1, 8, 8, 32), torch.zeros(32, 32, 4, 4), None)
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        norm_act_pool(torch.zeros(1, 8, 8, 32), None, None, True)
