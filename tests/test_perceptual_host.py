"""CPU-side checks of the perceptual loss's modules (eamm_amd/perceptual.py, perceptual_ops.py): the state-dict layout of the
reference's ``Vgg19`` / ``ImagePyramide`` (modules/model.py:10-68), loading, every refusal, and the binding table."""
import os
import re

import pytest
import torch

import eamm_amd
from conftest import ROOT
from eamm_amd import ImagePyramide, PerceptualLoss, Vgg19, _lib
from eamm_amd import perceptual_ops as P
from perceptual_common import vgg_state

SHAPES = {"slice1.0": (64, 3), "slice2.2": (64, 64), "slice2.5": (128, 64), "slice3.7": (128, 128), "slice3.10": (256, 128),
          "slice4.12": (256, 256), "slice4.14": (256, 256), "slice4.16": (256, 256), "slice4.19": (512, 256),
          "slice5.21": (512, 512), "slice5.23": (512, 512), "slice5.25": (512, 512), "slice5.28": (512, 512)}
ENTRIES = {"eamm_op_vgg_input": 12, "eamm_op_vgg_input_backward": 12, "eamm_op_relu_pool": 8, "eamm_op_relu_pool_backward": 10,
           "eamm_op_l1_pair": 10, "eamm_op_l1_pair_backward": 6}


def test_state_dict_is_the_reference_modules():
    sd = Vgg19().state_dict()
    want = {"mean": (1, 3, 1, 1), "std": (1, 3, 1, 1)}
    for name, (cout, cin) in SHAPES.items():
        want[name + ".weight"], want[name + ".bias"] = (cout, cin, 3, 3), (cout,)
    assert len(want) == 28 and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert torch.equal(sd["mean"].reshape(-1), torch.tensor([0.485, 0.456, 0.406]))
    assert torch.equal(sd["std"].reshape(-1), torch.tensor([0.229, 0.224, 0.225]))
    assert not any(p.requires_grad for p in Vgg19().parameters())
    assert all(n in eamm_amd.__all__ for n in ("Vgg19", "ImagePyramide", "PerceptualLoss", "l1_pair", "relu_pool", "vgg_input"))


def test_loading_is_strict():
    sd = vgg_state()
    net = Vgg19()
    net.load_state_dict(sd)
    assert torch.equal(getattr(net.slice4, "19").weight, sd["slice4.19.weight"])
    missing = {k: v for k, v in sd.items() if k != "slice3.10.bias"}
    with pytest.raises(RuntimeError, match="slice3.10.bias"):
        Vgg19().load_state_dict(missing)
    with pytest.raises(RuntimeError, match="slice6.30.weight"):
        Vgg19().load_state_dict(dict(sd, **{"slice6.30.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        Vgg19().load_state_dict(dict(sd, **{"slice1.0.weight": torch.zeros(64, 4, 3, 3)}))


@pytest.mark.parametrize("prefix, classifier", [("features.", True), ("", False), ("features.", False)])
def test_from_torchvision(prefix, classifier):
    sd = vgg_state()
    tv = {prefix + k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("slice")}
    for i in (30, 32, 34):     # conv5_2 .. conv5_4 of torchvision's vgg19: behind relu5_1, ignored
        tv[f"{prefix}{i}.weight"], tv[f"{prefix}{i}.bias"] = torch.zeros(512, 512, 3, 3), torch.zeros(512)
    if classifier:
        tv["classifier.0.weight"], tv["classifier.0.bias"] = torch.zeros(8, 8), torch.zeros(8)
    net = Vgg19.from_torchvision(tv)
    got = net.state_dict()
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert not any(p.requires_grad for p in net.parameters())
    with pytest.raises(RuntimeError, match="slice5.28.bias"):
        Vgg19.from_torchvision({k: v for k, v in tv.items() if k != prefix + "28.bias"})
    with pytest.raises(KeyError, match="unexpected key"):
        Vgg19.from_torchvision(dict(tv, avgpool=torch.zeros(1)))
    with pytest.raises(KeyError, match="no convolution"):
        Vgg19.from_torchvision(dict(tv, **{prefix + "1.weight": torch.zeros(1)}))


def test_pyramid_buffers():
    pyr = ImagePyramide([1, 0.5, 0.25, 0.125], 3)
    sd = pyr.state_dict()
    assert list(sd) == ["downs.1.weight", "downs.0-5.weight", "downs.0-25.weight", "downs.0-125.weight"]
    ax = torch.arange(13, dtype=torch.float64) - 6
    g = torch.exp(-ax ** 2 / (2 * 1.5 ** 2))
    k = g[:, None] * g[None, :]
    k = (k / k.sum()).float()
    for v in sd.values():     # sigma 1.5 at EVERY scale (modules/util.py:1011-1013)
        assert tuple(v.shape) == (3, 1, 13, 13) and float((v - k).abs().max()) < 1e-8
    assert [d.int_inv_scale for d in pyr.downs.values()] == [1, 2, 4, 8]


def test_refusals_by_name():
    with pytest.raises(ValueError, match="requires_grad=True is not supported"):
        Vgg19(requires_grad=True)
    with pytest.raises(ValueError, match="num_channels must be 3"):
        ImagePyramide([1], 4)
    with pytest.raises(ValueError, match="1 / scale must be an integer, got scale 0.3"):
        ImagePyramide([1, 0.3], 3)
    with pytest.raises(ValueError, match="all loss_weights are zero"):
        PerceptualLoss([1], [0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="five values"):
        PerceptualLoss([1], [1, 1, 1])
    with pytest.raises(ValueError, match="scales is empty"):
        PerceptualLoss([], [1] * 5)
    assert PerceptualLoss([1, 0.5], [10, 10, 10, 0, 0]).taps == 3
    with pytest.raises(ValueError, match=r"inv_scale 3 must be an integer >= 1 dividing H and W"):
        P._check_levels(torch.zeros(1, 3, 16, 16), torch.zeros(3, 1, 13, 13), (3,), "vgg_input")
    with pytest.raises(ValueError, match=r"\[3,1,13,13\] Gaussian buffer"):
        P._check_levels(torch.zeros(1, 3, 16, 16), None, (2,), "vgg_input")
    with pytest.raises(ValueError, match="RGB NCHW"):
        P._check_levels(torch.zeros(1, 4, 16, 16), None, (1,), "vgg_input")


@pytest.mark.parametrize("what, call", [
    ("perceptual.Vgg19", lambda x: Vgg19()(x)),
    ("perceptual.ImagePyramide", lambda x: ImagePyramide([1, 0.5], 3)(x)),
    ("perceptual.PerceptualLoss", lambda x: PerceptualLoss([1], [1] * 5)(x, x)),
    ("perceptual_ops.vgg_input", lambda x: P.vgg_input(x, None, torch.zeros(3), torch.ones(3))),
    ("perceptual_ops.pyramid_levels", lambda x: P.pyramid_levels(x, torch.zeros(3, 1, 13, 13), (2,))),
    ("perceptual_ops.relu_pool", lambda x: P.relu_pool(torch.zeros(1, 4, 4, 32))),
    ("perceptual_ops.l1_pair", lambda x: P.l1_pair(x, x)),
    ("perceptual_ops.frozen_conv3x3", lambda x: P.frozen_conv3x3(torch.zeros(1, 4, 4, 32), torch.zeros(32, 32, 3, 3), None)),
    ("perceptual_ops.vgg_stem", lambda x: P.vgg_stem(x, None, torch.zeros(3), torch.ones(3), torch.zeros(64, 32, 3, 3), torch.zeros(64))),
])
def test_cpu_tensors_are_refused(what, call):
    with pytest.raises(RuntimeError, match=re.escape(f"eamm_amd.{what} runs only on a ROCm GPU")):
        call(torch.zeros(1, 3, 16, 16))


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs == m.group(1).count(",") + 1, name
    assert re.search(r"\bsize_t eamm_op_l1_pair_workspace_floats\(long long n\);", header)
    lib = _lib.lib()
    assert lib.eamm_op_l1_pair_workspace_floats(0) == 0 and lib.eamm_op_l1_pair_workspace_floats(1155) == 4
    assert lib.eamm_op_l1_pair_workspace_floats(1 << 26) == 2048       # the grid is capped: the sum's order depends on n alone


@pytest.mark.parametrize("name, args, message", [
    ("eamm_op_vgg_input", (None, None, None, None, 1, 16, 16, 1, None, None), "image is null"),
    ("eamm_op_relu_pool", (None, 1, 4, 4, 32, None), "x is null"),
    ("eamm_op_relu_pool_backward", (None, None, None, 1, 4, 4, 32, None), "y / dx is null"),
    ("eamm_op_vgg_input_backward", (None, 4, None, None, None, 1, 16, 16, 1, None), "both null"),
    ("eamm_op_l1_pair", (None, None, 16, 1.0, None, None, None, 0), "is null"),
    ("eamm_op_l1_pair_backward", (None, 16, None, None), "is null"),
    # (a fake, aligned, never dereferenced address: the argument checks come before anything touches the device)
    ("eamm_op_vgg_input", (4096, 4096, 4096, 4096, 1, 16, 16, 3, 4096, None), "inv_scale must be an integer >= 1 dividing H and W"),
    ("eamm_op_vgg_input", (4096, None, 4096, 4096, 1, 16, 16, 2, 4096, None), "aa_weight"),
    ("eamm_op_vgg_input", (4096, 4096, None, 4096, 1, 16, 16, 2, 4096, None), "mean / std are null"),
    ("eamm_op_vgg_input", (4096, 4096, 4096, 4096, 0, 16, 16, 2, 4096, None), "B, H, W must be positive"),
    ("eamm_op_vgg_input", (4096, 4096, 4096, 4096, 1, 16, 16, 2, 4100, None), "not 16-byte aligned"),
    ("eamm_op_vgg_input_backward", (4096, 6, None, 4096, 4096, 1, 16, 16, 2, 4096), "multiple of 4"),
    ("eamm_op_vgg_input_backward", (4096, 4, None, 4096, None, 1, 16, 16, 2, 4096), "std is null"),
    ("eamm_op_relu_pool", (4096, 1, 4, 4, 48, None), "C a multiple of 32"),
    ("eamm_op_relu_pool", (4096, 1, 1, 4, 32, 4096), "no pooling window"),
    ("eamm_op_relu_pool", (4100, 1, 4, 4, 32, None), "not 16-byte aligned"),
    ("eamm_op_relu_pool_backward", (4096, None, None, 1, 4, 4, 32, 4096), "dy and dp are both null"),
    ("eamm_op_relu_pool_backward", (4096, None, 4096, 1, 4, 1, 32, 4096), "no pooling window"),
    ("eamm_op_l1_pair", (4096, 4096, 0, 1.0, 4096, 4096, 4096, 64), "n must be positive"),
    ("eamm_op_l1_pair", (4096, 4096, 1155, 1.0, 4096, 4096, 4096, 3), "workspace of eamm_op_l1_pair_workspace_floats"),
    ("eamm_op_l1_pair", (4096, 4100, 16, 1.0, 4096, 4096, 4096, 64), "not 16-byte aligned"),
    ("eamm_op_l1_pair_backward", (4096, 0, 4096, 4096), "n must be positive"),
])
def test_entries_refuse_bad_arguments_by_name(name, args, message):
    lib = _lib.lib()
    assert getattr(lib, name)(0, *args, None) == _lib.ERR_ARG
    text = lib.eamm_last_error(None).decode()
    assert name + ":" in text and message in text, text
