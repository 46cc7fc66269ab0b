"""Host side of the trainable audio network: the C ABI's new entries are declared and bound (ABI still 6), a frozen ``AudioFeatureNet``
/ ``DeconvTail`` refuses what it refused before, an opted-in one asked for a gradient without a GPU says that it needs one -- not
"inference-only" -- the operators of ``audio_ops`` check their shapes by name before any launch, and the two training fixtures are
data with the documented layout."""
import json
import os
import re

import numpy as np
import pytest
import torch

from eamm_amd import AudioFeatureNet, DeconvTail, _lib, audio_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"eamm_op_lstm_workspace_floats": 2, "eamm_op_lstm_forward": 9, "eamm_op_lstm_scan": 6, "eamm_op_lstm_backward_workspace_floats": 2,
           "eamm_op_lstm_backward": 11, "eamm_op_lstm_check": 2, "eamm_op_audio_maxpool": 10, "eamm_op_audio_maxpool_backward": 11,
           "eamm_op_deconv4s2_workspace_floats": 5, "eamm_op_deconv4s2": 13, "eamm_op_deconv4s2_dgrad_workspace_floats": 5,
           "eamm_op_deconv4s2_dgrad": 12, "eamm_op_deconv4s2_wgrad_workspace_floats": 5, "eamm_op_deconv4s2_wgrad": 13}


def inputs(n=2, t=3):
    return torch.zeros(n, 3, 256, 256), torch.zeros(n, t, 28, 12), torch.zeros(n, t, 6)


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b(int|size_t) " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs == m.group(2).count(",") + 1, name
    assert "#define EAMM_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6


def test_a_frozen_network_refuses_what_it_refused_before():
    net = AudioFeatureNet()
    assert not any(p.requires_grad for p in net.parameters()) and net.training       # a fresh nn.Module: frozen, in training mode
    image, audio, pose = inputs()
    assert not net._wants_graph(image, audio, pose) and not net.decon._wants_graph()
    with pytest.raises(RuntimeError, match="inference-only"):                           # an input asking for a gradient
        net.lstm_features(image.clone().requires_grad_(), audio, pose)
    with pytest.raises(RuntimeError, match="inference-only"):
        net.decon(torch.zeros(2, 256).requires_grad_())
    for mode in (net.train(), net.eval()):
        with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):              # frozen, nothing asks: the engine's refusal
            mode(image, audio, pose, "cnn", 1.6)
        with pytest.raises(NotImplementedError, match="StyleGAN2"):
            mode(image, audio, pose, "gan", 1.6)
        with pytest.raises(Exception, match="jaco_net type wrong"):
            mode(image, audio, pose, "mlp", 1.6)
        with pytest.raises(ValueError, match=r"audio must be \[N,T,28,12\]"):
            mode(image, audio[:, :, :27], pose, "cnn", 1.6)
        with pytest.raises(ValueError, match=r"pose must be \[N,T,6\]"):
            mode(image, audio, pose[:, :2], "cnn", 1.6)
        with pytest.raises(ValueError, match="1 to 8 clips"):
            mode(torch.zeros(9, 3, 256, 256), torch.zeros(9, 3, 28, 12), torch.zeros(9, 3, 6), "cnn", 1.6)


def test_an_opted_in_network_without_a_gpu_says_that_it_needs_one():
    net = AudioFeatureNet().requires_grad_(True)
    assert net.process_group is None and net.sync_batchnorm is None
    image, audio, pose = inputs()
    for mode in (net.train(), net.eval()):
        assert mode._wants_graph(image, audio, pose)
        for call in (lambda: mode(image, audio, pose, "cnn", 1.6), lambda: mode.lstm_features(image, audio, pose),
                     lambda: mode.decon(torch.zeros(2, 256))):
            with pytest.raises(RuntimeError, match="runs only on a ROCm GPU") as e:
                call()
            assert "inference-only" not in str(e.value)
        # the order of the checks and their messages are the frozen module's
        with pytest.raises(NotImplementedError, match="StyleGAN2"):
            mode(image, audio, pose, "gan", 1.6)
        with pytest.raises(Exception, match="jaco_net type wrong"):
            mode(image, audio, pose, "mlp", 1.6)
        with pytest.raises(ValueError, match=r"example_image must be \[N,3,256,256\]"):
            mode(image[:, :, :128], audio, pose, "cnn", 1.6)
        with pytest.raises(ValueError, match=r"audio must be \[N,T,28,12\]"):
            mode(image, audio[:, :, :27], pose, "cnn", 1.6)
        with pytest.raises(ValueError, match="state="):
            mode.lstm_features(image, audio, pose, state={})
        with pytest.raises(RuntimeError, match="inference-only"):                       # forward_split stays an inference entry
            mode.decon.forward_split(torch.zeros(2, 256))
    with torch.no_grad():
        assert net.train()._wants_graph(image, audio, pose) and not net.eval()._wants_graph(image, audio, pose)
        assert net.decon.train()._wants_graph() and not net.decon.eval()._wants_graph()
    net.requires_grad_(False)
    assert not net.train()._wants_graph(image, audio, pose)


def test_lstm_layer_checks_its_shapes():
    w = torch.zeros(1024, 256)
    with pytest.raises(ValueError, match=r"xproj must be \[N,T,1024\]"):
        audio_ops.lstm_layer(torch.zeros(2, 3, 512), w)
    with pytest.raises(ValueError, match=r"xproj must be \[N,T,1024\]"):
        audio_ops.lstm_layer(torch.zeros(3, 1024), w)
    with pytest.raises(ValueError, match="1 to 8 clips"):
        audio_ops.lstm_layer(torch.zeros(9, 3, 1024), w)
    with pytest.raises(ValueError, match="no time steps"):
        audio_ops.lstm_layer(torch.zeros(2, 0, 1024), w)
    with pytest.raises(ValueError, match=r"w_hh must be \[1024,256\]"):
        audio_ops.lstm_layer(torch.zeros(2, 3, 1024), torch.zeros(256, 1024))
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        audio_ops.lstm_layer(torch.zeros(2, 3, 1024), w)


def test_conv_transpose4s2_checks_its_shapes():
    x, w = torch.zeros(1, 4, 4, 64), torch.zeros(64, 35, 4, 4)
    with pytest.raises(ValueError, match="NHWC input"):
        audio_ops.conv_transpose4s2_nhwc(torch.zeros(4, 4, 64), w)
    with pytest.raises(ValueError, match="4x4 filters only"):
        audio_ops.conv_transpose4s2_nhwc(x, torch.zeros(64, 35, 6, 6))
    with pytest.raises(ValueError, match="does not fit input"):
        audio_ops.conv_transpose4s2_nhwc(x, torch.zeros(32, 35, 4, 4))
    with pytest.raises(ValueError, match=r"bias must be \[35\]"):
        audio_ops.conv_transpose4s2_nhwc(x, w, torch.zeros(32))
    with pytest.raises(ValueError, match="empty input"):
        audio_ops.conv_transpose4s2_nhwc(torch.zeros(1, 0, 4, 64), w)
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        audio_ops.conv_transpose4s2_nhwc(x, w, torch.zeros(35))


def test_maxpool3_checks_its_shapes():
    with pytest.raises(ValueError, match="NHWC input"):
        audio_ops.maxpool3_nhwc(torch.zeros(28, 12, 128), 1, 2)
    with pytest.raises(ValueError, match="strides 1 or 2"):
        audio_ops.maxpool3_nhwc(torch.zeros(1, 28, 12, 128), 3, 2)
    with pytest.raises(ValueError, match="map sides of at least 3"):
        audio_ops.maxpool3_nhwc(torch.zeros(1, 2, 12, 128), 1, 2)
    with pytest.raises(ValueError, match="multiple of 4"):
        audio_ops.maxpool3_nhwc(torch.zeros(1, 28, 12, 6), 1, 2)
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        audio_ops.maxpool3_nhwc(torch.zeros(1, 28, 12, 128), 1, 2)


def test_the_library_refuses_the_same_shapes():
    """The *_workspace_floats queries: zero = unsupported, and the entries refuse before any launch (NULL pointers never reach one)."""
    L = _lib.lib()
    assert L.eamm_op_lstm_workspace_floats(8, 5) > 0 and L.eamm_op_lstm_backward_workspace_floats(1, 1) == 2 * 2 * 8 * 1024
    for q in (L.eamm_op_lstm_workspace_floats, L.eamm_op_lstm_backward_workspace_floats):
        assert q(0, 5) == 0 and q(9, 5) == 0 and q(2, 0) == 0
    for q in (L.eamm_op_deconv4s2_workspace_floats, L.eamm_op_deconv4s2_dgrad_workspace_floats, L.eamm_op_deconv4s2_wgrad_workspace_floats):
        assert q(2, 5, 3, 256, 128) > 0 and q(1, 1, 1, 32, 32) > 0
        assert q(2, 5, 3, 48, 128) == 0 and q(2, 5, 3, 256, 35) == 0 and q(0, 5, 3, 256, 128) == 0 and q(2, 0, 3, 256, 128) == 0
    assert L.eamm_op_lstm_forward(0, None, None, 9, 5, None, None, 0, None) == _lib.ERR_ARG
    assert b"eamm_op_lstm_forward" in L.eamm_last_error(None)
    assert L.eamm_op_lstm_backward(0, None, None, None, None, 2, 0, None, None, 0, None) == _lib.ERR_ARG
    assert L.eamm_op_lstm_scan(0, None, 2, 3, None, None) == _lib.ERR_ARG
    assert L.eamm_op_deconv4s2(0, None, 2, 5, 3, 48, None, None, 128, None, None, 0, None) == _lib.ERR_ARG
    assert L.eamm_op_deconv4s2_dgrad(0, None, 2, 5, 3, 256, None, 35, None, None, 0, None) == _lib.ERR_ARG
    assert L.eamm_op_deconv4s2_wgrad(0, None, None, 2, 5, 3, 256, 128, None, None, None, 0, None) == _lib.ERR_ARG
    assert L.eamm_op_audio_maxpool_backward(0, None, None, 1, 2, 12, 128, 1, 2, None, None) == _lib.ERR_ARG
    assert L.eamm_op_audio_maxpool(0, None, 1, 28, 12, 128, 3, 2, None, None) == _lib.ERR_ARG


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_training_fixtures_are_data_with_the_documented_layout(mode):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"audio_{mode}_backward.npz"))
    net = AudioFeatureNet()
    params = dict(net.named_parameters())
    unused = json.loads(str(z["no_grad"]))
    assert unused == sorted(n for n in params if n.startswith("generator.")) and len(unused) == 82
    with_grad = [k[5:] for k in z.files if k.startswith("grad/")]
    assert len(with_grad) == 88 and sorted(with_grad) == sorted([n for n in params if n not in unused] + ["input/image", "input/audio", "input/pose"])
    n, t = int(z["clips"]), int(z["steps"])
    assert (n, t, float(z["weight"]), int(z["weight_seed"]), int(z["input_seed"]), int(z["loss_seed"])) == (2, 3, 1.6, 2468, 31, 3)
    numel = {"input/image": n * 3 * 256 * 256, "input/audio": n * t * 28 * 12, "input/pose": n * t * 6}
    for name in with_grad:
        size = numel[name] if name in numel else params[name].numel()
        stride = int(z["stride/" + name])
        assert z["grad/" + name].dtype == np.float64 and z["grad/" + name].size <= 2048
        assert z["grad/" + name].size == len(range(0, size, stride)), name
        assert float(z["dist/" + name]) >= 0 and float(z["gmax/" + name]) >= float(np.abs(z["grad/" + name]).max())
    for name, size in (("deco_out", n * t * 35 * 64 * 64), ("lstm_out", n * t * 256)):
        assert z["out/" + name].size == len(range(0, size, int(z["ostride/" + name]))) <= 2048 and float(z["floor/" + name]) >= 0
    bufs = [k for k in z.files if k.startswith("buf/")]
    if mode == "eval":
        assert not bufs
        return
    mine = dict(net.named_buffers())
    assert len(bufs) == 3 * 17
    for k in bufs:
        assert z[k].size == len(range(0, mine[k[4:]].numel(), int(z["bstride/" + k[4:]]))), k
    # a plain nn.BatchNorm2d counts its T training-mode calls; the image encoder's synchronised BatchNorms do not (as in the reference)
    from eamm_amd.weights import audio_feature_state_dict_spec, synthetic_state_dict
    sd = synthetic_state_dict(None, seed=2468, spec=audio_feature_state_dict_spec())
    assert int(z["buf/decon.1.num_batches_tracked"][0]) == int(sd["decon.1.num_batches_tracked"]) + t
    assert int(z["buf/audio_eocder.0.1.num_batches_tracked"][0]) == int(sd["audio_eocder.0.1.num_batches_tracked"]) + t
    assert int(z["buf/down_blocks.0.norm.num_batches_tracked"][0]) == int(sd["down_blocks.0.norm.num_batches_tracked"])
