"""Host side of the trainable emotion detector: the C ABI's new entries are declared and bound (ABI still 6), a detector asked for a
gradient without a GPU says that it needs one -- ``forward`` is no longer "inference-only", ``feature`` still is -- and the
operators of ``emo_ops`` check their shapes before any launch."""
import json
import os
import re

import numpy as np
import pytest
import torch

from eamm_amd import EmotionDetector, _lib, emo_ops, emotion_detector_config
from eamm_amd.weights import emotion_state_dict_spec, synthetic_keypoints, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"eamm_op_conv_s2_workspace_floats": 6, "eamm_op_conv_s2": 13, "eamm_op_conv_s2_dgrad_workspace_floats": 6,
           "eamm_op_conv_s2_dgrad": 13, "eamm_op_conv_s2_wgrad_workspace_floats": 6, "eamm_op_conv_s2_wgrad": 13,
           "eamm_op_emo_maxpool": 8, "eamm_op_emo_maxpool_backward": 9, "eamm_op_emo_final": 7, "eamm_op_emo_final_workspace_floats": 1,
           "eamm_op_emo_final_backward": 11}
UNUSED = ("fc.", "fc_n.", "final_4.", "final_10.")


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b(int|size_t) " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs == m.group(2).count(",") + 1, name
    assert "#define EAMM_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6


def test_a_cpu_detector_asked_for_a_gradient_needs_a_gpu():
    det = EmotionDetector(**{**emotion_detector_config(), "max_features": 256}).eval()
    assert not any(p.requires_grad for p in det.parameters())
    assert det.process_group is None and det.sync_batchnorm is None
    x = torch.zeros(2, 3, 128, 128)
    kp = synthetic_keypoints(2, 10, seed=1)
    v, j = kp["value"], kp["jacobian"]
    assert not det._wants_graph(x, v, j)
    with torch.no_grad():
        assert not det._wants_graph(x, v.clone().requires_grad_(), j)
    for which in range(3):      # the image, value or jacobian asking for a gradient
        args = [t.clone().requires_grad_() if i == which else t for i, t in enumerate((x, v, j))]
        assert det._wants_graph(*args)
        with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
            det(*args)
    det.requires_grad_(True)
    assert det._wants_graph(x, v, j)
    for mode in (det.eval(), det.train()):
        with pytest.raises(RuntimeError, match="runs only on a ROCm GPU") as e:
            mode(x, v, j)
        assert "inference-only" not in str(e.value)
    det.eval()
    with pytest.raises(RuntimeError, match="inference-only"):      # the demo's inference entries stay what they were
        det.feature(x)
    with pytest.raises(RuntimeError, match="inference-only"):
        det.detect(x, v, j)
    det.requires_grad_(False)
    with torch.no_grad():
        assert det.train()._wants_graph(x, v, j) and not det.eval()._wants_graph(x, v, j)


def test_the_graph_route_checks_its_inputs_first():
    det = EmotionDetector(**{**emotion_detector_config(), "max_features": 256}).eval().requires_grad_(True)
    kp5 = synthetic_keypoints(2, 5, seed=1)
    with pytest.raises(ValueError, match="num_kp 10"):
        det(torch.zeros(2, 3, 128, 128), kp5["value"], kp5["jacobian"])


def test_conv2d_s2_checks_its_shapes():
    w3, w1 = torch.zeros(64, 32, 3, 3), torch.zeros(64, 32, 1, 1)
    with pytest.raises(ValueError, match="even map sides"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 7, 8, 32), w3)                 # odd H
    with pytest.raises(ValueError, match="even map sides"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 5, 32), w1)                 # odd W
    with pytest.raises(ValueError, match="multiples of 32"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 8, 48), torch.zeros(64, 48, 3, 3))     # Cin = 48
    with pytest.raises(ValueError, match="multiples of 32"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 8, 32), torch.zeros(40, 32, 1, 1))     # Cout = 40
    with pytest.raises(ValueError, match="multiples of 32"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 8, 64), w3)                 # the input's channels are not the filter's
    with pytest.raises(ValueError, match="1x1 or 3x3"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 8, 32), torch.zeros(64, 32, 5, 5))     # k = 5
    with pytest.raises(ValueError, match="1x1 or 3x3"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 8, 32), torch.zeros(64, 32, 3, 1))
    with pytest.raises(ValueError, match="NHWC input"):
        emo_ops.conv2d_s2_nhwc(torch.zeros(8, 8, 32), w3)
    for w in (w3, w1):
        with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):   # well-formed, but on the CPU
            emo_ops.conv2d_s2_nhwc(torch.zeros(1, 8, 8, 32), w)


def test_the_library_refuses_the_same_shapes():
    """The *_workspace_floats queries: zero = unsupported, and the entries refuse before any launch (NULL pointers never reach one)."""
    L = _lib.lib()
    for q in (L.eamm_op_conv_s2_workspace_floats, L.eamm_op_conv_s2_dgrad_workspace_floats, L.eamm_op_conv_s2_wgrad_workspace_floats):
        assert q(2, 8, 8, 32, 64, 3) > 0 and q(2, 8, 8, 32, 64, 1) > 0
        assert q(2, 7, 8, 32, 64, 3) == 0 and q(2, 8, 6 + 1, 32, 64, 3) == 0      # odd sides
        assert q(2, 8, 8, 48, 64, 3) == 0 and q(2, 8, 8, 32, 40, 1) == 0          # channels off the granule
        assert q(2, 8, 8, 32, 64, 5) == 0 and q(2, 8, 8, 32, 64, 2) == 0          # k
        assert q(0, 8, 8, 32, 64, 3) == 0
    assert L.eamm_op_emo_final_workspace_floats(9) == 9 * 98 and L.eamm_op_emo_final_workspace_floats(0) == 0
    assert L.eamm_op_conv_s2_dgrad(0, None, 2, 7, 8, 32, None, 64, 3, None, None, 0, None) == _lib.ERR_ARG
    assert b"eamm_op_conv_s2_dgrad" in L.eamm_last_error(None)
    assert L.eamm_op_conv_s2_wgrad(0, None, None, 2, 8, 8, 32, 64, 5, None, None, 0, None) == _lib.ERR_ARG
    assert L.eamm_op_conv_s2(0, None, 2, 8, 8, 48, None, 64, 3, None, None, 0, None) == _lib.ERR_ARG
    assert L.eamm_op_emo_maxpool_backward(0, None, None, 1, 3, 4, 64, None, None) == _lib.ERR_ARG


def test_maxpool_and_final_check_their_shapes():
    with pytest.raises(ValueError, match="even map sides"):
        emo_ops.maxpool3s2_nhwc(torch.zeros(1, 5, 8, 64))
    with pytest.raises(ValueError, match="NHWC input"):
        emo_ops.maxpool3s2_nhwc(torch.zeros(8, 8, 64))
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        emo_ops.maxpool3s2_nhwc(torch.zeros(1, 8, 8, 64))
    with pytest.raises(ValueError, match=r"input \[B,64\]"):
        emo_ops.emo_final(torch.zeros(2, 32), torch.zeros(98))
    with pytest.raises(ValueError, match="98 weights"):
        emo_ops.emo_final(torch.zeros(2, 64), torch.zeros(97))
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):
        emo_ops.emo_final(torch.zeros(2, 64), torch.zeros(98))
    det = EmotionDetector(**{**emotion_detector_config(), "max_features": 256})
    w = emo_ops.final_weights(det.final)
    assert tuple(w.shape) == (98,)
    assert torch.equal(w[:8], det.final[0].weight.reshape(-1)) and torch.equal(w[94:], det.final[5].bias)


def test_training_fixture_is_data_with_the_documented_layout():
    z = np.load(os.path.join(ROOT, "tests", "golden", "emotion_tiny128_train_backward.npz"))
    det = EmotionDetector(**json.loads(str(z["config"])))
    names = [n for n, _ in det.named_parameters()]
    unused = sorted(n for n in names if n.startswith(UNUSED))
    assert json.loads(str(z["no_grad"])) == unused and len(unused) == 14
    for n, p in det.named_parameters():
        if n in unused:
            assert "grad/" + n not in z.files
            continue
        stride = int(z["stride/" + n])
        assert z["grad/" + n].dtype == np.float64 and z["grad/" + n].size <= 2048
        assert z["grad/" + n].size == len(range(0, p.numel(), stride)), n
        assert float(z["dist/" + n]) >= 0 and float(z["gmax/" + n]) >= float(np.abs(z["grad/" + n]).max())
    for n in ("image", "value", "jacobian"):
        assert "grad/input/" + n in z.files
    bufs = dict(det.named_buffers())
    for k in z.files:
        if k.startswith("buf/"):
            assert z[k].size == len(range(0, bufs[k[4:]].numel(), int(z["bstride/" + k[4:]]))), k
    # a plain nn.BatchNorm2d counts the training-mode call; the hourglass's synchronised BatchNorms do not (as in the reference)
    cfg = json.loads(str(z["config"]))
    sd = synthetic_state_dict(cfg, seed=int(z["weight_seed"]), spec=emotion_state_dict_spec(cfg))
    assert int(z["buf/layer4.1.bn2.num_batches_tracked"][0]) == int(sd["layer4.1.bn2.num_batches_tracked"]) + 1
    assert int(z["buf/bn1.num_batches_tracked"][0]) == int(sd["bn1.num_batches_tracked"]) + 1
