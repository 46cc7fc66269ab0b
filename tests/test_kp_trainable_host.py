"""Host side of the trainable key-point detectors: the C ABI's new entries are declared and bound, a detector asked for a gradient
without a GPU says that it needs one (it is no longer "inference-only"), and ``kp_ops.kp_head`` checks its shapes before any launch."""
import os
import re

import pytest
import torch

from eamm_amd import KPDetector, KPDetector_a, _lib, kp_ops, tiny_kp_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("eamm_op_kp_head_workspace_floats", "eamm_op_kp_head", "eamm_op_kp_head_backward")


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    table = _lib.SIGNATURES
    for name in ENTRIES:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
        assert name in table, name
    assert len(table["eamm_op_kp_head"][1]) == 17 and len(table["eamm_op_kp_head_backward"][1]) == 20
    assert "#define EAMM_ABI_VERSION 6" in header


@pytest.mark.parametrize("audio", [False, True])
def test_a_cpu_detector_asked_for_a_gradient_needs_a_gpu(audio):
    cfg = tiny_kp_config(audio=audio)
    det = (KPDetector_a if audio else KPDetector)(**cfg).eval()
    assert not any(p.requires_grad for p in det.parameters())
    assert det.process_group is None and det.sync_batchnorm is None
    x = torch.zeros(1, det.out_filters, 16, 16) if audio else torch.zeros(1, 3, 64, 64)
    assert not det._wants_graph(x)
    with torch.no_grad():
        assert not det._wants_graph(x.clone().requires_grad_())
    assert det._wants_graph(x.clone().requires_grad_())
    det.requires_grad_(True)
    assert det._wants_graph(x)
    for mode in (det.eval(), det.train()):
        with pytest.raises(RuntimeError, match="runs only on a ROCm GPU") as e:
            mode(x)
        assert "inference-only" not in str(e.value)
    det.requires_grad_(False)
    with torch.no_grad():
        assert det.train()._wants_graph(x) and not det.eval()._wants_graph(x)


def test_kp_head_checks_its_shapes():
    with pytest.raises(ValueError, match="do not hold"):
        kp_ops.kp_head(torch.zeros(1, 16, 16, 32), 10, 10, 0, 0.1)          # Cs = 32 < 10 + 40
    with pytest.raises(ValueError, match="do not hold"):
        kp_ops.kp_head(torch.zeros(1, 16, 16, 12), 10, 1, 0, 0.1)           # 12 < 14
    with pytest.raises(ValueError, match="no window"):
        kp_ops.kp_head(torch.zeros(1, 6, 16, 64), 10, 10, 0, 0.1)           # 6 - 6 rows
    with pytest.raises(ValueError, match="no window"):
        kp_ops.kp_head(torch.zeros(1, 16, 4, 64), 10, 10, 0, 0.1)
    with pytest.raises(ValueError, match="0, 1 or K"):
        kp_ops.kp_head(torch.zeros(1, 16, 16, 64), 10, 5, 0, 0.1)
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):      # well-formed, but on the CPU
        kp_ops.kp_head(torch.zeros(1, 16, 16, 64), 10, 10, 0, 0.1)
