"""tests/calling.py without a GPU: every ``torch.autograd.Function`` of ``eamm_amd`` is reached by a row of ``OPERATORS`` (or exempt, with
a reason), ``checked()`` refuses by name what the library must never be handed, and the binding's two operand helpers (``_op.operands``,
``_op.dense``) do on CPU tensors what the GPU tests rely on."""
import glob
import importlib
import os

import pytest
import torch

import calling
from calling import EXEMPT_FUNCTIONS, OPERATORS, checked


def _functions():
    import eamm_amd
    found = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(eamm_amd.__file__), "*.py"))):
        mod = importlib.import_module("eamm_amd." + os.path.basename(path)[:-3])
        for name, obj in vars(mod).items():
            if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__:
                found[name] = mod.__name__
    return found


def test_every_autograd_function_is_reached_by_a_row_or_exempt():
    found = _functions()
    assert len(found) == 25, sorted(found)
    reached = {f for row in OPERATORS.values() for f in row.functions}
    assert reached <= set(found), sorted(reached - set(found))
    assert len(EXEMPT_FUNCTIONS) <= 2 and all(n in found and isinstance(why, str) and len(why) > 10 for n, why in EXEMPT_FUNCTIONS.items())
    assert not reached & set(EXEMPT_FUNCTIONS), "a Function is either reached or exempt"
    missing = sorted(set(found) - reached - set(EXEMPT_FUNCTIONS))
    assert not missing, ("Functions that no row of calling.OPERATORS reaches and calling.EXEMPT_FUNCTIONS does not list", missing)


def test_the_rows_the_issue_names_are_all_there():
    assert len(OPERATORS) == 38
    for row in OPERATORS.values():
        assert set(row.diff) <= set(row.make()) or row.name == "conv2d_same_nhwc_saved", row.name
        assert set(row.unstable) <= set(row.diff) and set(row.inplace) <= set(row.diff), row.name
    ops = {row.op for row in OPERATORS.values()}
    assert ops == {"warp", "warp_nhwc", "conv2d_same", "conv2d_same_nhwc", "first_conv7", "final_conv7_sigmoid", "antialias_down", "kp_records",
                   "motion_front", "motion_head", "kp_head", "conv2d_s2_nhwc", "maxpool3s2_nhwc", "emo_final", "lstm_layer",
                   "conv_transpose4s2_nhwc", "maxpool3_nhwc", "vgg_input", "pyramid_levels", "relu_pool", "l1_pair", "frozen_conv3x3", "vgg_stem",
                   "conv4_valid", "norm_act_pool", "tps_warp_frame", "tps_warp_points", "SynchronizedBatchNorm2d"}


def test_the_saved_transform_row_has_the_smallest_shape_with_an_offset():
    """conv2d_same_nhwc's backward starts from the forward's workspace only where eamm_op_conv_saved_transform_offset names an offset:
    at least 2048 4x4 tiles (the forward's F(4x4,3x3) form) and Cin a multiple of 64.  The row's shape has one, and no shape with
    fewer tiles, or with the next smaller Cin, has."""
    from eamm_amd import _lib
    L, none = _lib.lib(), 2 ** 64 - 1
    B, H, W, cin, cout = calling.SAVED_SHAPE
    assert L.eamm_op_conv_saved_transform_offset(B, H, W, cin, cout, 3, 3) != none
    assert B * (H // 4) * (W // 4) == 2048 and cin == 64 and cout == 32
    assert L.eamm_op_conv_saved_transform_offset(B, H, W - 4, cin, cout, 3, 3) == none
    assert L.eamm_op_conv_saved_transform_offset(B, H, W, 32, cout, 3, 3) == none
    assert L.eamm_op_conv_saved_transform_offset(B, H, W, cin, cout, 7, 7) == none


# ---- checked() on CPU tensors ---------------------------------------------------------------------------------------------------------
def _offset_view(n):
    """n floats, contiguous, starting 4 bytes past a 16-byte boundary."""
    flat = torch.zeros(n + 8)
    lead = (-flat.data_ptr() // 4) % 4 + 1
    v = flat[lead:lead + n]
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_checked_lets_an_aligned_contiguous_float32_tensor_pass_and_counts_it():
    from eamm_amd import _handle
    t = torch.zeros(6, 8)
    assert t.data_ptr() % 16 == 0
    with checked("cpu") as seen:
        p = _handle.ptr(t, "eamm_op_warp", 1)
        assert _handle.ptr(None, "eamm_op_warp", 3) is None
    assert p.value == t.data_ptr() and seen.converted == [("eamm_op_warp", 1)] and seen.reached == 1
    assert _handle.ptr.__module__ == "eamm_amd._handle"          # put back


@pytest.mark.parametrize("what, make, text", [
    ("strided", lambda: torch.zeros(8, 6).t(), "not contiguous"),
    ("offset", lambda: _offset_view(24), "starts 4 bytes past a 16-byte boundary"),
    ("float64", lambda: torch.zeros(6, 8, dtype=torch.float64), "torch.float64, the header documents torch.float32"),
    ("meta", lambda: torch.empty(6, 8, device="meta"), "on meta, the call is on cpu"),
])
def test_checked_refuses_by_name_and_forwards_nothing(what, make, text, monkeypatch):
    from eamm_amd import _handle, _op
    reached = []
    # through _op.call the refusal comes before the library is even looked up
    monkeypatch.setattr(_op._lib, "lib", lambda: reached.append(1))
    with checked("cpu") as seen:
        with pytest.raises(AssertionError, match=f"eamm_op_conv_dev, operand 6: .*{text}"):
            _handle.ptr(make(), "eamm_op_conv_dev", 6)
        with pytest.raises(AssertionError, match=f"eamm_op_relu_pool, operand 1: .*{text}"):
            _op.call("relu_pool", torch.device("cpu"), make(), 1, 2, 3, 32, None)
    assert seen.reached == 0 and not reached


def test_checked_knows_the_operands_the_header_documents_as_another_type():
    from eamm_amd import _handle
    with checked("cpu") as seen:
        _handle.ptr(torch.zeros(2, 4, 2, dtype=torch.float64), "eamm_disc_norm_act_pool", 10)
        _handle.ptr(torch.zeros(1, dtype=torch.int32), "eamm_op_kp_records", 8)
        _handle.ptr(torch.zeros(5, 7, 3, dtype=torch.uint8)[1:], "eamm_op_to_u8", 5)
        with pytest.raises(AssertionError, match="eamm_op_kp_records, operand 8: torch.float32, the header documents torch.int32"):
            _handle.ptr(torch.zeros(4), "eamm_op_kp_records", 8)
        with pytest.raises(AssertionError, match="eamm_disc_norm_act_pool, operand 1: torch.float64"):
            _handle.ptr(torch.zeros(4, dtype=torch.float64), "eamm_disc_norm_act_pool", 1)
    assert seen.reached == 3


def test_checked_replaces_every_name_the_conversion_is_imported_under():
    from eamm_amd import _handle, _op, autograd_ops, sync_batchnorm
    original = _handle.ptr
    with checked("cpu"):
        assert all(f is not original for f in (_handle.ptr, _op.ptr, autograd_ops._ptr, sync_batchnorm.ptr))
    assert all(f is original for f in (_handle.ptr, _op.ptr, autograd_ops._ptr, sync_batchnorm.ptr))


# ---- the binding's operand helpers ------------------------------------------------------------------------------------------------------
def test_dense_returns_the_tensor_itself_or_an_aligned_equal_copy():
    from eamm_amd import _op
    t = torch.arange(48.0).reshape(6, 8)
    assert _op.dense(t) is t and _op.dense(None) is None
    for v in (t.t(), _offset_view(24).copy_(torch.arange(24.0)).view(4, 6), t[:, ::2], t.expand(3, 6, 8)):
        d = _op.dense(v)
        assert d is not v and d.is_contiguous() and d.data_ptr() % 16 == 0 and torch.equal(d, v)
    leaf = _offset_view(8).requires_grad_()
    _op.dense(leaf * 1.0).sum().backward()                       # a copy is differentiable
    assert torch.equal(leaf.grad, torch.ones(8))


def test_operands_refuses_any_operand_by_the_operators_name(monkeypatch):
    from eamm_amd import _op
    gpu = lambda dtype=torch.float32: torch.empty(2, 3, device="meta", dtype=dtype)      # stands for a tensor on the GPU
    monkeypatch.setattr(_op, "need_gpu", lambda t, module, what: None if t.device.type == "meta" and t.dtype == torch.float32
                        else (_ for _ in ()).throw(RuntimeError(f"{what}: refused {t.dtype} on {t.device}")))
    _op.operands("m", "op", gpu(), None, gpu())
    with pytest.raises(RuntimeError, match="op: refused torch.float64 on meta"):
        _op.operands("m", "op", gpu(), None, gpu(torch.float64))
    with pytest.raises(RuntimeError, match="op: refused torch.float32 on cpu"):
        _op.operands("m", "op", gpu(), torch.zeros(2))
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match=r"eamm_amd.m.op runs only on a ROCm GPU \(there is no CPU fallback\)"):
        _op.operands("m", "op", torch.zeros(2), torch.zeros(2))
