"""Host side of the split-bf16 final layer: the three bf16 planes the host packs for conv_col7b_kernel sum to the fp32 row-split
weight bit for bit (eamm_final_split_planes, no device involved), and tile code 4003 of eamm_op_conv (the final layer with fp32
products forced) refuses what 4002 refuses, under the entry's name, before any device work."""
import ctypes

import numpy as np
import pytest
import torch

from eamm_amd import _lib
from test_conv_modes_host import P, conv, refused


def planes_of(w):
    """w [3, C, 7, 7] float32 -> (rowsplit [21, C, 7] float32, planes uint16 [C/16, 7, 3, 2, 21, 8], the padding behind them)"""
    L = _lib.lib()
    C = w.shape[1]
    n = L.eamm_final_split_planes_elems(C)
    used = (C // 16) * 7 * 3 * 2 * 21 * 8
    assert n >= used and n * 2 % 1024 == 0 and (n - used) * 2 < 1024          # whole KiB, less than one of padding
    rowsplit = np.full((21, C, 7), np.nan, dtype=np.float32)
    planes = np.full(n, 0xFFFF, dtype=np.uint16)
    wc = np.ascontiguousarray(w)
    rc = L.eamm_final_split_planes(wc.ctypes.data, C, rowsplit.ctypes.data, planes.ctypes.data)
    _lib.check(rc, None)
    return rowsplit, planes[:used].reshape(C // 16, 7, 3, 2, 21, 8), planes[used:]


@pytest.mark.parametrize("C", [32, 64])
def test_the_three_planes_sum_to_the_fp32_weight_bit_for_bit(C):
    g = torch.Generator().manual_seed(77 + C)
    w = (torch.randn(3, C, 7, 7, generator=g) * (2.0 / (C * 49)) ** 0.5).numpy()
    w[:, 5] *= 1e-4                                                         # the magnitudes of the adversarial GPU cases
    w[:, 9] *= 1e4
    w[1, 3, 2, 4] = 0.0
    rowsplit, planes, pad = planes_of(w)
    # rowsplit[dx * 3 + co][c][dy] = w[co][c][dy][dx]
    assert np.array_equal(rowsplit.reshape(7, 3, C, 7), w.transpose(3, 0, 1, 2))
    assert not pad.any()
    # [group][tap][plane][octet][row][element] -> [plane][row n][channel 16 group + 8 octet + element][tap] as float32
    f = (planes.astype(np.uint32) << 16).view(np.float32).transpose(2, 4, 0, 3, 5, 1).reshape(3, 21, C, 7)
    total = (f[0] + f[1]) + f[2]
    assert np.array_equal(total.view(np.uint32), rowsplit.view(np.uint32))
    # by truncation: each plane is the top half of what the planes before it left over
    assert np.array_equal(f[0].view(np.uint32), rowsplit.view(np.uint32) & 0xFFFF0000)
    r1 = rowsplit - f[0]
    assert np.array_equal(f[1].view(np.uint32), r1.view(np.uint32) & 0xFFFF0000)
    assert np.array_equal(f[2], r1 - f[1])


def test_the_packer_refuses_bad_arguments():
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.float32)
    for args in ((None, 64, buf.ctypes.data, buf.ctypes.data), (buf.ctypes.data, 48, buf.ctypes.data, buf.ctypes.data),
                 (buf.ctypes.data, 64, None, buf.ctypes.data), (buf.ctypes.data, 64, buf.ctypes.data, None)):
        assert L.eamm_final_split_planes(*args) == _lib.ERR_ARG
        assert L.eamm_last_error(None).decode().startswith("eamm_final_split_planes:")
    assert L.eamm_final_split_planes_elems(48) == 0 and L.eamm_final_split_planes_elems(0) == 0


@pytest.mark.parametrize("tile", [4002, 4003])
def test_the_final_layer_tiles_refuse_other_layers_under_the_entrys_name(tile):
    good = dict(tile=tile, kh=7, kw=7, cout=3, act=2)
    for name, cut in (("eamm_op_conv_ex", None), ("eamm_op_conv", 21)):
        for bad in (dict(kh=3, kw=3), dict(kh=7, kw=1), dict(cout=4), dict(cout=21), dict(act=0), dict(act=1), dict(c0=96), dict(c0=0),
                    dict(in1=P, c1=32), dict(up=1), dict(pool=1), dict(resid=P)):
            assert refused(name, conv(**{**good, **bad})[:cut]), (name, bad)
        assert f"tile code {tile}" in _lib.lib().eamm_last_error(None).decode()
