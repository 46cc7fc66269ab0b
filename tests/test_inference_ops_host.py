"""Host side of the inference path's operator entries (eamm_op_first7 ... eamm_op_audio_scale): each is declared and bound (ABI
still 6) and refuses a bad argument with EAMM_ERR_ARG before any launch -- a host buffer stands in for every device pointer here, so a
call that got past its checks would fault instead of returning."""
import ctypes
import os
import re

import pytest

from eamm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"eamm_op_first7": 10, "eamm_op_motion_head_infer": 13, "eamm_op_motion_head_rowsplit": 16, "eamm_op_final_shift_sum": 8,
           "eamm_op_to_u8": 7, "eamm_op_warp_image": 13, "eamm_op_source_prepare": 11, "eamm_op_broadcast_features": 12,
           "eamm_op_nchw_to_nhwc_pad": 10, "eamm_op_emo_avgpool": 7, "eamm_op_emo_embed": 6, "eamm_op_emo_linear": 12,
           "eamm_op_audio_conv1": 9, "eamm_op_audio_scale": 5}

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte aligned non-null pointer (host memory: never to be launched on)

# entry -> a call that passes every check, as (positional arguments without the device and the stream)
GOOD = {
    "eamm_op_first7": [P, 2, 16, 16, P, P, 64, P],
    "eamm_op_motion_head_infer": [P, P, 2, 10, 16, 16, 1, P, P, P, P],
    "eamm_op_motion_head_rowsplit": [P, 128, 12, P, P, 2, 10, 3, 20, 1, P, P, P, P],
    "eamm_op_final_shift_sum": [P, P, 2, 3, 20, P],
    "eamm_op_to_u8": [P, 3, 5, 7, P],
    "eamm_op_warp_image": [P, P, 2, 2, 24, 40, 6, 10, 3, 3, P],
    "eamm_op_source_prepare": [P, P, 2, 32, 48, 4, 32, P, P],
    "eamm_op_broadcast_features": [P, 3, 1, 4, 6, 32, P, P, P, P],
    "eamm_op_nchw_to_nhwc_pad": [P, 2, 32, 35, 5, 7, 32, P],
    "eamm_op_emo_avgpool": [P, 9, 16, 512, P],
    "eamm_op_emo_embed": [P, P, 9, P],
    "eamm_op_emo_linear": [P, 1260, P, 512, P, P, 300, 9, 1, P],
    "eamm_op_audio_conv1": [P, P, P, 5, 28, 12, P],
    "eamm_op_audio_scale": [P, 257, 1.6],
}
# entry -> indices (into GOOD's list) of the pointers that must not be NULL, and of the sizes that must be positive
REQUIRED = {
    "eamm_op_first7": ([0, 4, 5, 7], [1, 2, 3]),
    "eamm_op_motion_head_infer": ([0, 1, 7, 8], [2, 3, 4, 5]),          # (occlusion: has_occ = 1)
    "eamm_op_motion_head_rowsplit": ([0, 3, 4, 10, 11], [1, 2, 5, 6, 7, 8]),
    "eamm_op_final_shift_sum": ([0, 1, 5], [2, 3, 4]),
    "eamm_op_to_u8": ([0, 4], [1, 2, 3]),
    "eamm_op_warp_image": ([0, 1, 10], [2, 3, 4, 5, 6, 7, 8, 9]),
    "eamm_op_source_prepare": ([0, 1, 7, 8], [2, 3, 4, 5, 6]),         # (aa_weight: inv_scale = 4)
    "eamm_op_broadcast_features": ([0, 6, 8, 9], [1, 2, 3, 4, 5]),      # (scale, shift: out2 given)
    "eamm_op_nchw_to_nhwc_pad": ([0, 7], [1, 2, 3, 4, 5, 6]),
    "eamm_op_emo_avgpool": ([0, 4], [1, 2, 3]),
    "eamm_op_emo_embed": ([0, 1, 3], [2]),
    "eamm_op_emo_linear": ([0, 2, 4, 5, 9], [1, 6, 7]),                 # (x1: K1 = 512)
    "eamm_op_audio_conv1": ([0, 1, 2, 6], [3, 4, 5]),
    "eamm_op_audio_scale": ([0], [1]),
}


def refused(name, args):
    L = _lib.lib()
    code = getattr(L, name)(0, *args, None)
    return code == _lib.ERR_ARG and name.encode() in L.eamm_last_error(None)


def changed(name, **at):
    args = list(GOOD[name])
    for i, v in at.items():
        args[int(i[1:])] = v
    return args


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs == m.group(1).count(",") + 1, name
        assert len(GOOD[name]) == nargs - 2, name
    assert "#define EAMM_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6
    assert sorted(GOOD) == sorted(REQUIRED) == sorted(ENTRIES)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_pointers_and_non_positive_sizes_are_refused(name):
    pointers, sizes = REQUIRED[name]
    for i in pointers:
        assert GOOD[name][i] == P
        assert refused(name, changed(name, **{f"a{i}": None})), (name, "NULL argument", i)
    for i in sizes:
        for v in (0, -1):
            if name == "eamm_op_audio_scale" and v < 0:
                continue                                               # (a size_t)
            assert refused(name, changed(name, **{f"a{i}": v})), (name, "size", i, v)


def test_first7_refuses_an_output_width_without_a_kernel():
    for cout in (3, 16, 48, 80, 160, 256):
        assert refused("eamm_op_first7", changed("eamm_op_first7", a6=cout)), cout


def test_the_heads_refuse_too_many_channels_or_key_points():
    assert refused("eamm_op_motion_head_infer", changed("eamm_op_motion_head_infer", a3=31))
    assert refused("eamm_op_motion_head_infer", changed("eamm_op_motion_head_infer", a4=1))              # the grid needs h, w >= 2
    assert refused("eamm_op_motion_head_infer", changed("eamm_op_motion_head_infer", a6=1, a8=None))     # has_occ without occlusion
    rs = "eamm_op_motion_head_rowsplit"
    assert refused(rs, changed(rs, a1=256, a2=33, a6=30))                                                # NC > 32
    assert refused(rs, changed(rs, a1=256, a2=32, a6=31))                                                # K > 30
    assert refused(rs, changed(rs, a2=11))                                                               # NC < K + 1 + has_occ
    assert refused(rs, changed(rs, a1=80))                                                               # PS < 7 NC
    assert refused(rs, changed(rs, a9=1, a11=None))


def test_broadcast_features_refuses_channels_off_the_float4_grid():
    bf = "eamm_op_broadcast_features"
    for c in (1, 6, 30, 33):
        assert refused(bf, changed(bf, a5=c)), c
    assert refused(bf, changed(bf, a2=2))                                                                # ns neither 1 nor n
    assert refused(bf, changed(bf, a0=P + 4))                                                            # a misaligned float4 pointer


def test_the_other_shape_rules():
    assert refused("eamm_op_warp_image", changed("eamm_op_warp_image", a9=4))                            # channels > src_planes
    assert refused("eamm_op_warp_image", changed("eamm_op_warp_image", a2=3, a3=2))                      # ns neither 1 nor n
    sp = "eamm_op_source_prepare"
    assert refused(sp, changed(sp, a5=3)) and refused(sp, changed(sp, a5=8))                             # inv_scale 1 | 2 | 4
    assert refused(sp, changed(sp, a3=30))                                                               # H % inv_scale
    assert refused(sp, changed(sp, a6=30))                                                               # Cpad % 4
    pad = "eamm_op_nchw_to_nhwc_pad"
    assert refused(pad, changed(pad, a3=31))                                                             # planes < C
    assert refused(pad, changed(pad, a6=16))                                                             # Cpad < C
    lin = "eamm_op_emo_linear"
    assert refused(lin, changed(lin, a1=2048, a3=1))                                                     # the staged rows exceed the LDS
    assert refused(lin, changed(lin, a3=-1))
    assert refused(lin, changed(lin, a8=2))
    assert refused("eamm_op_to_u8", changed("eamm_op_to_u8", a1=1 << 20, a2=1 << 10, a3=1 << 10))        # 2^31 elements and more
