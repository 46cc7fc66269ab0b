"""Host side of eamm_op_conv_ex, eamm_op_wino_transform and eamm_op_warp_ex: each is declared and bound (ABI still 6) and refuses
a bad combination of the engine-only operands with EAMM_ERR_ARG under its own name before any device work -- a host buffer stands in
for every device pointer here, so a call that got past its checks would fault instead of returning.  Every call below is a refusal."""
import ctypes
import os
import re

import pytest

from eamm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"eamm_op_conv_ex": 30, "eamm_op_wino_transform": 11, "eamm_op_warp_ex": 18}

_BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte aligned non-null pointer (host memory: never to be launched on)

# positions in the argument lists below (the device in front and the stream behind are added by refused())
IN0, C0, IN1, C1, B, HIN, WIN, UP, WGT, BIAS, COUT, KH, KW, ACT, POOL, RESID, SPLITK, TILE, OUT, ITERS, AVG, PRE_S, PRE_T, OUT2, S2, T2, NCHW, \
    SPLIT_N = range(28)
# a 3x3 convolution 64 -> 64 on 1 x 8 x 8 that passes every check (never called as it is)
CONV = [P, 64, None, 0, 1, 8, 8, 0, P, P, 64, 3, 3, 0, 0, None, 0, 0, P, 0, None, None, None, None, None, None, 0, 0]
# x, scale, shift, B, H, W, C, tile, V
TRANSFORM = [P, None, None, 1, 8, 8, 64, 4, P]
# feat, deformation, occlusion, n, ns, hf, wf, C, h, w, out, iters, avg_ms, out2, scale2, shift2
WARP = [P, P, P, 2, 1, 8, 8, 32, 8, 8, P, 0, None, P, P, P]

GEMM_TILES = (0, 32, 64, 128, 1001, 1002, 1003, 1004, 1005)
WINO_TILES = (2000, 2100, 2103, 2106, 2152, 2153, 2156)
OTHER_TILES = (3000, 3003, 3004, 4000, 4001, 4002)


def refused(name, args):
    L = _lib.lib()
    code = getattr(L, name)(0, *args, None)
    return code == _lib.ERR_ARG and L.eamm_last_error(None).decode().startswith(name + ":")


def conv(**at):
    args = list(CONV)
    for k, v in at.items():
        args[globals()[k.upper()]] = v
    return args


def at(base, **changes):
    args = list(base)
    for k, v in changes.items():
        args[int(k[1:])] = v
    return args


def test_the_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "eamm_hip.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == nargs == m.group(1).count(",") + 1, name
    assert len(CONV) == 28 and len(TRANSFORM) == 9 and len(WARP) == 16
    assert len(_lib.SIGNATURES["eamm_op_conv_ex"][1]) == len(_lib.SIGNATURES["eamm_op_conv"][1]) + 7
    assert len(_lib.SIGNATURES["eamm_op_warp_ex"][1]) == len(_lib.SIGNATURES["eamm_op_warp"][1]) + 3
    assert "#define EAMM_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6


def test_conv_ex_refuses_null_pointers():
    for k in ("in0", "wgt", "bias", "out"):
        assert refused("eamm_op_conv_ex", conv(**{k: None})), k


def test_pre_activation_belongs_to_the_winograd_transform():
    for tile in WINO_TILES:                                                   # one without the other
        assert refused("eamm_op_conv_ex", conv(tile=tile, pre_s=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, pre_t=P)), tile
    for tile in GEMM_TILES + OTHER_TILES + (5, 1000, 1006, 2200):
        assert refused("eamm_op_conv_ex", conv(tile=tile, pre_s=P, pre_t=P, up=int(tile in (3000, 3003, 3004)))), tile


def test_the_gemm_modes_belong_to_the_implicit_gemm():
    for tile in WINO_TILES + OTHER_TILES + (5, 1000, 1006, 2200):
        up = int(tile in (3000, 3003, 3004))
        assert refused("eamm_op_conv_ex", conv(tile=tile, up=up, out2=P, s2=P, t2=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, up=up, nchw=1)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, up=up, cout=36, out2=P, split_n=32)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, up=up, s2=P, t2=P)), tile


def test_the_second_output_needs_scale_and_shift():
    for tile in GEMM_TILES:
        assert refused("eamm_op_conv_ex", conv(tile=tile, out2=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, out2=P, s2=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, out2=P, t2=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, s2=P, t2=P)), tile          # nothing to write them to
    assert refused("eamm_op_conv_ex", conv(nchw=2)) and refused("eamm_op_conv_ex", conv(nchw=-1))


def test_the_float4_operands_must_be_aligned():
    for tile in WINO_TILES:
        assert refused("eamm_op_conv_ex", conv(tile=tile, pre_s=P + 4, pre_t=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, pre_s=P, pre_t=P + 8)), tile
    for tile in GEMM_TILES:
        for k in ("out2", "s2", "t2"):
            assert refused("eamm_op_conv_ex", conv(tile=tile, **{**dict(out2=P, s2=P, t2=P), k: P + 4})), (tile, k)
        assert refused("eamm_op_conv_ex", conv(tile=tile, up=1, cout=36, out2=P + 12, split_n=32)), tile


def test_pool_combines_with_none_of_resid_nchw_out2_split_n():
    for tile in GEMM_TILES + (2152, 2153, 2156):
        assert refused("eamm_op_conv_ex", conv(tile=tile, pool=1, resid=P)), tile
    for tile in GEMM_TILES:
        assert refused("eamm_op_conv_ex", conv(tile=tile, pool=1, nchw=1)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, pool=1, out2=P, s2=P, t2=P)), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, pool=1, cout=36, out2=P, split_n=32)), tile
    # ... and eamm_op_conv itself, under its own name
    plain = conv(pool=1, resid=P)[:AVG + 1]
    assert refused("eamm_op_conv", plain)
    assert refused("eamm_op_conv", conv(tile=1001, pool=1, resid=P)[:AVG + 1])


def test_each_rule_of_split_n():
    good = dict(cout=36, out2=P, split_n=32, up=1)
    for tile in (0, 1003):
        assert refused("eamm_op_conv_ex", conv(tile=tile, **{**good, "out2": None})), tile            # out2 given
        assert refused("eamm_op_conv_ex", conv(tile=tile, **good, resid=P)), tile                     # no resid
        assert refused("eamm_op_conv_ex", conv(tile=tile, **{**good, "up": 0}, pool=1)), tile         # no pool
        assert refused("eamm_op_conv_ex", conv(tile=tile, **good, nchw=1)), tile                      # no nchw
        assert refused("eamm_op_conv_ex", conv(tile=tile, **{**good, "cout": 32})), tile              # split_n < Cout
        assert refused("eamm_op_conv_ex", conv(tile=tile, **{**good, "cout": 31})), tile
        assert refused("eamm_op_conv_ex", conv(tile=tile, **{**good, "cout": 37})), tile              # Cout <= split_n + 4
        assert refused("eamm_op_conv_ex", conv(tile=tile, **{**good, "split_n": -32})), tile


def test_one_by_one_filters_only_on_the_register_staged_kernel():
    one = dict(kh=1, kw=1)
    for tile in (1001, 1002, 1003, 1004, 1005) + WINO_TILES + OTHER_TILES:
        assert refused("eamm_op_conv_ex", conv(tile=tile, **one)), tile
    for tile in (0, 32, 64, 128):
        assert refused("eamm_op_conv_ex", conv(tile=tile, **one, up=1)), tile
    assert refused("eamm_op_conv_ex", conv(kh=1, kw=3)) and refused("eamm_op_conv_ex", conv(kh=3, kw=1))
    assert refused("eamm_op_conv", conv(tile=1001, **one)[:AVG + 1])
    assert refused("eamm_op_conv_ex", conv(c0=48)) and refused("eamm_op_conv_ex", conv(in1=P, c1=16))


def test_wino_transform_refuses_what_the_launches_cannot_run():
    name = "eamm_op_wino_transform"
    for i in (0, 8):
        assert refused(name, at(TRANSFORM, **{f"a{i}": None})), i                    # NULL x / V
        assert refused(name, at(TRANSFORM, **{f"a{i}": P + 4})), i                   # a misaligned float4 pointer
    for i in (3, 4, 5, 6):
        for v in (0, -1, -4):
            assert refused(name, at(TRANSFORM, **{f"a{i}": v})), (i, v)
    for tile in (0, 1, 3, 6, 8, -2):
        assert refused(name, at(TRANSFORM, a7=tile)), tile
    assert refused(name, at(TRANSFORM, a4=6)) and refused(name, at(TRANSFORM, a5=10))                 # tile 4: H, W % 4
    assert refused(name, at(TRANSFORM, a7=2, a4=3)) and refused(name, at(TRANSFORM, a7=2, a5=7))      # tile 2: H, W % 2
    for tile in (2, 4):
        for c in (1, 2, 6, 30, 33):
            assert refused(name, at(TRANSFORM, a7=tile, a6=c)), (tile, c)
        assert refused(name, at(TRANSFORM, a7=tile, a1=P)), tile                     # scale without shift
        assert refused(name, at(TRANSFORM, a7=tile, a2=P)), tile
        assert refused(name, at(TRANSFORM, a7=tile, a1=P + 8, a2=P)), tile
        # 2^31 output elements and more: tile 4 writes 36 / 16 per input element, tile 2 writes 4
        assert refused(name, at(TRANSFORM, a7=tile, a3=1024, a4=1024, a5=1024, a6=64)), tile
    assert refused(name, at(TRANSFORM, a7=2, a3=1, a4=4096, a5=4096, a6=32))          # 16 * 2^22 * 32 = 2^31 exactly
    assert refused(name, at(TRANSFORM, a7=4, a3=8, a4=4096, a5=4096, a6=8))           # 36 * 2^23 * 8 > 2^31


def test_warp_ex_takes_all_three_or_none():
    name = "eamm_op_warp_ex"
    for i in (13, 14, 15):
        assert refused(name, at(WARP, **{f"a{i}": None})), i
    assert refused(name, at(WARP, a13=None, a14=None)) and refused(name, at(WARP, a13=None, a15=None))
    for i in (0, 1, 10):
        assert refused(name, at(WARP, **{f"a{i}": None})), i
    assert refused(name, at(WARP, a7=12)) and refused(name, at(WARP, a7=4)) and refused(name, at(WARP, a4=3))
    for i in (3, 5, 6, 8, 9):
        assert refused(name, at(WARP, **{f"a{i}": 0})), i
