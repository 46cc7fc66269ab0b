"""Every discriminator entry (eamm_disc_*) that takes a pointer between poisoned guard bands (tests/guarded.py), as
tests/test_gpu_guarded_ops.py does for the other families: each case of tests/test_gpu_disc_ops.py runs on plain tensors, in an arena
whose views start on a 256-byte boundary and in one whose views start 16 bytes past it.  After a guarded run no guard word has
changed, no input was written to, no output holds a NaN, and every output is bit-equal to the plain run's.

``GUARDED`` maps an entry of ``_lib.SIGNATURES`` to the cases that cover it; tests/test_discriminator_host.py checks that it is
complete."""
import pytest
import torch

import test_gpu_disc_ops as ops
from guarded import Arena, Plain, same_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_CONV = ["fwd_mtail", "fwd_one_pixel", "fwd_row_past_tile", "fwd_two_mtiles_n96", "dgrad", "dgrad_small_map", "dgrad_thin4", "dgrad_thin16", "thin4", "thin8",
         "thin16", "thin16_rubbish"]
_WGRAD = ["wgrad_ragged_split", "wgrad_one_pixel", "wgrad_row_past_tile", "wgrad_thin4", "wgrad_thin8", "wgrad_thin16"]
_NORM = ["norm_pool_odd", "norm_nopool", "block0_pool", "block0_nopool", "norm_two_values", "norm_many_ranges"]
GUARDED = {
    "eamm_disc_conv4": _CONV,
    "eamm_disc_conv4_wgrad": _WGRAD,
    "eamm_disc_norm_act_pool": _NORM,
    "eamm_disc_norm_act_pool_backward": _NORM,
}
EXEMPT = {}      # entries that take a pointer but have no guarded case, with the reason: none
CASES = sorted({c for ids in GUARDED.values() for c in ids})


@pytest.mark.parametrize("cid", CASES)
def test_case_between_guard_bands(cid):
    fn = ops.CASES[cid]
    plain = Plain(DEV)
    fn(place=plain)
    torch.cuda.synchronize()
    for skew in (0, 16):
        arena = Arena(DEV, skew=skew)
        fn(place=arena)
        torch.cuda.synchronize()
        arena.check()
        assert same_outputs(plain, arena) == [], (cid, f"skew {skew}: outputs differ from the plain call")
