"""Every operator entry (eamm_op_*, eamm_disc_*, eamm_equi_*, include/eamm_hip.h) refuses an all-NULL, all-zero call with
EAMM_ERR_ARG and a message that starts with its own name, before it touches a device -- the argument check comes first in each
entry, so this runs without a GPU.  An entry that lost its check, or two entries whose messages were swapped, fail here."""
import ctypes

import pytest

from eamm_amd import _lib
from guarded import OPERATOR_FAMILIES

# not eamm_bn_*: that family takes no device argument and reports through eamm_bn_last_error, with messages that carry no entry name
FAMILIES = tuple(f for f in OPERATOR_FAMILIES if f != "eamm_bn_")
# takes no refusable argument (a device and a stream): an all-zero call would open device 0 and wait for its NULL stream
NO_ARGUMENT_CHECK = {"eamm_op_lstm_check"}

OP_ENTRIES = sorted(n for n, (res, _) in _lib.SIGNATURES.items()
                    if n.startswith(FAMILIES) and res is ctypes.c_int and n not in NO_ARGUMENT_CHECK)
WORKSPACE_QUERIES = sorted(n for n in _lib.SIGNATURES if n.startswith(FAMILIES) and n.endswith("_workspace_floats"))


def zeros(name):
    """NULL for every pointer argument, 0 for every number."""
    return [0.0 if t is ctypes.c_float else 0 if t in (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint64) else None
            for t in _lib.SIGNATURES[name][1]]


def test_the_lists_are_not_empty():
    assert len(OP_ENTRIES) >= 53 + 4 + 3 and len(WORKSPACE_QUERIES) >= 13 + 4         # + eamm_disc_*, eamm_equi_*
    assert all(_lib.SIGNATURES[n][0] is ctypes.c_size_t for n in WORKSPACE_QUERIES)


@pytest.mark.parametrize("name", OP_ENTRIES)
def test_an_all_zero_call_is_refused_under_the_entrys_own_name(name):
    L = _lib.lib()
    assert getattr(L, name)(*zeros(name)) == _lib.ERR_ARG
    assert L.eamm_last_error(None).decode().startswith(name + ":")


@pytest.mark.parametrize("name", WORKSPACE_QUERIES)
def test_a_workspace_query_of_an_empty_shape_is_zero(name):
    assert getattr(_lib.lib(), name)(*zeros(name)) == 0
