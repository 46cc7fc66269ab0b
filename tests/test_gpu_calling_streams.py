"""Every case of the guard-band registry (tests/guarded.py ``CASES``) once more, on a side stream whose inputs exist in that stream's
order only (``guarded.run_late``).  An entry that put one memset, packing launch or reduction on the null stream instead of the
caller's would pass every test that runs on the default stream with nothing else in flight; here that launch runs ahead of the
delayed copies, reads NaN or is overwritten, and the outputs differ from the plain run's.

A case proves something only if the side stream was still held when the case first called the library on placed operands (a few
cases first make an input with a public operator on tensors of their own, as they do in an arena run): ``run_late`` notes that at the
entry itself and fails the case by name otherwise (``guarded.UNOBSERVED`` lists the cases where it cannot be seen, with the reason).
The side stream does not synchronise implicitly with the null stream: ``test_the_side_stream_is_non_blocking`` reads its flags from
the runtime.  One case runs at a time, so no LSTM case ever runs beside another LSTM launch.

Like tests/test_gpu_guarded_ops.py this file is run one family at a time on a machine with a GPU (``-k conv-``, ``-k warp-``,
``-k infer-``, ``-k train-``, ``-k emo-``, ``-k audio-``, ``-k kp-``, ``-k motion-``, ``-k perc-``, ``-k bn-``, ``-k modes-``, ``-k clip-``,
``-k disc-``, ``-k equi-``): a launch in the wrong stream is the failure it exists to find, and a family that has one should not be
followed by another."""
import ctypes as C

import pytest
import torch

import guarded
import test_gpu_guarded_ops  # noqa: F401  (imports every module that registers cases)
from guarded import CASES, UNOBSERVED, run_late

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_the_side_stream_is_non_blocking():
    side = guarded.side_stream(DEV)
    flags = C.c_uint(0)
    assert C.CDLL("libamdhip64.so").hipStreamGetFlags(C.c_void_p(side.cuda_stream), C.byref(flags)) == 0
    assert flags.value & 1, "hipStreamNonBlocking is not set: the side stream would wait for the null stream"
    assert side.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream


def test_a_late_operand_exists_in_the_side_streams_order_only():
    """The placer itself: NaN until the side stream gets there, the data afterwards; the event behind the delay is pending meanwhile."""
    side = guarded.side_stream(DEV)
    late = guarded.Late(DEV, side)
    data = torch.arange(1000.0)
    with torch.cuda.stream(side):
        v = late.place(data, "in")
        out = late.place((10,), "out", name="o")
        with torch.cuda.stream(torch.cuda.default_stream(DEV)):       # the default stream reads at once, ahead of the delayed copy
            early = v.clone()
            torch.cuda.current_stream().synchronize()
        pending = not late.started.query()
    assert pending and bool(torch.isnan(early).all())
    side.synchronize()
    assert late.started.query() and torch.equal(v.cpu(), data) and bool(torch.isnan(out).all())
    assert [n for n, _ in late.outs] == ["o"]


def test_the_unobserved_cases_are_few_and_have_reasons():
    assert len(UNOBSERVED) <= 5 and all(cid in CASES and isinstance(why, str) and len(why) > 10 for cid, why in UNOBSERVED.items())


@pytest.mark.parametrize("cid", list(CASES))
def test_late(cid):
    run_late(cid, DEV)
