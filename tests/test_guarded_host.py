"""tests/guarded.py on CPU tensors (placement arithmetic, both skews, the band-width rule, what check() reports) and the
completeness of its registry once every registering module is imported: every entry of ``guarded.OPERATOR_FAMILIES`` that takes a
pointer has a guarded case or a stated reason for having none.  No GPU."""
import ctypes as C

import pytest
import torch

import guarded
from guarded import ALIGN, GUARD_WORD, MAX_BAND, MIN_BAND, Arena, Plain, band_bytes, same_outputs


def test_band_width_rule():
    assert band_bytes(0) == band_bytes(4) == band_bytes(MIN_BAND) == MIN_BAND == 64 << 10
    assert band_bytes(MIN_BAND + 1) == MIN_BAND + ALIGN                     # the operand's own size, in whole 256-byte units
    assert band_bytes(3 << 20) == 3 << 20
    assert band_bytes(MAX_BAND) == band_bytes(1 << 30) == MAX_BAND == 16 << 20


@pytest.mark.parametrize("skew", [0, 16])
def test_placement_arithmetic(skew):
    arena = Arena("cpu", skew=skew, chunk=4 << 20)
    data = torch.arange(1155, dtype=torch.float32)
    views = [arena.place(data, "in", name="a"), arena.place((3, 5, 7), "out", name="b"), arena.place(100000, "work", name="w"),
             arena.place(torch.ones(2, 3), "inout", name="io"), arena.place((5, 7, 3), "out", dtype=torch.uint8, name="bytes"),
             arena.place(torch.zeros(1, dtype=torch.int32), "inout", name="flag")]
    for v, rec in zip(views, arena.records):
        assert v.data_ptr() % ALIGN == skew and v.is_contiguous() and v.data_ptr() == rec["view"].data_ptr()
        own = v.numel() * v.element_size()
        lead, trail = rec["lead"], rec["trail"]
        base = rec["base"].data_ptr()
        assert base + lead[1] == v.data_ptr() and lead[1] - lead[0] == band_bytes(own) + skew
        assert trail[1] - trail[0] >= band_bytes(own) and trail[0] - (lead[1] + own) < 4
        assert (base + lead[0]) % ALIGN == 0 and (base + trail[1]) % ALIGN == 0
    assert tuple(views[1].shape) == (3, 5, 7) and tuple(views[2].shape) == (100000,) and views[4].dtype == torch.uint8
    assert torch.equal(views[0], data) and torch.equal(views[3], torch.ones(2, 3))
    # "out" and "work" views start as the guard pattern: a NaN that names itself
    for v in (views[1], views[2]):
        assert bool(torch.isnan(v).all()) and bool((v.view(torch.int32) == GUARD_WORD).all())
    # views do not overlap, nor does a view overlap another's bands
    spans = sorted((r["base"].data_ptr() + r["lead"][0], r["base"].data_ptr() + r["trail"][1]) for r in arena.records)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    for v in views[1:3] + views[4:5]:
        v.fill_(1)
    arena.check()
    with pytest.raises(AssertionError):
        Arena("cpu", skew=4)
    with pytest.raises(AssertionError):
        arena.place(8, "out", skew=8)


def test_an_operand_larger_than_a_chunk_gets_a_buffer_of_its_own():
    arena = Arena("cpu", skew=16, chunk=1 << 20)
    small, big = arena.place(10, "out", name="small"), arena.place(1 << 19, "work", name="big")      # 2 MiB with 2 MiB bands
    assert arena.records[0]["base"].data_ptr() != arena.records[1]["base"].data_ptr()
    assert big.data_ptr() % ALIGN == 16 and small.data_ptr() % ALIGN == 16
    small.fill_(0)
    arena.check()


@pytest.mark.parametrize("skew", [0, 16])
def test_a_write_beside_a_view_is_reported_with_operand_side_and_offset(skew):
    arena = Arena("cpu", skew=skew, chunk=4 << 20)
    arena.place(torch.zeros(40), "in", name="first")
    out = arena.place((6, 7), "out", name="second")
    out.fill_(0)
    arena.check()
    rec = arena.records[1]
    words = rec["base"].view(torch.int32) if rec["base"].data_ptr() % 4 == 0 else None
    assert words is not None
    after, before = rec["trail"][0] // 4, rec["lead"][1] // 4 - 1
    words[after] = 0                                        # one element past the end, through the arena's base buffer
    damage = arena.damage()
    assert [(d["name"], d["side"], d["first"], d["last"], d["count"]) for d in damage] == [("second", "after", 0, 0, 1)]
    with pytest.raises(AssertionError, match=r"guard after operand 'second' damaged: 1 words, offsets 0\.\.0 of the band \(0 to 3 bytes past its end\)"):
        arena.check()
    words[after] = guarded._as_int32(GUARD_WORD)
    arena.check()
    words[before] = 1                                       # one element before the start
    band = (rec["lead"][1] - rec["lead"][0]) // 4
    damage = arena.damage()
    assert [(d["name"], d["side"], d["first"], d["last"]) for d in damage] == [("second", "before", band - 1, band - 1)]
    with pytest.raises(AssertionError, match="guard before operand 'second' damaged: 1 words.*4 to 8 bytes before its start|guard before operand 'second'"):
        arena.check()
    words[before] = guarded._as_int32(GUARD_WORD)
    words[after + 5], words[after + 9] = 7, 7               # first and last damaged offset
    (d,) = arena.damage()
    assert (d["first"], d["last"], d["count"]) == (5, 9, 2)


def test_a_changed_input_and_a_nan_output_are_reported():
    arena = Arena("cpu", skew=16, chunk=4 << 20)
    x = arena.place(torch.tensor([1.0, float("nan"), 3.0]), "in", name="x")         # a NaN in the data is no change
    io = arena.place(torch.ones(4), "inout", name="io")
    y, ws = arena.place(5, "out", name="y"), arena.place(5, "work", name="ws")
    with pytest.raises(AssertionError, match="output operand 'y' holds NaN"):
        arena.check()
    arena.check(nan_ok=("y",))
    y.fill_(2)
    io.fill_(5)                                             # "inout" may change, a workspace may stay NaN
    arena.check()
    x[2] = 4.0
    assert arena.changed_inputs() == ["x"]
    with pytest.raises(AssertionError, match="input operand 'x' was written to"):
        arena.check()


def test_plain_placement_is_what_the_tests_did_and_outputs_compare_bit_for_bit():
    plain, arena = Plain("cpu"), Arena("cpu", skew=16, chunk=4 << 20)
    src = torch.arange(6.0)
    for p in (plain, arena):
        a, o, w = p(src, "in"), p((2, 3), "out", name="o"), p(7, "work")
        o8 = p((3,), "out", dtype=torch.uint8)
        io = p(torch.zeros(2), "inout")
        assert torch.equal(a, src) and bool(torch.isnan(o).all()) and tuple(w.shape) == (7,)
        assert bool((o8 == 255).all()) if p is plain else o8.tolist() == [0xA5, 0xA5, 0xC5]     # 0xFF bytes; the guard word's own, little-endian
        o[0] = a[:3]                                        # the second row stays unwritten: torch's NaN there, a guard word here
        io += 1
        o8.fill_(9)                                         # (an unwritten integer element has no NaN to be equal as: it differs)
    assert plain(src, "in") is src                         # .to(device) of a tensor that is there already
    assert [n for n, _ in plain.outs] == [n for n, _ in arena.outs] == ["o", "out3", "inout4"]
    assert same_outputs(plain, arena) == []
    arena.outs[0][1][0, 1] = -1.0
    assert same_outputs(plain, arena) == ["o"]


# ---- completeness of the guarded registry ----------------------------------------------------------------------------------------
def test_every_operator_entry_with_a_pointer_has_a_guarded_case_or_a_reason():
    from eamm_amd import _lib
    import test_gpu_guarded_ops as g            # imports every module that registers cases, and shows the registry
    need = [name for name, (_, args) in _lib.SIGNATURES.items()
            if name.startswith(guarded.OPERATOR_FAMILIES) and any(a is C.c_void_p for a in args)]
    count = lambda *prefixes: sum(n.startswith(prefixes) for n in need)
    assert (count("eamm_op_", "eamm_bn_"), count("eamm_disc_"), count("eamm_equi_")) == (75, 4, 3) and len(need) == 82, need
    assert sum(n in g.GUARDED for n in need) == 81 and "eamm_op_lstm_check" in g.EXEMPT and "eamm_final_split_planes" in g.EXEMPT
    missing = [n for n in need if n not in g.GUARDED and n not in g.EXEMPT]
    assert not missing, ("entries with neither a guarded case registered in tests/guarded.py nor a reason in its EXEMPT", missing)
    assert not [n for n in g.EXEMPT if n in g.GUARDED], "an entry is either guarded or exempt"
    assert all(n in _lib.SIGNATURES and isinstance(why, str) and len(why) > 10 for n, why in g.EXEMPT.items())
    assert all(ids and all(i in g.CASES for i in ids) for ids in g.GUARDED.values())
    # every case runs: the GPU test is parametrised over the whole registry
    assert sorted(g.CASES) == sorted({i for ids in g.GUARDED.values() for i in ids})
    # the size queries take no pointer; each discriminator entry with a workspace has one
    assert all(n + "_workspace_floats" in _lib.SIGNATURES for n in need if n.startswith("eamm_disc_"))
