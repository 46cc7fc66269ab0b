"""Guard-band placement of operator operands: every tensor a test hands to the library is a view into a large buffer (``torch.empty``;
the arena takes a further one when the first is full), between two bands of a NaN pattern, at the weakest alignment include/eamm_hip.h
documents.  A store past an output or a workspace damages a
band, a load past an input brings a NaN into the result, and a kernel that needs more alignment than documented meets a pointer
that is 16 bytes off a 256-byte boundary.  Plain helper module: no pytest hooks, no fixtures, works on CPU tensors as well.

    arena = Arena("cuda:0", skew=16)
    x = arena.place(host_tensor, "in")          # a copy of the data
    y = arena.place((n, h, w, c), "out")        # NaN-filled
    ws = arena.place(n_floats, "work")          # NaN-filled: a read before the first write shows
    ... launch ...; torch.cuda.synchronize()
    arena.check()

``Plain(device)`` has the same call signature and does what the tests did before there was an arena (``.to(device)``,
``torch.full(nan)``); the case helpers take either as their ``place=`` argument.  Both remember the "out" and "inout" views they
handed out, in order, so that two runs of one case can be compared bit for bit (``same_outputs``).

The registry: a guarded case is a function of ``place`` that calls entries on placed operands and makes its own comparison.  The
test files that define such cases register them with ``case`` at import: ``CASES`` holds them by id, ``GUARDED`` maps an entry of
``_lib.SIGNATURES`` to the ids of its cases, ``EXEMPT`` maps an entry without one to the reason.  ``run_three`` is the one driver.
tests/test_gpu_guarded_ops.py imports every registering module and runs the whole registry; tests/test_guarded_host.py checks that
every entry of ``OPERATOR_FAMILIES`` that takes a pointer is guarded or exempt.

``Late(device, stream)`` is a third placer and ``run_late`` its driver: the same cases with inputs that exist in a side stream's
order only, against the plain run's bits (tests/test_gpu_calling_streams.py) -- what an entry launches on another stream than the
caller's shows there.  No guard bands in that run: the arena runs have looked for stray stores already.

A new handle-less operator family joins by adding its prefix to ``OPERATOR_FAMILIES`` and registering its cases (a new module is
added to the imports at the end of test_gpu_guarded_ops.py); tests/test_op_entries_host.py's all-zero refusal check then covers it too."""
import torch

GUARD_WORD = 0x7FC5A5A5          # a quiet NaN with a payload: poisons what reads it, and is recognisable in a dump
MIN_BAND = 64 << 10              # covers a row-pitch or tile overrun beside a small operand
MAX_BAND = 16 << 20
ALIGN = 256                      # a view starts at 0 mod ALIGN, plus the skew
SKEWS = (0, 16)                  # 16 bytes is what the header documents; nothing below it is ever launched on
ROLES = ("in", "out", "inout", "work")
CHUNK = 64 << 20                 # the arena grows by buffers of at least this size; an operand and its bands lie in one of them

# the handle-less operator families: every entry of theirs that takes a pointer is guarded or exempt
OPERATOR_FAMILIES = ("eamm_op_", "eamm_bn_", "eamm_disc_", "eamm_equi_")
CASES = {}        # id -> (function of place, names of outputs that may stay NaN, names of outputs exempt from bit-equality)
GUARDED = {}      # entry -> [case ids]
# entries that take a pointer argument but have no guarded case, with the reason
EXEMPT = {
    "eamm_op_lstm_check": "no tensor: its pointer argument is the stream",
    "eamm_final_split_planes": "host pointers only: it packs the final layer's filter on the CPU",
}


def band_bytes(own_bytes):
    """At least the operand's own size (an index one image or one slab too far), at least 64 KiB, at most 16 MiB; whole 256-byte
    units so that the next view's alignment is independent of it."""
    n = min(MAX_BAND, max(MIN_BAND, int(own_bytes)))
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _shape_of(t_or_shape):
    if isinstance(t_or_shape, int):
        return (t_or_shape,)
    return tuple(t_or_shape.shape) if isinstance(t_or_shape, torch.Tensor) else tuple(int(s) for s in t_or_shape)


def _fill_value(dtype):
    """What an "out" view starts as outside an arena: NaN, or all-ones bits for an integer type (as the uint8 frame tests do)."""
    return float("nan") if dtype.is_floating_point else -1 if dtype.is_signed else torch.iinfo(dtype).max


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


class Plain:
    """The placement the tests used before: a fresh tensor per operand."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.placed = 0
        self.outs = []

    def place(self, t_or_shape, role, dtype=torch.float32, skew=0, name=None):
        assert role in ROLES, role
        name = name or f"{role}{self.placed}"
        self.placed += 1
        if role in ("in", "inout"):
            v = t_or_shape.to(self.device)
        elif role == "out":
            v = torch.full(_shape_of(t_or_shape), _fill_value(dtype), dtype=dtype, device=self.device)
        else:
            v = torch.empty(_shape_of(t_or_shape), dtype=dtype, device=self.device)
        if role in ("out", "inout"):
            self.outs.append((name, v))
        return v

    __call__ = place


class Arena:
    def __init__(self, device, skew=0, chunk=CHUNK):
        assert skew in SKEWS, skew
        self.device = torch.device(device)
        self.skew = skew
        self.chunk = chunk
        self.base = None                                # the buffer the next operand goes into
        self.records = []
        self.outs = []

    def _grow(self, need):
        self.base = torch.empty(max(self.chunk, need + ALIGN), dtype=torch.uint8, device=self.device)
        self.origin = (-self.base.data_ptr()) % ALIGN   # offset of the first 256-byte boundary
        self.top = self.origin

    @staticmethod
    def _words(base, lo, hi):
        return base[lo:hi].view(torch.int32)

    def place(self, t_or_shape, role, dtype=torch.float32, skew=None, name=None):
        assert role in ROLES, role
        skew = self.skew if skew is None else skew
        assert skew in SKEWS, skew
        data = None
        if role in ("in", "inout"):
            data = t_or_shape.detach().contiguous()
            dtype = data.dtype
        shape = _shape_of(t_or_shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        band = band_bytes(nbytes)
        if self.base is None or self.top + 2 * band + nbytes + 2 * ALIGN > self.base.numel():
            self._grow(2 * band + nbytes + 2 * ALIGN)
        lead = self.top                                  # 0 mod 256
        start = lead + band + skew                       # the leading band is `band + skew` bytes wide
        end = start + nbytes
        trail_end = self.origin + (end - self.origin + band + ALIGN - 1) // ALIGN * ALIGN
        assert trail_end <= self.base.numel()
        trail = (end + 3) // 4 * 4                       # a byte tensor may end inside a guard word: those bytes are compared apart
        self.top = trail_end
        self._words(self.base, lead, trail_end).fill_(_as_int32(GUARD_WORD))       # bands and the view itself: NaN before any data
        view = self.base[start:end].view(dtype).view(shape)
        assert view.data_ptr() % ALIGN == skew and view.is_contiguous()
        if data is not None:
            view.copy_(data)
        name = name or f"{role}{len(self.records)}"
        rec = dict(name=name, role=role, view=view, base=self.base, lead=(lead, start), trail=(trail, trail_end), odd=(end, trail),
                   odd_bytes=self.base[end:trail].cpu().clone(),
                   snapshot=_bits(data).cpu().clone() if role == "in" else None)
        self.records.append(rec)
        if role in ("out", "inout"):
            self.outs.append((name, view))
        return view

    __call__ = place

    def damage(self):
        """One entry per damaged guard band: operand name, side ("before" / "after"), the first and last damaged 4-byte word counted
        from the band's low end, and how many words differ."""
        found = []
        for rec in self.records:
            for side, (lo, hi) in (("before", rec["lead"]), ("after", rec["trail"])):
                bad = self._words(rec["base"], lo, hi) != _as_int32(GUARD_WORD)
                if bool(bad.any()):
                    idx = bad.nonzero().reshape(-1)
                    found.append(dict(name=rec["name"], side=side, first=int(idx[0]), last=int(idx[-1]), count=int(idx.numel()),
                                      band_words=(hi - lo) // 4))
            lo, hi = rec["odd"]
            if hi > lo and not torch.equal(rec["base"][lo:hi].cpu(), rec["odd_bytes"]):
                found.append(dict(name=rec["name"], side="after, in the bytes that fill its last word", first=0, last=0, count=1, band_words=1))
        return found

    def changed_inputs(self):
        return [rec["name"] for rec in self.records
                if rec["role"] == "in" and not torch.equal(_bits(rec["view"]).cpu(), rec["snapshot"])]

    def nan_outputs(self, nan_ok=()):
        return [rec["name"] for rec in self.records
                if rec["role"] == "out" and rec["name"] not in nan_ok and rec["view"].dtype.is_floating_point
                and bool(torch.isnan(rec["view"]).any())]

    def check(self, nan_ok=()):
        """After the device has finished (``torch.cuda.synchronize()``): no guard word changed, no "in" view changed, no NaN left in
        an "out" view other than those named in ``nan_ok``."""
        lines = []
        for d in self.damage():
            where = (f"{(d['band_words'] - d['last']) * 4} to {(d['band_words'] - d['first']) * 4} bytes before its start"
                     if d["side"] == "before" else f"{d['first'] * 4} to {d['last'] * 4 + 3} bytes past its end")
            lines.append(f"guard {d['side']} operand {d['name']!r} damaged: {d['count']} words, offsets {d['first']}..{d['last']} "
                         f"of the band ({where})")
        lines += [f"input operand {n!r} was written to" for n in self.changed_inputs()]
        lines += [f"output operand {n!r} holds NaN (unwritten, or computed from a guard word)" for n in self.nan_outputs(nan_ok)]
        assert not lines, "; ".join(lines)


def _as_int32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def _same_bits(x, y):
    """Bit-equal, a NaN of any payload equal to a NaN: an element nobody wrote is torch's NaN in one run and a guard word in the other."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    x, y = x.detach().cpu(), y.detach().cpu()
    if x.dtype.is_floating_point:
        nx, ny = torch.isnan(x), torch.isnan(y)
        if not torch.equal(nx, ny):
            return False
        x, y = torch.where(nx, torch.zeros_like(x), x), torch.where(ny, torch.zeros_like(y), y)
    return torch.equal(_bits(x), _bits(y))


def same_outputs(a, b):
    """Names of the "out" / "inout" operands of two placers' runs of one case that are not bit-identical."""
    assert [n for n, _ in a.outs] == [n for n, _ in b.outs], "the two runs placed different outputs"
    return [n for (n, x), (_, y) in zip(a.outs, b.outs) if not _same_bits(x, y)]


def case(cid, entries, fn=None, nan_ok=(), unstable=()):
    """Register ``fn(place)`` as case ``cid`` covering ``entries`` (full names).  Usable as a decorator when ``fn`` is None."""
    def register(f):
        from eamm_amd import _lib      # here, so that the placement helpers above need nothing but torch
        assert cid not in CASES, cid
        CASES[cid] = (f, tuple(nan_ok), tuple(unstable))
        for e in entries:
            assert e in _lib.SIGNATURES, e
            GUARDED.setdefault(e, []).append(cid)
        return f
    return register if fn is None else register(fn)


# ---- the same cases in a side stream's order only ----------------------------------------------------------------------------------
DELAY_MS = 100.0         # how long the side stream is held before a case's inputs are copied in: an order of magnitude above the host
                         # work between a case's first placement and its first library call (placements, size queries, pinned copies)
# cases whose first library call cannot be seen pending (at most 5), with the reason
UNOBSERVED = {}
_ticks_per_ms = {}


def _non_blocking_stream(device):
    """torch creates its streams non-blocking; that is confirmed through hipStreamGetFlags, and where it does not hold a
    hipStreamNonBlocking stream of the runtime's is wrapped instead."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    non_blocking = 1                                     # hipStreamNonBlocking
    st = torch.cuda.Stream(device=device)
    flags = C.c_uint(0xFFFFFFFF)
    rc = hip.hipStreamGetFlags(C.c_void_p(st.cuda_stream), C.byref(flags))
    assert rc == 0, ("hipStreamGetFlags", rc)
    if flags.value & non_blocking:
        return st
    raw = C.c_void_p()
    with torch.cuda.device(device):
        rc = hip.hipStreamCreateWithFlags(C.byref(raw), C.c_uint(non_blocking))
    assert rc == 0, ("hipStreamCreateWithFlags", rc)
    return torch.cuda.ExternalStream(raw.value, device=device)


def _holds_up_the_default_stream(stream, hold_ms=20.0):
    """Whether work on the default stream waits for earlier work on ``stream``.  A non-blocking stream never makes it wait by rule,
    but the runtime multiplexes its streams onto a few hardware queues (four by default), and a stream that shares the null stream's
    queue delays it all the same: a ``Late`` placer's NaN fills would then sit out the delay they are meant to precede."""
    import time
    default = torch.cuda.default_stream(stream.device)
    probe = torch.zeros(1, device=stream.device)
    torch.cuda.synchronize(stream.device)
    _delay(stream, hold_ms)
    begun = time.perf_counter()
    with torch.cuda.stream(default):
        probe.add_(1)
    default.synchronize()
    waited_ms = (time.perf_counter() - begun) * 1e3
    stream.synchronize()
    return waited_ms > hold_ms / 2


_side_streams = {}


def side_stream(device):
    """THE side stream of ``device`` for these runs (one per process): non-blocking, so that it does not synchronise implicitly with
    the null stream, and not sharing the null stream's hardware queue either."""
    device = torch.device(device)
    if device not in _side_streams:
        for _ in range(16):
            st = _non_blocking_stream(device)
            if not _holds_up_the_default_stream(st):
                _side_streams[device] = st
                break
        else:
            raise AssertionError("no stream was found that leaves the default stream alone")
    return _side_streams[device]


def _delay(stream, ms=DELAY_MS):
    """Hold ``stream`` for about ``ms`` with one ``torch.cuda._sleep``, its tick rate measured once per device."""
    dev = stream.device
    if dev not in _ticks_per_ms:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(1000)                      # (the first launch loads the kernel)
            a.record()
            torch.cuda._sleep(2_000_000)
            b.record()
        b.synchronize()
        _ticks_per_ms[dev] = 2_000_000 / max(a.elapsed_time(b), 1e-3)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * _ticks_per_ms[dev]))


class Late(Plain):
    """``Plain`` for a run in a side stream: every operand is allocated and NaN-filled on the default stream, which is then waited
    for; on ``stream`` one delay is enqueued in front of the first operand, and the data of every "in" / "inout" operand is copied
    there (from pinned memory, without waiting).  A case run under ``torch.cuda.stream(stream)`` thus sees its inputs in ``stream``'s
    order only: work an entry put on another stream reads NaN, or is overwritten.  ``started`` is the event behind the delay."""

    def __init__(self, device, stream):
        super().__init__(device)
        self.stream = stream
        self.started = None
        self.roles = []
        self._pinned = []

    def place(self, t_or_shape, role, dtype=torch.float32, skew=0, name=None):
        assert role in ROLES, role
        name = name or f"{role}{self.placed}"
        self.placed += 1
        data = None
        if role in ("in", "inout"):
            data = t_or_shape.detach().contiguous()      # host data, or what an earlier call of the case left on the device
            dtype = data.dtype
        default = torch.cuda.default_stream(self.device)
        with torch.cuda.stream(default):
            v = torch.empty(_shape_of(t_or_shape), dtype=dtype, device=self.device)
            v.fill_(_fill_value(dtype))
        default.synchronize()
        v.record_stream(self.stream)
        if self.started is None:
            _delay(self.stream)
            self.started = torch.cuda.Event()
            self.started.record(self.stream)
        if data is not None:
            if data.device.type == "cpu":
                data = data.pin_memory()
                self._pinned.append(data)
            with torch.cuda.stream(self.stream):
                v.copy_(data, non_blocking=True)
        self.roles.append((name, role, v))
        if role in ("out", "inout"):
            self.outs.append((name, v))
        return v

    __call__ = place


class watching:
    """While active, every entry of ``OPERATOR_FAMILIES`` that takes a pointer notes, immediately before the library is called,
    its name and whether ``placer.started`` (the event behind a ``Late`` placer's delay) was still pending.  The note is taken on
    the bound entry itself: every route to the library passes it -- ``_op.call`` and the BatchNorm calls behind ``_handle.ptr``, and
    the cases that bind an entry themselves."""

    def __init__(self, placer):
        self.placer = placer
        self.calls = []

    def __enter__(self):
        import ctypes as C
        from eamm_amd import _lib
        self.lib = _lib.lib()
        self.saved = {}
        for name, (_, args) in _lib.SIGNATURES.items():
            if name.startswith(OPERATOR_FAMILIES) and any(a is C.c_void_p for a in args):
                fn = getattr(self.lib, name)
                self.saved[name] = fn
                setattr(self.lib, name, self._noting(name, fn))
        return self

    def _noting(self, name, fn):
        def entry(*args):
            started = self.placer.started
            self.calls.append((name, None if started is None else not started.query()))
            return fn(*args)
        return entry

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False


def run_late(cid, device="cuda:0"):
    """The case once on plain tensors and the default stream, once under ``torch.cuda.stream(side)`` with a ``Late`` placer: the same
    bits in every output (``unstable`` ones excepted), no NaN in an output that may not keep one, and -- or the run proves nothing --
    the delay still pending at the case's first library call that can read a placed operand."""
    fn, nan_ok, unstable = CASES[cid]
    plain = Plain(device)
    fn(plain)
    torch.cuda.synchronize()
    side = side_stream(device)
    late = Late(device, side)
    with watching(late) as seen, torch.cuda.stream(side):
        fn(late)
    torch.cuda.synchronize()
    if cid not in UNOBSERVED:
        # A call in front of the first placement takes no placed operand: the case is still making an input there, with the public
        # operator on tensors of its own (the motion cases' records, the augmentation cases' aligned video), as it does in an arena
        # run.  The case's first call in the sense of this check is the first one that can read a placed operand.
        placed = [(name, pending) for name, pending in seen.calls if pending is not None]
        assert placed, (cid, "the case reached no operator entry after its first placement: nothing was observed")
        assert placed[0][1], (cid, f"the delay was over at the first library call, {placed[0][0]}: the run proves nothing")
    nan = [n for n, role, v in late.roles if role == "out" and n not in nan_ok and v.dtype.is_floating_point and bool(torch.isnan(v).any())]
    assert not nan, (cid, "outputs hold NaN (unwritten, or computed before the inputs arrived)", nan)
    differ = [n for n in same_outputs(plain, late) if n not in unstable]
    assert not differ, (cid, "outputs of the side-stream run differ from the plain call", differ)


def run_three(cid, device="cuda:0"):
    fn, nan_ok, unstable = CASES[cid]
    sync = torch.cuda.synchronize if torch.device(device).type == "cuda" else lambda: None
    plain = Plain(device)
    fn(plain)
    sync()
    for skew in SKEWS:
        arena = Arena(device, skew=skew)
        fn(arena)
        sync()
        arena.check(nan_ok=nan_ok)
        differ = [n for n in same_outputs(plain, arena) if n not in unstable]
        if differ:      # tell an alignment / neighbourhood dependence from an entry that does not repeat itself
            again = Plain(device)
            fn(again)
            sync()
            assert not differ, (cid, f"skew {skew}: outputs differ from the plain call", differ,
                                "two plain calls differ in", same_outputs(plain, again))
