"""Does a *_dev entry point keep the stream contract of include/silent_hip.h:19-28?  (test infrastructure, like tests/write_coverage.py)

  "the *_dev twins ... are stream-ordered and do not synchronise", "the library never keeps a caller pointer past return", and when a
  workspace-using call arrives on another stream than the previous one "that previous stream is drained first".

Every other GPU test runs on the legacy default stream with the device synchronised around each call: there a launch that went to
stream 0 instead of the caller's stream, a table read after return or a missing drain computes the same bits.  Here the calls of
tests/write_coverage_cases.py run on a stream S that is HELD: silent_busy_wait_dev occupies S for D microseconds, an event `held`
is recorded behind it, and everything the scenario enqueues -- the producer of the inputs, the calls, the overwriter -- queues up
behind the hold while the host runs ahead.  Whatever leaves that order shows as wrong bits:

  * a launch on another stream runs DURING the hold and reads the decoy values the input buffers hold until the producer ran;
  * a read deferred past the call sees the next input or the zeros the overwriter leaves;
  * a host argument read after return sees what the harness wrote there as soon as the call returned.

The reference of every comparison is the quiet call: the same closure on the same values on the legacy default stream, device
synchronised before and after (what the rest of the suite ties to the oracle).  Outputs are deterministic, so bits must agree.

`pending` keeps the scenarios from passing vacuously: right after a call returns, `held` must not have completed -- the call did
not wait for the stream, and the host really was ahead of the device.  It is a stream query, not a clock comparison.  D is measured
per sequence: after a warm-up (workspace growth, module loading, allocator) the host time to enqueue the sequence without a hold is
taken with perf_counter; D = MARGIN x that, at least MIN_HOLD_US (what pick_concurrent_stream spins), at most the entry point's
1 000 000.  A call that is not pending gets ONE repeat with 4 x D; then it is reported as "synchronised".

Watch swaps the ctypes handle of pysilent_amd._lib for a proxy for the length of a scenario: behind every silent_*_dev call it
notes the stream argument (it must be torch's current stream: the wrapper's part of the contract), whether a pointer argument lies
inside the scenario's input buffers (a wrapper that hands the library a converted COPY would hide a late read), and -- scenario 4 --
overwrites every argument the header places in host memory (clobber_host_args).
"""
import contextlib
import ctypes as C
import gc
import time

import numpy as np

import write_coverage as wc
import write_coverage_cases as wcc

MIN_HOLD_US = 400          # pysilent_amd.pipeline.pick_concurrent_stream's spin
MAX_HOLD_US = 1000000      # silent_busy_wait_dev refuses more
MARGIN = 4                 # D = MARGIN x the measured enqueue time: room for host jitter

# Calls of scenario 1 that may return with the hold already over: (case id, call index) -> "file:line: what synchronises there".  Only
# the two drains of include/silent_hip.h (workspace handed to another stream; a workspace that grows -- the warm-up avoids both) and a
# host read-back inside a Python wrapper may stand here.  Empty: no *_dev call of the catalogue synchronises.
SYNCHRONISES = {}

HOLDS = []                 # (what, D in microseconds) of every held sequence of this process


# ----------------------------------------------------------------------------- inputs: a, b, decoy, zeros

def _like(x, data):
    if isinstance(x, wcc.Packed):
        p = wcc.Packed.__new__(wcc.Packed)
        p.levels, p.extents, p.channels, p.n_frames, p.data = None, x.extents, x.channels, x.n_frames, data
        return p
    return data


def shuffled(x, seed):
    """A second input of the geometry, dtype, sign and sparsity of ``x``: its values in another order (seeded) and HALVED (exact
    for the float32 inputs, a shift for the integer ones).  Another order alone would leave the per-level extrema of a noise input
    what they were -- 0 and 255 -- and a workspace that still holds, or has already merged, the other call's extrema would give the
    right threshold."""
    data = wcc.raw(x)
    new = np.random.default_rng(seed).permutation(data.reshape(-1)).reshape(data.shape)
    new = new // 2 if data.dtype.kind == "u" else new * np.float32(0.5)
    return _like(x, np.ascontiguousarray(new.astype(data.dtype)))


def decoy(x):
    """What the input buffers hold before the producer ran: write_coverage_cases.other_values(x, 2) in the dtype of ``x``."""
    return _like(x, wcc.raw(wcc.other_values(x, 2)).astype(wcc.raw(x).dtype))


def zeros(x):
    return _like(x, np.zeros_like(wcc.raw(x)))


class Subject(object):
    """What a scenario runs: ``calls(rt, *inputs) -> [closure]`` of a case of the catalogue and its inputs ``a``; ``b``, the decoy and
    the zeros are derived once."""

    def __init__(self, id, calls, a, workspace=False):
        self.id, self.calls, self.workspace = id, calls, workspace
        self.a = tuple(a)
        self.b = tuple(shuffled(x, 4200 + i) for i, x in enumerate(self.a))
        self.decoy = tuple(decoy(x) for x in self.a)
        self.zeros = tuple(zeros(x) for x in self.a)
        self.quiet, self.on_device = {}, {}


_SUBJECTS = {}      # the subject of the case at hand (one: the quiet results of a case are megabytes)


def _regulate_direct(case):
    """regulate-*: the catalogue's closure is rt.regulate(abs(x), ...) -- abs() is a torch launch that hands the library a COPY of the
    buffer.  The same calls on inputs that are non-negative already, the buffer itself as the argument."""
    ks = tuple(int(v) for v in case.id.split("-")[1].split("x"))
    k = np.abs(np.random.default_rng(12).standard_normal(ks)) * 1e-3
    calls = wcc.each(lambda rt, x: [lambda p=p: (rt.regulate(x, k, 1.0, 0.1, flat_policy=p),) for p in ("ieee", "zero")])
    return calls, [np.abs(x) for x in case.inputs()]


def _overflow_gray_direct(case):
    """overflow-gray_keypoints: the catalogue's closure passes ``f32 * 0`` (a copy); here the black frames are the input."""
    def calls(rt, f32, u8, u8x3):
        from pysilent_amd.util.zoom.from_image import classic_levels
        plan = wcc.plan_of(rt, ("tiny", (16, 56)), (16, 56), 1, classic_levels((16, 56), 2.0, 2))
        return [lambda: wcc.gray_keypoints(rt, plan, f32, 4, selection=False, cap=wcc.CAP, overflow=True)]
    a = list(case.inputs())
    return calls, [a[0] * 0] + a[1:]


# cases whose catalogue closure copies its input before the library sees it: the same library calls on the buffer itself
# (test_the_direct_routes_make_the_catalogues_calls ties them to the catalogue's results)
DIRECT = {"overflow-gray_keypoints": _overflow_gray_direct}
DIRECT.update({c.id: _regulate_direct for c in wcc.CASES if c.id.startswith("regulate-")})


def subject(case):
    if case.id not in _SUBJECTS:
        _SUBJECTS.clear()
        calls, a = DIRECT[case.id](case) if case.id in DIRECT else (case.calls, case.inputs())
        _SUBJECTS[case.id] = Subject(case.id, calls, a, case.workspace)
    return _SUBJECTS[case.id]


# ----------------------------------------------------------------------------- host-memory arguments (scenario 4)

def _weights_table():
    """entry point (without silent_ / _dev) -> [(index of the float* among the arguments behind ctx, floats(args))]: the weights the
    header places in host memory; g(j) is the integer argument j.  (Extent tables, parameter blocks and frame views are found by their argument types.)"""
    t = {"conv2d_same": [(5, lambda g: g(6) * g(7) * g(4) * g(8))],
         "regulate": [(5, lambda g: g(6) * g(7) * g(4) * g(4))],
         "gray_line_end": [(4, lambda g: 9), (5, lambda g: 9 * g(6))]}
    gray = [(3, lambda g: 9), (4, lambda g: 9 * g(5))]
    for sfx in ("", "_u8", "_u8x3", "_view", "_u16", "_view16"):
        t["gray_keypoints" + sfx] = gray
        if sfx:
            t["gray_pass" + sfx] = gray
    for name in ("gray_pass", "gray_pass_parts", "gray_pass_h"):
        t[name] = gray
    return t


WEIGHTS = _weights_table()
RGB_KERNEL_FLOATS = (("rgc", 81), ("rgby", 81), ("stripe", 81), ("blur", 441), ("end", 81))


def _short(name):
    return name[len("silent_"):-len("_dev")]


def _host_struct_types():
    from pysilent_amd import _lib
    return {C.POINTER(t): t for t in (_lib.RgbChainParams, _lib.BoostingParams, _lib.AffineParams, _lib.FrameView, _lib.FrameView16)}


def dev_entry_points_with_host_arguments():
    """Every silent_*_dev of the binding that takes an argument in host memory, by its signature: a silent_extent table, a parameter
    block, a frame view, or float weights (WEIGHTS)."""
    from pysilent_amd import _lib
    structs = _host_struct_types()
    out = []
    for name, argtypes in sorted(_lib._SIGNATURES.items()):
        if name.endswith("_dev") and (any(t is _lib._ep or t in structs for t in argtypes[1:-1]) or _short(name) in WEIGHTS):
            out.append(name)
    return out


def _int(v):
    return int(getattr(v, "value", v) or 0)


def _pointee(arg):
    """The structure behind a byref() / pointer() argument."""
    return arg._obj if hasattr(arg, "_obj") else arg.contents


def clobber_host_args(name, argtypes, args):
    """Overwrites what the header places in host memory for this *_dev call, in place: weights become -3 * w, silent_extent tables
    1 x 1, parameter blocks and frame views all-zero bytes (the kernels a silent_rgb_chain_params points to: -3 * w first).  Returns
    what it overwrote."""
    from pysilent_amd import _lib
    structs = _host_struct_types()
    a, types, done = args[1:-1], argtypes[1:-1], []
    for i, (t, v) in enumerate(zip(types, a)):
        if v is None:
            continue
        if t is _lib._ep:
            for e in v:
                e.h = e.w = 1
            done.append("extent table %d" % i)
        elif t in structs:
            s = _pointee(v)
            if isinstance(s, _lib.RgbChainParams):
                for field, n in RGB_KERNEL_FLOATS:
                    np.ctypeslib.as_array(getattr(s, field), shape=(n,))[...] *= np.float32(-3.0)
            C.memset(C.addressof(s), 0, C.sizeof(s))
            done.append(type(s).__name__)
    for i, floats in WEIGHTS.get(_short(name), ()):
        n = int(floats(lambda j: _int(a[j])))
        w = np.ctypeslib.as_array((C.c_float * n).from_address(_int(a[i])))
        w *= np.float32(-3.0)
        done.append("weights %d (%d floats)" % (i, n))
    return done


def _pointers(argtypes, args):
    from pysilent_amd import _lib
    out = []
    for t, v in zip(argtypes[1:-1], args[1:-1]):
        if v is None:
            continue
        if t is C.c_void_p:
            out.append(_int(v))
        elif t in (_lib._bp, _lib._sp):
            out.append(_int(C.cast(v, C.c_void_p)))
        elif t in (_lib._wp, _lib._xp):
            out.append(_int(v.contents.data))
    return out


class Watch(object):
    """The proxy behind pysilent_amd._lib.load() while a scenario runs: records every silent_*_dev call (but the hold's own)."""

    def __init__(self, harness):
        self.h, self.records, self.clobber, self.inputs = harness, [], False, []

    def __getattr__(self, name):
        fn = getattr(self.h.lib, name)
        if not name.endswith("_dev") or name in ("silent_busy_wait_dev", "silent_trace_marker_dev"):
            return fn

        def call(*args):
            rc = fn(*args)
            pending = self.h.pending()
            current = self.h.torch.cuda.current_stream(self.h.dev).cuda_stream
            assert _int(args[-1]) == current, "%s was given stream %#x, torch's current stream is %#x" % (name, _int(args[-1]), current)
            rec = {"name": name, "pending": pending,
                   "reads_input": any(lo <= p < hi for p in _pointers(fn.argtypes, args) for lo, hi in self.inputs)}
            if self.clobber and rc == 0:
                rec["clobbered"] = clobber_host_args(name, fn.argtypes, args)
            self.records.append(rec)
            return rc
        return call


# ----------------------------------------------------------------------------- the harness

class Buffers(object):
    """The device input buffers of a subject, holding ``values``, and its closures, built ONCE on them: a scenario changes the
    buffers in place (load), never the closures."""

    def __init__(self, rt, subj, values):
        self.tensors = [wcc.on_device(rt, v) for v in values]
        self.raw = [t.data if isinstance(t, rt.PackedPyramid) else t for t in self.tensors]
        self.calls = subj.calls(rt, *self.tensors)

    def load(self, staged):
        """Enqueues, on torch's current stream, the copies that make the buffers hold ``staged``."""
        for r, s in zip(self.raw, staged):
            r.copy_(s, non_blocking=True)

    def ranges(self):
        return [(r.data_ptr(), r.data_ptr() + r.numel() * r.element_size()) for r in self.raw]


class Harness(object):
    def __init__(self, rt):
        import torch
        from pysilent_amd import _lib
        from pysilent_amd.pipeline import pick_concurrent_stream
        self.rt, self.torch, self._lib_module = rt, torch, _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda", 0)
        self.ctx = rt.get_context(0)
        self.S, self.verified = pick_concurrent_stream(torch, self.dev, [torch.cuda.default_stream(self.dev)])
        self.S2, self.verified2 = pick_concurrent_stream(torch, self.dev, [self.S])
        self.held = None
        self.watch = None
        print("stream-order streams: S verified=%s, S2 verified=%s" % (self.verified, self.verified2))

    # -- the hold
    def hold(self, microseconds, stream=None):
        """Occupies ``stream`` (S) for ``microseconds`` and records `held` behind it."""
        stream = stream or self.S
        self.ctx.check(self.lib.silent_busy_wait_dev(self.ctx.handle, int(microseconds), C.c_void_p(stream.cuda_stream)))
        self.held = self.torch.cuda.Event()
        self.held.record(stream)

    def pending(self):
        """True while the hold has not run out; None without a hold."""
        return None if self.held is None else not self.held.query()

    def sync(self):
        self.torch.cuda.synchronize(self.dev)
        self.held = None

    @contextlib.contextmanager
    def watching(self, inputs=(), clobber=False):
        """pysilent_amd._lib.load() hands out the recording proxy inside the block.  wcc._overflowed -- a host read-back of the
        counts inside the catalogue's own helper, behind the library call -- is deferred to the end of the block."""
        w = Watch(self)
        w.inputs, w.clobber = list(inputs), clobber
        deferred = []
        real_lib, real_overflowed = self._lib_module._lib, wcc._overflowed
        self._lib_module._lib, wcc._overflowed, self.watch = w, (lambda counts, cap: deferred.append((counts, cap))), w
        try:
            yield w
        finally:
            self._lib_module._lib, wcc._overflowed, self.watch = real_lib, real_overflowed, None
        self.sync()
        for counts, cap in deferred:
            real_overflowed(counts, cap)

    def staged(self, subj, which):
        """Input ``which`` ("a", "b", "decoy", "zeros") of the subject on the device, shaped like Buffers.raw: the sources of the
        producer's and the overwriter's copies.  Made once."""
        if which not in subj.on_device:
            subj.on_device[which] = [self.torch.from_numpy(np.array(wcc.raw(v))).to(self.dev) for v in getattr(subj, which)]
            self.sync()
        return subj.on_device[which]

    # -- a held sequence
    def run_held(self, what, seq, reset, asserted, exempt=None):
        """``seq(D)`` enqueues the scenario (D > 0: with the hold in front) and returns (results, [pending of each call]); ``reset()``
        restores the buffers before each run.  Warm-up, measurement of D, the run; ONE repeat with 4 x D when an ``asserted`` call was
        not pending.  Returns (results, records of the proxy, D)."""
        def once(d):
            self.sync()
            reset()
            self.sync()
            gc_was_on = gc.isenabled()
            gc.disable()                   # (a collection between the hold and a call is host time the measurement did not see)
            try:
                with self.watching(self._inputs) as w:
                    t0 = time.perf_counter()
                    out, pend = seq(d)
                    dt = time.perf_counter() - t0
            finally:
                if gc_was_on:
                    gc.enable()
            return out, pend, w.records, dt
        once(0)
        d = int(min(max(MIN_HOLD_US, MARGIN * once(0)[3] * 1e6), MAX_HOLD_US))
        for attempt in (0, 1):
            out, pend, records, _ = once(d)
            late = [i for i in asserted if not pend[i]]
            HOLDS.append((what, d))
            print("stream-order hold: %s D=%d us%s" % (what, d, " (not pending: %s)" % late if late else ""))
            if not late or exempt:
                break
            d = min(4 * d, MAX_HOLD_US)
        assert not late or exempt, ("%s: synchronised: call %s of the sequence returned only after the hold had run out, with D and with "
                                    "4 x D = %d us (include/silent_hip.h:28: the *_dev twins do not synchronise)" % (what, late, d))
        return out, records, d

    _inputs = ()


def quiet(h, subj, which):
    """The reference: every call of the subject on input ``which`` ("a" / "b"), on the legacy default stream, the device synchronised
    before and after.  [[(name, ndarray)]] per call; computed once."""
    if which not in subj.quiet:
        bufs = Buffers(h.rt, subj, getattr(subj, which))
        out = []
        for call in bufs.calls:
            h.sync()
            res = call()
            h.sync()
            out.append(wc.specified(res))
        assert out and all(out), subj.id
        subj.quiet[which] = out
    return subj.quiet[which]


def _check_records(what, records, n_calls):
    assert len(records) >= n_calls, "%s: %d library calls seen for %d calls of the sequence" % (what, len(records), n_calls)
    bad = [r["name"] for r in records if not r["reads_input"]]
    assert not bad, ("%s: %s was not given the input buffer itself (a converted copy hides a late read): add a direct route to "
                     "stream_order.DIRECT" % (what, bad))


def scenario_producer_call_overwriter(h, subj, i, bufs=None, library=True):
    """Scenario 1 for call ``i`` of the subject: decoy in the buffers; on S: hold, copy a, call, copy b, call, copy zeros.
    library=False: the closures are stand-ins that make no library call (the harness's own test)."""
    qa, qb = quiet(h, subj, "a"), quiet(h, subj, "b")
    bufs = bufs or Buffers(h.rt, subj, subj.decoy)
    a, b, z, dec = (h.staged(subj, w) for w in ("a", "b", "zeros", "decoy"))
    call = bufs.calls[i]

    def seq(d):
        with h.torch.cuda.stream(h.S):
            if d:
                h.hold(d)
            bufs.load(a)
            ra, pa = call(), h.pending()
            bufs.load(b)
            rb, pb = call(), h.pending()
            bufs.load(z)
        return (ra, rb), [pa, pb]

    what = "%s call %d" % (subj.id, i)
    h._inputs = bufs.ranges()
    try:
        (ra, rb), records, d = h.run_held(what, seq, lambda: bufs.load(dec), asserted=(0, 1), exempt=SYNCHRONISES.get((subj.id, i)))
    finally:
        h._inputs = ()
    if library:
        _check_records(what, records, 2)
    wc.assert_same_bits(wc.specified(ra), qa[i], what + ": first call behind the producer, against the quiet call on a")
    wc.assert_same_bits(wc.specified(rb), qb[i], what + ": second call right behind it, against the quiet call on b")
    return d


def scenario_two_streams(h, subj, i, pair, hold_both=False):
    """Scenario 2: hold + call on a on S, the call on b at once on S2 (the workspace changes hands: the documented drain may block
    the second call, so only the first must be pending).  hold_both: S2 is held for as long as S in front of its call.  Without
    that, a call on S2 that was NOT ordered behind S would run to its end while S is still held and the two calls would never meet
    in the workspace; with both streams released together they do."""
    qa, qb = quiet(h, subj, "a"), quiet(h, subj, "b")
    xa, xb = pair
    a, b = h.staged(subj, "a"), h.staged(subj, "b")

    def reset():
        xa.load(a)
        xb.load(b)

    def seq(d):
        with h.torch.cuda.stream(h.S):
            if d:
                h.hold(d)
            ra, pa = xa.calls[i](), h.pending()
        with h.torch.cuda.stream(h.S2):
            if d and hold_both:
                h.ctx.check(h.lib.silent_busy_wait_dev(h.ctx.handle, int(d), C.c_void_p(h.S2.cuda_stream)))
            rb = xb.calls[i]()
        return (ra, rb), [pa]

    what = "%s call %d, two streams%s" % (subj.id, i, ", both held" if hold_both else "")
    (ra, rb), _, d = h.run_held(what, seq, reset, asserted=(0,))
    wc.assert_same_bits(wc.specified(ra), qa[i], what + ": the held call on S, against the quiet call on a")
    wc.assert_same_bits(wc.specified(rb), qb[i], what + ": the call on S2, against the quiet call on b")
    return d


def scenario_host_form_behind_device_form(h, subj, i, bufs, host_calls):
    """Scenario 3: hold + the *_dev call on a on S, then the host-pointer form on b (legacy default stream, same workspace)."""
    qa, qb = quiet(h, subj, "a"), quiet(h, subj, "b")
    a = h.staged(subj, "a")

    def seq(d):
        with h.torch.cuda.stream(h.S):
            if d:
                h.hold(d)
            ra, pa = bufs.calls[i](), h.pending()
        rb = host_calls[i]()
        return (ra, rb), [pa]

    what = "%s call %d, host form behind the device form" % (subj.id, i)
    (ra, rb), _, d = h.run_held(what, seq, lambda: bufs.load(a), asserted=(0,))
    wc.assert_same_bits(wc.specified(ra), qa[i], what + ": the held device form, against the quiet call on a")
    wc.assert_same_bits(wc.specified(rb), qb[i], what + ": the host form, against the quiet device form on b")
    return d


def scenario_host_arguments(h, subj, i, bufs, host_arrays=()):
    """Scenario 4: hold + the call on a on S; as soon as the library returns -- the hold still pending -- every host-memory
    argument is overwritten (by the proxy, at the ctypes call; ``host_arrays``: arrays of a stand-in op, multiplied by -3 here)."""
    qa = quiet(h, subj, "a")            # (before anything is overwritten)
    a = h.staged(subj, "a")
    keep = [np.array(x) for x in host_arrays]

    def reset():
        bufs.load(a)
        for x, k in zip(host_arrays, keep):
            x[...] = k

    def seq(d):
        with h.torch.cuda.stream(h.S):
            if d:
                h.hold(d)
            if h.watch is not None:
                h.watch.clobber = True
            ra, pa = bufs.calls[i](), h.pending()
            for x in host_arrays:
                x *= -3
        return ra, [pa]

    what = "%s call %d, host arguments overwritten at return" % (subj.id, i)
    try:
        ra, records, d = h.run_held(what, seq, reset, asserted=(0,))
    finally:
        for x, k in zip(host_arrays, keep):
            x[...] = k
    wc.assert_same_bits(wc.specified(ra), qa[i], what + ", against the quiet call with the original arguments")
    return records
