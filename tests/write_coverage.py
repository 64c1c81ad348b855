"""Did an entry point write EVERY element of its outputs, and ONLY those?  (test infrastructure, like tests/plan_geometry.py)

The way results are allocated hides wrong answers to both questions.  The host-pointer entry points stage their outputs in one
persistent device arena whose offsets depend on the argument sizes alone, and the wrappers of pysilent_amd/_runtime.py allocate
device results with torch.empty, which hands a freed block of the same size straight back: an element a kernel skips still holds
what the previous call of the same geometry put there -- usually the correct value.  And an allocation is rounded up, so a store a
few elements past the end of a map, or before its start, lands in padding nobody looks at.

The harness therefore hands out result buffers that are the MIDDLE of a larger allocation, every byte of it -- guards and payload
-- set to a fill byte:

  * a skipped element keeps the fill.  One fill is not enough (a hole in a 0 / 1 mask filled with 0x00 reads as a legitimate 0),
    so every case runs under TWO fills, 0xA5 and 0x5A -- as float32 about -2.9e-16 and +1.5e16, as float16 -0.0221 and 203.25, as
    int64 two unrelated huge numbers -- and the two results must agree bit for bit: a kernel that is deterministic and writes all
    of its output cannot tell the fills apart; one that skips an element, or accumulates into it, returns the fill (or a function
    of it) in one run and another value in the other;
  * a store outside the payload changes a guard byte: ``check()`` reports buffer, side and the damaged byte range.

A hole is an UNWRITTEN element, not a zero: an op that writes zeros where another would write values passes here (what the values
must be is the business of the parity tests).

tests/test_write_coverage.py shows on the CPU, with fake ops, that each of these mistakes is reported with the right buffer and
offset; tests/test_gpu_write_coverage.py runs the entry points of include/silent_hip.h through it.
"""
import contextlib
import ctypes as C

import numpy as np

GUARD = 256                     # bytes of guard on each side of a payload, at least
FILLS = (0xA5, 0x5A)
ARENA_POISON_BYTES = 64 << 20   # what poison_arena() covers of the host-form staging arena
ARENA_ALIGN = 256               # csrc/silent_internal.h align_up: every staged argument starts on a multiple of it


# ----------------------------------------------------------------------------- bit patterns

def to_numpy(a):
    """An ndarray with the bytes of ``a`` (ndarray, torch tensor or PackedPyramid)."""
    a = getattr(a, "data", a) if type(a).__name__ == "PackedPyramid" else a
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a)


_BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16, np.dtype(np.int64): np.uint64,
         np.dtype(np.uint8): np.uint8}


def bits(a):
    """The raw bit patterns of a float32 / float16 / int64 array (uint8: the bytes themselves) as unsigned integers of the same
    width.  No NaN folding: the kernels are deterministic, so two runs of one op agree on NaN signs and payloads too."""
    a = to_numpy(a)
    if a.dtype not in _BITS:
        raise TypeError("bits(): float32, float16, int64 or uint8 expected, got %s" % a.dtype)
    return a.view(_BITS[a.dtype])


def assert_same_bits(got, want, what):
    """Two lists of (name, array): same names, shapes, dtypes and bit patterns.  The message names the buffer, the number of
    differing elements and the first and last of them as element index and byte offset."""
    assert [n for n, _ in got] == [n for n, _ in want], "%s: results differ in number or name: %s vs %s" % (
        what, [n for n, _ in got], [n for n, _ in want])
    for (name, a), (_, b) in zip(got, want):
        a, b = to_numpy(a), to_numpy(b)
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: buffer %s: %s %s vs %s %s" % (what, name, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.flatnonzero(bits(a).reshape(-1) != bits(b).reshape(-1))
        if bad.size:
            first, last, sz = int(bad[0]), int(bad[-1]), a.dtype.itemsize
            raise AssertionError("%s: buffer %s: %d of %d elements differ, first element %d (byte offset %d: %r vs %r), last element %d "
                                 "(byte offset %d)" % (what, name, bad.size, a.size, first, first * sz, a.reshape(-1)[first],
                                                       b.reshape(-1)[first], last, last * sz))


# ----------------------------------------------------------------------------- guarded buffers

class GuardedBuffers(object):
    """Result buffers with guards.  ``backend``: "torch" (a uint8 CUDA tensor viewed as the requested dtype) or "numpy" (the CPU
    self-test).  ``lead_bytes``: the payload starts GUARD + lead_bytes bytes into its 256-byte aligned allocation -- an int below
    256, or a callable (np.dtype, ordinal of the buffer among those of its dtype) -> int for a placement per argument."""

    def __init__(self, backend, fill_byte, lead_bytes=0, device="cuda:0"):
        if backend not in ("torch", "numpy"):
            raise ValueError("backend must be 'torch' or 'numpy'")
        self.backend, self.fill, self.lead, self.device = backend, int(fill_byte) & 0xff, lead_bytes, device
        self.records = []

    def _lead_of(self, dtype):
        lead = self.lead
        if callable(lead):
            lead = lead(dtype, sum(1 for r in self.records if r["dtype"] == dtype))
        lead = int(lead)
        if not 0 <= lead < 256 or lead % dtype.itemsize:
            raise ValueError("lead_bytes %d: must be in [0, 256) and a multiple of the element size %d" % (lead, dtype.itemsize))
        return lead

    def empty(self, shape, dtype=np.float32, device=None):
        """A buffer of ``shape`` / ``dtype`` whose every byte is the fill, between two guards."""
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if np.ndim(shape) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        start = GUARD + self._lead_of(dtype)
        total = -(-(start + nbytes + GUARD) // 256) * 256
        if self.backend == "numpy":
            raw = np.full(total + 256, self.fill, np.uint8)
            skew = -raw.ctypes.data % 256
            whole = raw[skew:skew + total]
            payload = whole[start:start + nbytes].view(dtype).reshape(shape)
        else:
            import torch
            tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16, np.dtype(np.int64): torch.int64,
                   np.dtype(np.uint8): torch.uint8}[dtype]
            whole = torch.full((total,), self.fill, dtype=torch.uint8, device=device or self.device)
            assert whole.data_ptr() % 256 == 0, "allocator returned a block that is not 256-byte aligned"
            payload = whole[start:start + nbytes].view(tdt).reshape(shape)
        self.records.append({"name": "#%d %s%s" % (len(self.records), dtype.name, list(shape)), "whole": whole, "start": start,
                             "nbytes": nbytes, "dtype": dtype, "payload": payload})
        return payload

    def name_of(self, payload):
        for r in self.records:
            if r["payload"] is payload:
                return r["name"]
        return None

    def owns(self, tensor):
        """True when the tensor's bytes lie inside the payload of a buffer handed out here (torch backend)."""
        lo, n = tensor.data_ptr(), tensor.numel() * tensor.element_size()
        for r in self.records:
            start = r["whole"].data_ptr() + r["start"]
            if start <= lo and lo + n <= start + r["nbytes"]:
                return True
        return False

    def damage(self):
        """[(buffer name, side, first, last, count)]: damaged guard bytes, offsets relative to the payload's first byte (the front
        guard's are negative, the back guard's start at the payload's size)."""
        out = []
        for r in self.records:
            whole = to_numpy(r["whole"])
            start, end = r["start"], r["start"] + r["nbytes"]
            for side, lo, hi in (("front", 0, start), ("back", end, whole.size)):
                bad = np.flatnonzero(whole[lo:hi] != self.fill)
                if bad.size:
                    out.append((r["name"], side, int(bad[0]) + lo - start, int(bad[-1]) + lo - start, int(bad.size)))
        return out

    def check(self, what=""):
        """Every guard byte of every buffer handed out still equals the fill."""
        dmg = self.damage()
        assert not dmg, "%s: written outside an output: %s" % (what, "; ".join(
            "buffer %s (payload %d bytes): %s guard, %d bytes damaged, byte offsets %+d .. %+d from the payload's start"
            % (n, next(r["nbytes"] for r in self.records if r["name"] == n), side, cnt, first, last)
            for n, side, first, last, cnt in dmg))


def weakest_alignment(dtype, ordinal):
    """The weakest placement include/silent_hip.h allows a result: the element size where the header states nothing (float32 maps:
    4 bytes, int64 index rows and counts: 8); for the float16 maps of silent_gray_pass_h "end_out must be 16-byte and cs_out 2-byte
    aligned" (silent_hip.h:198) -- the wrappers allocate cs before end, so the float16 buffers alternate cs, end."""
    dtype = np.dtype(dtype)
    if dtype == np.float16:
        return 16 if ordinal % 2 else 2
    return dtype.itemsize


CURRENT = []        # the GuardedBuffers of the enclosing guarded() blocks


@contextlib.contextmanager
def guarded(rt, monkeypatch, fill_byte, lead_bytes=0):
    """Inside the block every result a wrapper of ``rt`` (pysilent_amd._runtime) allocates for a DEVICE operand -- op.empty and
    op.alloc, i.e. _Operand.empty -- comes from one GuardedBuffers, which the block yields.  Host operands keep np.empty."""
    gb = GuardedBuffers("torch", fill_byte, lead_bytes)
    plain = rt._Operand.empty

    def empty(self, shape, dtype=np.float32):
        if not self.dev:
            return plain(self, shape, dtype)
        out = gb.empty(shape, dtype, device=self._torch_device)
        return out, C.c_void_p(out.data_ptr())

    with monkeypatch.context() as m:
        m.setattr(rt._Operand, "empty", empty)
        CURRENT.append(gb)
        try:
            yield gb
        finally:
            CURRENT.pop()


def result_like(x, shape, dtype=np.float32):
    """A result buffer for an entry point that is called without a wrapper's allocation (silent_cast_interleave_dev, the in-place
    boosting state): placed like ``x``; guarded inside a guarded() block when ``x`` is a device tensor."""
    if hasattr(x, "data_ptr"):
        if CURRENT:
            return CURRENT[-1].empty(shape, dtype, device=x.device)
        import torch
        return torch.empty(shape, dtype={np.float32: torch.float32, np.int64: torch.int64, np.float16: torch.float16}[dtype], device=x.device)
    return np.empty(shape, dtype)


# ----------------------------------------------------------------------------- the host forms' staging arena

def staged_bytes(arrays_nbytes):
    """What HostStage (csrc/silent_core.hip) takes of the arena for arguments of these sizes: each rounded up to ARENA_ALIGN."""
    return sum(-(-max(int(b), 1) // ARENA_ALIGN) * ARENA_ALIGN for b in arrays_nbytes)


def poison_arena(rt, value, nbytes=ARENA_POISON_BYTES):
    """Leaves bytes [0, nbytes) of the context's host-form staging arena holding float32 ``value``: ONE host-form call, the identity
    silent_affine_clip on nbytes / 8 floats -- its input is staged at arena offset 0, its output directly after."""
    x = np.full((1, 1, nbytes // 8, 1), value, np.float32)
    assert staged_bytes([x.nbytes, x.nbytes]) == nbytes
    out = rt.affine_clip(x)
    assert out.shape == x.shape and bits(out)[0, 0, 0, 0] == bits(x)[0, 0, 0, 0] and (bits(out) == bits(x)[0, 0, 0, 0]).all()


# ----------------------------------------------------------------------------- specified parts

class Rows(object):
    """The keypoint rows of silent_max_value_indices_region and the calls that end in it: idx [n_frames, cap, 4] int64 and counts
    [n_frames].  include/silent_hip.h:344-346: "counts[f] = number of rows frame f produced.  If any count exceeds cap_per_frame only
    the first cap_per_frame rows of that frame are written" -- rows from min(counts[f], cap) on are unspecified and are not compared.
    (Their bytes still lie inside the payload: the guards behind the buffer are checked in full.)"""

    def __init__(self, idx, counts):
        self.idx, self.counts = idx, counts


def buffers_of(results):
    """Every array / tensor among a case's results (PackedPyramid: its data; Rows: idx and counts; None skipped)."""
    out = []
    for r in results:
        if r is None:
            continue
        for a in ((r.idx, r.counts) if isinstance(r, Rows) else (r,)):
            out.append(a.data if type(a).__name__ == "PackedPyramid" else a)
    return out


def specified(results, prefix=""):
    """A case's results -> [(name, ndarray)] of the parts the header specifies: arrays, tensors and PackedPyramids whole; Rows as
    counts and, per frame, the first min(counts[f], cap) rows; None (an output the call was not asked for) is skipped."""
    out = []
    for i, r in enumerate(results):
        name = "%sresult %d" % (prefix, i)
        if r is None:
            continue
        if isinstance(r, Rows):
            idx, counts = to_numpy(r.idx), to_numpy(r.counts)
            out.append((name + " counts", counts))
            keep = [idx[f, :max(0, min(int(counts[f]), idx.shape[1]))] for f in range(idx.shape[0])]
            out.append((name + " rows", np.concatenate(keep) if keep else idx[:0, 0]))
        else:
            out.append((name, to_numpy(r)))
    return out


def two_fill_check(run, what, fills=FILLS, lead_bytes=0):
    """``run(GuardedBuffers) -> results`` once per fill on the numpy backend: guards intact, the two results bit-identical.
    Returns the first run's specified results."""
    got = []
    for fill in fills:
        gb = GuardedBuffers("numpy", fill, lead_bytes)
        res = run(gb)
        named = []
        for i, r in enumerate(res):
            named.append((gb.name_of(r) or "result %d" % i, np.array(r)))
        gb.check("%s, fill 0x%02X" % (what, fill))
        got.append(named)
    assert_same_bits(got[1], got[0], "%s: fill 0x%02X against fill 0x%02X (an element that follows the fill was not written)"
                     % (what, fills[1], fills[0]))
    return got[0]
