"""The harness of tests/write_coverage.py on the CPU (numpy backend, fake ops): a correct op passes, and an op that skips an element,
writes outside its output or assumes a zeroed output is reported with the buffer and the byte offset.  Plus what the GPU table of
tests/write_coverage_cases.py promises without a GPU: every case fits the poisoned part of the staging arena, and the allocation
patch leaves host operands alone."""
import re

import numpy as np
import pytest

import write_coverage as wc
import write_coverage_cases as wcc

SHAPE = (2, 7, 13, 3)
N = int(np.prod(SHAPE))
X = (np.random.default_rng(5).integers(1, 256, SHAPE)).astype(np.float32)
NAME = re.escape("#0 float32[2, 7, 13, 3]")


def _flat_around(out, lo, hi):
    """The floats of the allocation around ``out`` from element ``lo`` to ``hi`` relative to out[0] (a fake kernel's stray pointer)."""
    base = out.base
    while base.base is not None:
        base = base.base
    start = (out.ctypes.data - base.ctypes.data)
    return base[start + 4 * lo:start + 4 * hi].view(np.float32)


def correct(gb):
    out = gb.empty(SHAPE)
    out[...] = X * 2
    return (out,)


def skips_last_column_of_last_row(gb):
    out = gb.empty(SHAPE)
    out[...] = X * 2
    out[-1, -1, -1, :] = np.frombuffer(bytes([gb.fill]) * 12, np.float32)      # never stored: the fill is still there
    return (out,)


def skips_one_interior_element(gb):
    out = gb.empty(SHAPE)
    keep = out[1, 3, 5, 1].copy()
    out[...] = X * 2
    out[1, 3, 5, 1] = keep
    return (out,)


def writes_one_past_the_end(gb):
    out = gb.empty(SHAPE)
    _flat_around(out, 0, N + 1)[:] = np.append((X * 2).reshape(-1), np.float32(3.0))
    return (out,)


def writes_one_before_the_start(gb):
    out = gb.empty(SHAPE)
    _flat_around(out, -1, N)[:] = np.append(np.float32(3.0), (X * 2).reshape(-1))
    return (out,)


def accumulates(gb):
    out = gb.empty(SHAPE)
    with np.errstate(all="ignore"):
        out += X * 2
    return (out,)


def writes_zeros_into_a_hole(gb):
    out = gb.empty(SHAPE)
    out[...] = X * 2
    out[1, 3, 5, :] = 0.0
    return (out,)


def test_a_correct_op_passes():
    (name, got), = wc.two_fill_check(correct, "correct")
    assert name == "#0 float32[2, 7, 13, 3]"
    np.testing.assert_array_equal(got, X * 2)


def test_zeros_written_into_a_hole_pass():
    """A hole is an unwritten element, not a zero."""
    (_, got), = wc.two_fill_check(writes_zeros_into_a_hole, "zeros")
    assert not got[1, 3, 5].any()


LAST = (N - 3, (N - 3) * 4, N - 1, (N - 1) * 4)
INTERIOR = (((1 * 7 + 3) * 13 + 5) * 3 + 1,) * 2


@pytest.mark.parametrize("op,message", [
    (skips_last_column_of_last_row, r"buffer %s: 3 of %d elements differ, first element %d \(byte offset %d: .*last element %d \(byte offset %d\)"
     % ((NAME, N) + LAST)),
    (skips_one_interior_element, r"buffer %s: 1 of %d elements differ, first element %d \(byte offset %d: .*last element %d \(byte offset %d\)"
     % (NAME, N, INTERIOR[0], INTERIOR[0] * 4, INTERIOR[0], INTERIOR[0] * 4)),
    (writes_one_past_the_end, r"buffer %s \(payload %d bytes\): back guard, \d bytes damaged, byte offsets \+%d \.\. \+%d " % (NAME, N * 4, N * 4, N * 4 + 3)),
    (writes_one_before_the_start, r"buffer %s \(payload %d bytes\): front guard, \d bytes damaged, byte offsets -4 \.\. -1 " % (NAME, N * 4)),
    (accumulates, r"buffer %s: %d of %d elements differ, first element 0 \(byte offset 0:" % (NAME, N, N)),
], ids=["a-last-column", "b-interior", "c-past-the-end", "d-before-the-start", "e-accumulates"])
def test_a_wrong_op_is_flagged_with_buffer_and_offset(op, message):
    with pytest.raises(AssertionError, match=message):
        wc.two_fill_check(op, op.__name__)


@pytest.mark.parametrize("lead", [4, 2 * 4, 16, 252])
def test_guards_hold_at_every_payload_alignment(lead):
    """lead_bytes: the payload starts at the chosen offset of a 256-byte aligned block, with a full guard in front of it."""
    gb = wc.GuardedBuffers("numpy", 0xA5, lead)
    out = gb.empty(SHAPE)
    assert out.ctypes.data % 256 == lead and gb.records[0]["start"] >= wc.GUARD
    whole = gb.records[0]["whole"]
    assert whole.size - gb.records[0]["start"] - out.nbytes >= wc.GUARD and (whole == 0xA5).all()
    for op in (writes_one_past_the_end, writes_one_before_the_start):
        with pytest.raises(AssertionError, match="guard"):
            wc.two_fill_check(op, "lead %d" % lead, lead_bytes=lead)
    wc.two_fill_check(correct, "lead %d" % lead, lead_bytes=lead)


def test_weakest_alignment_rule():
    f16 = wc.GuardedBuffers("numpy", 0x5A, wc.weakest_alignment)
    ptrs = [f16.empty(10, dt).ctypes.data % 256 for dt in (np.float32, np.float16, np.float16, np.int64, np.float16, np.float16)]
    assert ptrs == [4, 2, 16, 8, 2, 16]
    with pytest.raises(ValueError):
        wc.GuardedBuffers("numpy", 0, 2).empty(4, np.float32)


def test_a_single_fill_is_not_enough():
    """A 0 / 1 mask with a hole where the true value is 0: filled with 0x00 the hole reads as the correct 0; the two fills disagree."""
    truth = (X > 128).astype(np.float32)
    truth[0, 2, 4, 1] = 0.0

    def holed_mask(gb):
        out = gb.empty(SHAPE)
        keep = out[0, 2, 4, 1].copy()
        out[...] = truth
        out[0, 2, 4, 1] = keep
        return (out,)

    gb = wc.GuardedBuffers("numpy", 0x00)
    got, = holed_mask(gb)
    gb.check("single fill")
    np.testing.assert_array_equal(wc.bits(got), wc.bits(truth))            # passes: the blind spot
    with pytest.raises(AssertionError, match=r"1 of %d elements differ, first element %d " % (N, (2 * 13 + 4) * 3 + 1)):
        wc.two_fill_check(holed_mask, "mask")


def test_bits_keeps_nan_payloads_and_widths():
    a = np.frombuffer(np.array([0x7fc00000, 0xffc00001, 0x80000000, 0], np.uint32).tobytes(), np.float32)
    assert wc.bits(a).tolist() == [0x7fc00000, 0xffc00001, 0x80000000, 0] and wc.bits(a).dtype == np.uint32
    assert wc.bits(np.array([-0.0, 1.0], np.float16)).tolist() == [0x8000, 0x3c00]
    assert wc.bits(np.array([-1], np.int64)).tolist() == [0xffffffffffffffff]
    with pytest.raises(TypeError):
        wc.bits(np.zeros(2, np.float64))
    with pytest.raises(AssertionError, match="buffer q: 1 of 4 elements differ, first element 1 "):
        wc.assert_same_bits([("q", a)], [("q", np.frombuffer(np.array([0x7fc00000, 0xffc00000, 0x80000000, 0], np.uint32).tobytes(), np.float32))], "nan")


def test_rows_past_counts_are_not_compared_but_guards_are():
    def op(junk):
        def run(gb):
            idx, counts = gb.empty((2, 5, 4), np.int64), gb.empty(2, np.int64)
            idx[...] = junk
            idx[0, :2], idx[1, :5] = 1, 2
            counts[:] = (2, 9)                          # frame 1 overflowed its 5 rows
            return idx, counts
        return run
    a, b = [wc.specified([wc.Rows(*op(j)(wc.GuardedBuffers("numpy", 0xA5)))]) for j in (7, 8)]
    wc.assert_same_bits(a, b, "rows")
    assert a[1][1].shape == (7, 4) and a[0][1].tolist() == [2, 9]


def test_every_gpu_case_fits_the_poisoned_part_of_the_arena():
    """poison_arena covers a fixed 64 MiB; the arguments any host-form call of a case stages lie inside it."""
    assert len(wcc.CASES) > 100
    worst = max(wcc.CASES, key=lambda c: c.staging_bound())
    for c in wcc.CASES:
        assert c.staging_bound() <= wc.ARENA_POISON_BYTES, (c.id, c.staging_bound())
    print("%d cases; largest staging bound %.1f MiB (%s)" % (len(wcc.CASES), worst.staging_bound() / 2.0 ** 20, worst.id))


def test_the_allocation_patch_leaves_host_operands_untouched(monkeypatch):
    from pysilent_amd import _runtime as rt
    plain = rt._Operand.empty
    op = rt._Operand(np.zeros((1, 2, 3, 1), np.float32), ctx=object())            # (a host operand needs no GPU)
    with wc.guarded(rt, monkeypatch, 0xA5) as gb:
        assert rt._Operand.empty is not plain
        out, ptr = op.empty((2, 3), np.int64)
        flat, _ = op.alloc(3)
        assert type(out) is np.ndarray and out.dtype == np.int64 and out.shape == (2, 3) and ptr.value == out.ctypes.data
        assert type(flat) is np.ndarray and flat.shape == (18,) and flat.dtype == np.float32
        assert gb.records == [] and wc.CURRENT == [gb]
    assert rt._Operand.empty is plain and wc.CURRENT == []
