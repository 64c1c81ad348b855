"""Every entry point writes ALL of its output and NOTHING else (tests/write_coverage.py; the cases: tests/write_coverage_cases.py).

The parity tests compare what the kernels compute; the way results are allocated hides which elements they computed.  Host forms
stage their outputs at fixed offsets of one persistent arena, device results come from torch.empty, and both hand a second call of
the same geometry the bytes of the first: an element a route skips (a tile tail, a ragged last column, a 1-row level) still holds the
previous route's correct value.  And nothing surrounds an output, so a store past its end lands in allocator padding.  Here

  * the device forms run on results that lie between 256-byte guards, everything filled with 0xA5 and then with 0x5A: the two runs
    and an ordinary run must agree bit for bit, the guards must be intact; default-route cases run once more with every result at
    the weakest alignment include/silent_hip.h allows (write_coverage.weakest_alignment);
  * the host forms run with the staging arena filled with -7.25 and then with 1.0 before EVERY library call (a case makes several
    calls of one geometry, and a call must not land on its predecessor's answer), and must return the device form's bits;
  * every call of an entry point that keeps intermediates in the context workspace runs right after the same call on an all-zero
    input of its own geometry and right after one on other noise, and must return the same bits both times.

Compared in part only: keypoint rows past counts[f] (write_coverage.Rows; include/silent_hip.h:344-346).  An in-place boosting state
is prefilled by the caller, so only its guards can speak.

Out of scope: the displayer (pinned host result slots, a HIP graph of its own), LineEndPipeline (owns its buffers, has a placement
tuner) and bench.py."""
import pytest

import write_coverage as wc
import write_coverage_cases as wcc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from pysilent_amd import _runtime
    if _runtime.device_count() == 0:
        pytest.skip("no GPU")
    return _runtime


def _calls(rt, case, place, inputs=None):
    return case.calls(rt, *[place(rt, x) for x in (case.inputs() if inputs is None else inputs)])


def _run(call):
    """One call, synchronised: its raw results."""
    import torch
    res = call()
    torch.cuda.synchronize()
    return res


def _named(per_call):
    """[(name, ndarray)] of the specified parts of the results of a list of calls."""
    return [na for i, res in enumerate(per_call) for na in wc.specified(res, "call %d " % i)]


def _device_baseline(rt, case):
    base = [_named([_run(c)]) for c in _calls(rt, case, wcc.on_device)]
    assert base and all(base), case.id
    return base


def _flat(per_call_named):
    return [(("call %d " % i) + n[len("call 0 "):], a) for i, named in enumerate(per_call_named) for n, a in named]


def test_the_torch_backend_reports_a_hole_and_a_stray_store(rt):
    """What tests/test_write_coverage.py shows on the numpy backend, on device memory (torch ops play the wrong kernel)."""
    import torch
    x = torch.arange(1, 2 * 7 * 13 * 3 + 1, dtype=torch.float32, device="cuda:0").reshape(2, 7, 13, 3)

    def run(fill, hole=False, stray=0):
        gb = wc.GuardedBuffers("torch", fill, wc.weakest_alignment)
        out = gb.empty(x.shape)
        assert out.data_ptr() % 256 == 4 and (wc.bits(out) == fill * 0x01010101).all()
        keep = out[1, 6, 12, 2].clone()
        out.copy_(x)
        if hole:
            out[1, 6, 12, 2] = keep
        if stray:
            r = gb.records[0]
            r["whole"][r["start"] + (r["nbytes"] if stray > 0 else -1)] = 0
        return gb, wc.specified([out])

    (a, ra), (b, rb) = run(0xA5), run(0x5A)
    a.check("clean"), b.check("clean")
    wc.assert_same_bits(ra, rb, "clean")
    with pytest.raises(AssertionError, match=r"1 of 546 elements differ, first element 545 \(byte offset 2180"):
        wc.assert_same_bits(run(0xA5, hole=True)[1], run(0x5A, hole=True)[1], "hole")
    with pytest.raises(AssertionError, match=r"back guard, 1 bytes damaged, byte offsets \+2184 \.\. \+2184 "):
        run(0xA5, stray=1)[0].check("stray")
    with pytest.raises(AssertionError, match=r"front guard, 1 bytes damaged, byte offsets -1 \.\. -1 "):
        run(0x5A, stray=-1)[0].check("stray")


@pytest.mark.parametrize("case", wcc.CASES, ids=wcc.IDS)
def test_device_form_writes_all_and_only_its_output(rt, monkeypatch, case):
    base = _flat(_device_baseline(rt, case))
    runs = [(fill, 0) for fill in wc.FILLS] + ([(wc.FILLS[0], wc.weakest_alignment)] if case.default_route else [])
    got = []
    for fill, lead in runs:
        what = "%s, fill 0x%02X%s" % (case.id, fill, ", weakest alignment" if lead else "")
        with wc.guarded(rt, monkeypatch, fill, lead) as gb:
            raw = [_run(c) for c in _calls(rt, case, wcc.on_device)]
        for i, res in enumerate(raw):
            for t in wc.buffers_of(res):
                assert gb.owns(t), "%s: a result of call %d was not allocated between guards" % (what, i)
        got.append(_named(raw))
        gb.check(what)
        wc.assert_same_bits(got[-1], base, what + " against an ordinary run")
    wc.assert_same_bits(got[1], got[0], "%s: fill 0x5A against fill 0xA5" % case.id)


@pytest.mark.parametrize("case", wcc.CASES, ids=wcc.IDS)
def test_host_form_does_not_return_stale_arena_bytes(rt, case):
    assert case.staging_bound() <= wc.ARENA_POISON_BYTES
    base = _device_baseline(rt, case)
    for named in base:
        assert sum(a.nbytes for _, a in named) <= case.out_bytes, (case.id, "the staging bound of the case table is too small")
    got = []
    for value in (-7.25, 1.0):
        raw = []
        for call in _calls(rt, case, wcc.on_host):
            wc.poison_arena(rt, value)
            raw.append(call())
        got.append(_named(raw))
        wc.assert_same_bits(got[-1], _flat(base), "%s: host form after the arena held %g, against the device form" % (case.id, value))
    wc.assert_same_bits(got[1], got[0], "%s: host form after an arena of 1.0 against after an arena of -7.25" % case.id)


WORKSPACE = [c for c in wcc.CASES if c.workspace]


@pytest.mark.parametrize("case", WORKSPACE, ids=[c.id for c in WORKSPACE])
def test_results_do_not_depend_on_the_previous_call(rt, case):
    base = _device_baseline(rt, case)
    xs = _calls(rt, case, wcc.on_device)
    ys = [_calls(rt, case, wcc.on_device, [wcc.other_values(x, kind) for x in case.inputs()]) for kind in (1, 2)]
    assert len(xs) == len(ys[0]) == len(ys[1]) == len(base)
    for i, x_call in enumerate(xs):
        got = []
        for kind, y_calls in zip(("an all-zero input", "other noise"), ys):
            _run(y_calls[i])
            got.append(_named([_run(x_call)]))
            wc.assert_same_bits(got[-1], base[i], "%s call %d right after the same call on %s" % (case.id, i, kind))
        wc.assert_same_bits(got[1], got[0], "%s call %d: after other noise against after an all-zero input" % (case.id, i))
