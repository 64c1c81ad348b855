"""What silent_pyramid_plan_create_ex BUILDS, without a GPU: tests/plan_tables_host_main.cpp -- the library's host side under ASan + UBSan
as a stand-alone program, run as a child process -- prints the planner's decisions, a hash of the text of every scalar of a plan and of
every device pointer as an offset (--text: that text), size and hash of the bytes of its four table allocations and the per-launch
decomposition of the walk; tests/golden/plan_tables.txt is that output as recorded with the single-function planner, before it was split
into the steps of csrc/silent_plan_build.h (tests/plan_geometry.py pins the ROUTES a plan takes, the GPU
suites the pyramids its tables produce; this pins the tables).  And its allocation-failure exits, with LeakSanitizer on."""
import math
import os
import subprocess
import sys

import pytest

import plan_geometry as pg
from conftest import ROOT

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_tables.txt")
F64 = 1                    # SILENT_PLAN_ACCUM_F64
NO_UNION = 4               # SILENT_TUNE_PYRAMID bit 4: no union walk plan
E5 = math.e ** .5


def line(name, hw, channels, levels, flags=0, tune=0, n_levels=None):
    """name H W channels flags pyramid_tune n_levels <8 integers per level>"""
    assert " " not in name
    vals = [int(v) for l in levels for v in l]
    return " ".join([name] + [str(v) for v in [hw[0], hw[1], channels, flags, tune, len(levels) if n_levels is None else n_levels] + vals])


def generated_plans():
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    plans = [("classic_1080_%s_%d" % (tag, n), (1080, 1920), classic_levels((1080, 1920), r, n))
             for tag, r, n in (("2", 2.0, 7), ("e.5", E5, 7), ("2.5", 2 ** .5, 7), ("2.5", 2 ** .5, 12))]
    plans += [("reference_%dx%d_%dx%d" % (hw + c), hw, reference_levels(hw, c, E5))
              for hw, c in (((1080, 1920), (192, 108)), ((1080, 1920), (120, 68)), ((480, 640), (288, 192)))]
    return plans


def table_lines():
    out = []
    for name in sorted(pg.CASES):
        case = pg.CASES[name]
        out += [line("%s/c%d" % (name, c), case["frame"], c, case["levels"]) for c in (1, 3)]
        out.append(line(name + "/c1_f64", case["frame"], 1, case["levels"], flags=F64))
        out.append(line(name + "/c3_no_union", case["frame"], 3, case["levels"], tune=NO_UNION))
    for seed in pg.RANDOM_SEEDS:
        hw, channels, levels = pg.random_case(seed)
        out.append(line("random_%02d/c%d" % (seed, channels), hw, channels, levels))
    for name, hw, levels in generated_plans():
        out += [line("%s/c%d" % (name, c), hw, c, levels) for c in (1, 3)]
    # ---- the invalid-argument exits
    lv = pg.ladder((0, 0, 40, 57), 2.0, 2)
    out += [line("null_levels", (40, 57), 3, lv), line("null_out", (40, 57), 3, lv),
            line("unknown_flag_bits", (40, 57), 1, lv, flags=2), line("unknown_flag_bits_beside_f64", (40, 57), 1, lv, flags=F64 | 8),
            line("frame_h_0", (0, 57), 1, lv), line("frame_w_negative", (40, -1), 1, lv), line("frame_above_2^30_pixels", (40000, 40000), 1, lv),
            line("channels_2", (40, 57), 2, lv), line("channels_4", (40, 57), 4, lv), line("f64_with_3_channels", (40, 57), 3, lv, flags=F64),
            line("n_levels_0", (40, 57), 1, [], n_levels=0), line("n_levels_17", (40, 57), 1, [lv[0]] * 17),
            line("level_outside_the_frame", (40, 57), 1, [lv[0], (1, 0, 40, 57, 20, 29, 20, 29)]),
            line("level_outside_the_frame_x", (40, 57), 3, [(0, 30, 40, 28, 20, 14, 20, 14)]),
            line("level_zoom_0", (40, 57), 1, [lv[0], (0, 0, 40, 57, 0, 29, 20, 29)]),
            line("level_canvas_0", (40, 57), 1, [(0, 0, 40, 57, 20, 29, 20, 0)])]
    return out


def fault_lines():
    """--alloc-faults: the 3-channel classic ladder and the 1-channel reference layout of tests/sanitizer_worker.py, and an F64 plan."""
    from pysilent_amd.util.zoom.from_image import classic_levels, reference_levels
    return [line("classic/c3", (64, 96), 3, classic_levels((64, 96), 2.0, 4)),
            line("reference/c1", (64, 96), 1, reference_levels((64, 96), (24, 16), E5)),
            line("sub_in_316_2.00/c1_f64", pg.FA, 1, pg.CASES["sub_in_316_2.00"]["levels"], flags=F64)]


def run(lines, *args):
    """The driver on `lines`; LeakSanitizer stays ON (the default of a stand-alone ASan program).  alloc_dealloc_mismatch: the plan is a
    new (std::nothrow) object and the host shim's operator delete is free(), as in the other host-side sanitizer runs."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    env = dict(os.environ, ASAN_OPTIONS="alloc_dealloc_mismatch=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([B.build_host_driver("plan_tables")] + list(args), input="\n".join(lines) + "\n", env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "Sanitizer" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]
    return p.stdout.strip().split("\n")


if __name__ == "__main__":           # python tests/test_plan_tables_host.py > tests/golden/plan_tables.txt (the lines of the driver as built)
    print("\n".join(run(table_lines())))
    sys.exit(0)


@pytest.fixture(scope="module")
def tables():
    return run(table_lines())


@needs_hipcc
def test_every_plan_is_built_as_recorded(tables):
    """Line by line: scalars, pointer offsets, table bytes and launch decompositions of 46 geometry cases x (1 channel, 3 channels, F64,
    union plan forbidden), 40 random draws, the 1080p ladders and the reference's crop layouts; status and message of every
    invalid-argument exit."""
    want = open(GOLDEN).read().strip().split("\n")
    assert len(want) == len(table_lines()) == 4 * len(pg.CASES) + len(pg.RANDOM_SEEDS) + 2 * 7 + 16
    assert [l.split(" | ")[0] for l in tables] == [l.split(" ")[0] for l in table_lines()]
    for got, rec in zip(tables, want):         # (a "scalars" hash that moved: run the driver with --text on both builds and compare)
        assert got == rec, got.split(" | ")[0]
    assert len(tables) == len(want)


@needs_hipcc
def test_the_recorded_plans_take_the_recorded_routes(tables):
    """The golden agrees with plan_geometry.ROUTES (so neither is a recording of another planner), and its hashes are of tables that
    exist: every successful plan has tap tables, F64 plans float64 tables, stream and walk tables exactly where the route says."""
    by_name = {l.split(" | ")[0]: l.split(" | ") for l in tables}
    for name, ((stream1, _), (_, (n_plans, px))) in pg.ROUTES.items():
        for tag, stream, plans in (("c1", stream1, 0), ("c3", False, n_plans), ("c1_f64", stream1, 0)):
            f = by_name["%s/%s" % (name, tag)]
            assert f[1] == "0", f[:3]
            field = {x.split(" ")[0]: x for x in f[2:]}
            assert field["stream"].startswith("stream %d " % stream), (name, tag)
            assert field["walk"].startswith("walk %d " % (plans > 0)), (name, tag)
            if plans:
                assert field["walk"].startswith("walk 1 px %d " % px) and " plans %d " % plans in field["walk"], (name, tag)
            assert f[5].startswith("scalars ") and [b != "-" for b in f[6:10]] == [True, tag == "c1_f64", stream, plans > 0], (name, tag)
    failed = [f for f in by_name.values() if f[1] != "0"]
    assert len(failed) == 16 and all(f[2].startswith("silent_pyramid_plan_create: ") for f in failed)
    assert all(f[3] == ("out untouched" if f[0] in ("null_levels", "null_out") else "out NULL") for f in failed)
    assert {f[1] for f in failed} == {"-1", "-4"}                    # SILENT_E_INVALID, SILENT_E_UNSUPPORTED


@needs_hipcc
def test_an_allocation_failure_anywhere_in_plan_creation_is_nomem_and_leaks_nothing():
    """silent_host_fail_new_after(k) for k = 1, 2, ... until the plan is created: SILENT_E_NOMEM, *out NULL, and -- LeakSanitizer on --
    neither the plan nor a table allocation is lost."""
    out = run(fault_lines(), "--alloc-faults")
    assert len(out) == 3, out
    for l in out:
        f = l.split(" | ")
        assert f[1].startswith("created with allocation ") and int(f[2].split(" ")[0]) >= 3, l
