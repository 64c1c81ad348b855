"""What the keypoint tail PLANS on the host, without a GPU: tests/kp_tables_host_main.cpp -- the library's host side under ASan + UBSan as a
stand-alone program, run as a child process -- drives region_prepare and select_prepare (csrc/silent_peaks_api.hip) and prints every field
of the region tables, the value-summary geometry, the block counts, every piece of the keypoint workspace as an offset, the zero range
and the workspace's capacity; the centroid cell tables and the boost parameters likewise.  tests/golden/kp_tables.txt is that output as
recorded at the commit BEFORE the planning moved into csrc/silent_peaks_plan.h and the workspace was laid out by a carver.  The driver
itself checks every accepted layout (aligned, disjoint, inside the total, the zero range exactly the four zeroed pieces)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kp_tables.txt")
MAX_LEVELS = 16            # SILENT_MAX_LEVELS


def case(name, levels, n_frames=1, sparse_th=0, pv_ws=0, reserve=0, n_levels=None):
    """name n_frames sparse_th pv_ws reserve n_levels <h w rh rw per level>; a level is (h, w, rh, rw)"""
    assert " " not in name
    vals = [name, n_frames, sparse_th, pv_ws, reserve, len(levels) if n_levels is None else n_levels] + [v for l in levels for v in l]
    return " ".join(str(v) for v in vals)


REF = (192, 288, 96, 144)          # the reference's two windows per axis
SMALL = (9, 7, 5, 4)
SUMMARY = [(37, 53, 19, 27), (19, 27, 10, 14)]     # heights no multiple of a tile height (4, 16, 32), odd widths
WIN4, WIN6 = (16, 16, 4, 4), (16, 16, 3, 3)        # kMaxWin windows per axis: cell tables; 6: the general path


def table_lines():
    out = [case("smallest", [(1, 1, 1, 1)]), case("one_row", [(1, 37, 1, 19)]), case("one_column", [(37, 1, 19, 1)])]
    out += [case("reference_windows_%d" % n, [REF], n_frames=n, sparse_th=16) for n in (1, 3, 32)]
    out += [case("windows_4", [WIN4], sparse_th=16), case("windows_6_general", [WIN6], sparse_th=16), case("unequal_pads", [(17, 17, 5, 5)]),
            case("stride_above_extent", [(8, 8, 20, 20)]), case("general_beside_cell_tables", [WIN4, WIN6, SMALL], n_frames=2, sparse_th=16, pv_ws=1),
            case("max_levels", [(3, 5, 2, 3)] * MAX_LEVELS, n_frames=2, sparse_th=4)]
    out += [case("summary_th%d_pv%d" % (th, pv), SUMMARY, n_frames=3, sparse_th=th, pv_ws=pv) for th in (0, 4, 16, 32) for pv in (0, 1)]
    out += [case("reserve_%d" % r, [SMALL], reserve=r) for r in (0, 1, 256, 257)]
    out += [case("frames_%d" % n, [(2, 2, 1, 1)] * 2, n_frames=n, sparse_th=16) for n in (65535, 65536)]
    # ---- refusals
    out += [case("n_levels_0", [], n_levels=0), case("n_levels_above_max", [SMALL] * (MAX_LEVELS + 1)), case("level_extent_0", [SMALL, (0, 5, 1, 1)]),
            case("region_extent_0", [SMALL, (5, 5, 0, 2)]), case("n_frames_0", [SMALL], n_frames=0)]
    return out


def layout_lines():
    """Sizes that cannot be allocated: the layout function alone (pure), checked by the driver.  The last one is where a frame's summary
    reaches 2^31 entries (16 levels x 8192 tile rows x 16384 pixel pairs) and the sparse layout is dropped."""
    p1080 = [(1080 >> l, 1920 >> l, (1080 >> l) // 2 + 1, (1920 >> l) // 2 + 1) for l in range(5)]
    return [case("32x1080p_5_levels", p1080, n_frames=32, sparse_th=16, pv_ws=1), case("65535x4K", [(2160, 3840, 1080, 1920)], n_frames=65535, sparse_th=16, pv_ws=1),
            case("summary_2^31_entries", [(32768, 32768, 16384, 16384)] * MAX_LEVELS, sparse_th=4)]


CELL_LINES = ["cells_1x1 3 3 1 1 1", "cells_7x10 3 3 1 7 10", "cells_192x288 3 3 1 192 288", "cells_3_levels 3 3 3 1 1 7 10 192 288", "cells_rh_0 0 3 1 7 10",
              "cells_rw_0 3 0 1 7 10"]
# name recovery_mode exhaustion_max excitation_max amount percentage visualize
BOOST_LINES = ["boost_mode_%d %d 1 1 10 0.8 %d" % (m, m, m & 1) for m in (0, 1, 2, 3, 4)] + ["boost_asymmetric 3 0.5 2 7 0.25 1", "null_params 1 1 1 10 0.8 0"]


def run(lines, *args):
    """The driver on `lines`; LeakSanitizer stays ON (the default of a stand-alone ASan program)."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    env = dict(os.environ, ASAN_OPTIONS="alloc_dealloc_mismatch=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([B.build_host_driver("kp_tables")] + list(args), input="\n".join(lines) + "\n", env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "Sanitizer" not in p.stdout and "runtime error" not in p.stdout and "CHECK FAILED" not in p.stdout, p.stdout[-4000:]
    return p.stdout.strip().split("\n")


def all_lines():
    return run(table_lines()) + run(CELL_LINES, "--cells") + run(BOOST_LINES, "--boost")


if __name__ == "__main__":           # python tests/test_kp_tables_host.py > tests/golden/kp_tables.txt (the lines of the driver as built)
    print("\n".join(all_lines()))
    sys.exit(0)


@pytest.fixture(scope="module")
def tables():
    return all_lines()


@needs_hipcc
def test_the_tail_is_planned_as_recorded(tables):
    """Line by line: region tables, summary geometry, block counts, workspace offsets, zero range and capacity of 26 cases through both
    prepares, 5 refusals with their messages, 6 cell-table and 7 boost-parameter cases.  The driver exited 0: every accepted layout
    passed its own checks, and no sanitizer reported."""
    want = open(GOLDEN).read().strip().split("\n")
    accepted = [l for l in table_lines()[:-5]]
    n_level_lines = sum(int(l.split(" ")[5]) for l in accepted)
    assert len(want) == 2 * (2 * len(accepted) + n_level_lines) + 2 * 5 + len(CELL_LINES) + len(BOOST_LINES) == 233
    for got, rec in zip(tables, want):
        assert got == rec, got.split(" | ")[0]
    assert len(tables) == len(want)


@needs_hipcc
def test_the_recorded_plans_take_the_recorded_decisions(tables):
    """The golden is of the decisions the cases were chosen for (so it is no recording of some other planner): which cases run the general
    path, where the sparse layout is dropped, what is refused and how."""
    last = {}
    for l in tables:
        f = l.split(" | ")
        last[f[0]] = f
    def general(name): return [x for x in last[name + " select"] if x.startswith("general ")][0].split(" ")[1] == "1"
    def entries(name): return int([x for x in last[name + " select"] if x.startswith("sum ")][0].split(" ")[-1])
    assert not general("windows_4") and general("windows_6_general") and general("general_beside_cell_tables") and not general("unequal_pads")
    assert entries("windows_4") > 0 and entries("windows_6_general") == 0 and entries("general_beside_cell_tables") == 0
    assert entries("frames_65535") > 0 and entries("frames_65536") == 0
    assert all((entries("summary_th%d_pv%d" % (th, pv)) > 0) == (th > 0) for th in (0, 4, 16, 32) for pv in (0, 1))
    for name in ("n_levels_0", "n_levels_above_max", "level_extent_0", "region_extent_0", "n_frames_0"):
        for half in ("region", "select"):
            f = last["%s %s" % (name, half)]
            assert f[1] == "-1" and f[2].startswith("kp_tables: "), f
    assert last["cells_rh_0 cells"][1:] == ["-1", "kp_tables: region extents must be >= 1"] == last["cells_rw_0 cells"][1:]
    assert [last["boost_mode_%d boost" % m][1] for m in (0, 1, 2, 3, 4)] == ["-1", "0", "0", "0", "-1"]
    assert last["null_params boost"][1:] == ["-1", "silent_boosting_step: NULL params"]


@needs_hipcc
def test_the_layout_holds_on_sizes_nobody_can_allocate():
    """32 x 1080p on five levels, 65535 x 4K, a frame summary of 2^31 entries: the pure layout function, and the driver's checks of it."""
    out = run(layout_lines(), "--layout")
    assert len(out) == 3 and all(l.split(" | ")[1] == "ok" for l in out), out
    assert [int(l.split(" entries ")[1]) > 0 for l in out] == [True, True, False], out
