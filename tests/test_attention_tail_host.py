"""The attention tail (silent_attention_tail, LineEndPipeline(attention=True)) without a GPU: the constructor's refusals; the geometry
silent_attention_extents gives against a restatement written here (ceil(h / rh), the float32 division and truncation of the half extents,
TF SAME firsts, float32 scales); argument validation and the planned tables of silent_attention_tail through
tests/attention_tail_host_main.cpp -- the library's host side under ASan + UBSan as a stand-alone program, run as a child process,
which checks every accepted workspace layout itself (aligned, disjoint, inside the total), the largest one included."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
MAX_LEVELS = 16
DIV = np.float32(math.e ** .5)            # recognition_testing.py:82-83
GEOMETRIES = {"A": [(16, 24)] * 2, "B": [(37, 53), (19, 27), (10, 14), (5, 7), (2, 2)], "C": [(4, 300), (3, 65), (3, 64), (3, 63), (65, 2)],
              "D": [(64, 96)], "E": [(17, 68)]}          # D, E: one level -- with n_frames > 1 the shape of a displayer frame
REGIONS = [(3, 3), (2, 3), (4, 5), (7, 7)]
CONFIG3 = [(1080, 1920), (540, 960), (270, 480), (135, 240), (68, 120), (34, 60)]      # 1080p, six levels at scale 2
REFERENCE = [(192, 288)] * 4


# ----------------------------------------------------------------------------- the geometry, restated

def bits(x):
    return int(np.float32(x).view(np.uint32))


def geometry(levels, region, div=DIV):
    """Per level: cells, half, cells2 as (h, w); SAME firsts (y, x) of both cell grids; float32 cell scales of both as bits; float32 resize
    scales as bits."""
    rh, rw = region
    out = []
    for h, w in levels:
        half = (int(np.float32(h) / np.float32(div)), int(np.float32(w) / np.float32(div)))     # float32 division, truncated
        row = {"half": half}
        for name, (eh, ew) in (("", (h, w)), ("2", half)):
            ch, cw = -(-eh // rh), -(-ew // rw)
            row["cells" + name] = (ch, cw)
            # tf.nn.*_pool SAME: pad_total = max((out - 1) * stride + window - in, 0), pad_before = pad_total // 2
            row["first" + name] = (-(max((ch - 1) * rh + rh - eh, 0) // 2), -(max((cw - 1) * rw + rw - ew, 0) // 2))
            row["scale" + name] = (bits(np.float32(ch) / np.float32(eh)), bits(np.float32(cw) / np.float32(ew)))
        row["resize"] = (bits(np.float32(h) / np.float32(half[0])), bits(np.float32(w) / np.float32(half[1])))
        out.append(row)
    return out


def prefix(values):
    out, s = [], 0
    for v in values:
        out.append(s)
        s += v
    return out, s


def case(name, levels, n_frames=1, region=(3, 3), div=DIV, mode=1, visualize=1, want=15, n_levels=None):
    """name n_frames rh rw resize_div recovery_mode visualize want n_levels <h w per level>"""
    assert " " not in name
    d = div if isinstance(div, str) else "%.9g" % np.float32(div)
    vals = [name, n_frames, region[0], region[1], d, mode, visualize, want, len(levels) if n_levels is None else n_levels] + [v for l in levels for v in l]
    return " ".join(str(v) for v in vals)


def run(lines, *args):
    """The driver on ``lines``; LeakSanitizer stays ON (the default of a stand-alone ASan program)."""
    sys.path.insert(0, os.path.join(ROOT, "pysilent_amd", "csrc"))
    import build as B
    env = dict(os.environ, ASAN_OPTIONS="alloc_dealloc_mismatch=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([B.build_host_driver("attn_tables")] + list(args), input="\n".join(lines) + "\n", env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "Sanitizer" not in p.stdout and "runtime error" not in p.stdout and "CHECK FAILED" not in p.stdout, p.stdout[-4000:]
    return p.stdout.strip().split("\n")


# ----------------------------------------------------------------------------- the constructor

@pytest.mark.parametrize("kw, word", [
    (dict(mode="gray"), "mode"), (dict(mode="rgb", value_map=False), "value_map"), (dict(mode="rgb", overlap=True), "overlap"),
    (dict(mode="rgb", overlap="auto"), "overlap"), (dict(mode="rgb", overlap="force"), "overlap"),
    (dict(mode="rgb", centroid_region=(0, 3)), "centroid_region"), (dict(mode="rgb", centroid_region=(3, -1)), "centroid_region"),
    (dict(mode="rgb", n_levels=7), "half extent"), (dict(mode="rgb", input_based_recovery=False, constant_recovery=False), "recovery")])
def test_the_constructor_refuses_before_any_gpu_work(kw, word, monkeypatch):
    """Every refusal is a ValueError that names ``attention``; none of them reaches torch or the GPU (torch.device would be the first
    call: it is made to fail)."""
    import torch
    from pysilent_amd.pipeline import LineEndPipeline

    def no_torch(*a, **k):
        raise AssertionError("torch work before the refusal")
    monkeypatch.setattr(torch, "device", no_torch)
    with pytest.raises(ValueError, match="attention") as e:
        LineEndPipeline((64, 96), attention=True, **kw)
    assert word in str(e.value), str(e.value)


def test_the_keywords_belong_to_the_call_and_init_keeps_its_parameters():
    """The five keywords are taken off the call's arguments (pipeline.ATTENTION_KEYWORDS); a misspelt one is still a TypeError."""
    import inspect
    from pysilent_amd import pipeline
    names = list(inspect.signature(pipeline.LineEndPipeline.__init__).parameters)
    assert list(pipeline.ATTENTION_KEYWORDS) == ["attention", "centroid_region", "input_based_recovery", "constant_recovery", "attention_visualize"]
    assert not set(pipeline.ATTENTION_KEYWORDS) & set(names)
    assert [pipeline.ATTENTION_KEYWORDS[k] for k in pipeline.ATTENTION_KEYWORDS] == [False, (3, 3), False, True, True]
    with pytest.raises(TypeError, match="attentoin"):
        pipeline.LineEndPipeline((64, 96), mode="rgb", attentoin=True)


# ----------------------------------------------------------------------------- silent_attention_extents

@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("name", sorted(GEOMETRIES) + ["config3", "reference"])
def test_the_extents_are_the_restated_geometry(name, region):
    from pysilent_amd import _runtime as rt
    levels = dict(GEOMETRIES, config3=CONFIG3, reference=REFERENCE)[name]
    cells, half, cells2 = rt.attention_extents(levels, rt.attention_params(region))
    want = geometry(levels, region)
    assert cells == [g["cells"] for g in want] and half == [g["half"] for g in want] and cells2 == [g["cells2"] for g in want]


def test_the_geometries_are_the_ones_asked_for():
    """A: SAME padding on both sides at 3 x 3, half map 9 x 14; B: down to a 1 x 1 half map; (7, 7): a stride above a half map.
    D and E are single levels, the shape of a displayer frame.  D (64, 96) is the canvas of the displayer tests: exactly one row of 64 x 64
    tiles, half map 38 x 58.  E (17, 68): the width is just past one 64-column tile; row 16 is the only row of a tile's second wave and
    the first of a group of four rows; half map 10 x 41, and at region (7, 7) -- the worst case -- cells 3 x 10 and cells2 2 x 6.  Every
    half extent of both is >= 1 at every region in REGIONS, so the per-op sequence (resize_nearest, centroids) accepts them all and
    no GPU case of tests/test_gpu_attention_tail.py is skipped."""
    d, e = geometry(GEOMETRIES["D"], (7, 7))[0], geometry(GEOMETRIES["E"], (7, 7))[0]
    assert d["half"] == (38, 58) and -(-64 // 64) == 1 and -(-96 // 64) == 2
    assert e["half"] == (10, 41) and e["cells"] == (3, 10) and e["cells2"] == (2, 6) and -(-68 // 64) == 2 and 17 % 16 == 1
    for name in "DE":
        for region in REGIONS:
            for g in geometry(GEOMETRIES[name], region):
                assert min(g["half"]) >= 1 and min(g["cells"]) >= 1 and min(g["cells2"]) >= 1, (name, region, g)
    a, b = geometry(GEOMETRIES["A"], (3, 3)), geometry(GEOMETRIES["B"], (3, 3))
    assert a[0]["half"] == (9, 14) and a[0]["first"] == (-1, 0) and a[0]["cells"] == (6, 8)
    assert b[-1]["half"] == (1, 1) and b[-1]["cells2"] == (1, 1)
    assert any(g["half"][0] < 7 or g["half"][1] < 7 for g in geometry(GEOMETRIES["B"], (7, 7)))
    assert float(DIV) == pytest.approx(1.6487212707, abs=1e-7)


def test_the_extents_are_refused_like_the_tail():
    from pysilent_amd import _lib, _runtime as rt
    ok = rt.attention_params()
    for levels, params, word in (([(1, 5)], ok, "half extent"), ([(5, 1)], ok, "half extent"), ([(0, 5)], ok, "extent"), ([(5, -2)], ok, "extent"),
                                 ([], ok, "n_levels"), ([(9, 9)] * (MAX_LEVELS + 1), ok, "n_levels"),
                                 ([(9, 9)], rt.attention_params(resize_div=0.5), "resize_div"),
                                 ([(9, 9)], rt.attention_params(resize_div=float("nan")), "resize_div"),
                                 ([(9, 9)], rt.attention_params(resize_div=float("inf")), "resize_div")):
        with pytest.raises(ValueError, match="silent_attention_extents") as e:
            rt.attention_extents(levels, params)
        assert word in str(e.value), str(e.value)
    bad = rt.attention_params()
    bad.region_w = 0
    with pytest.raises(ValueError, match="region extents must be >= 1"):
        rt.attention_extents([(9, 9)], bad)
    with pytest.raises(ValueError, match="region extents must be >= 1"):
        rt.attention_params((3, 0))
    assert _lib.load().silent_attention_extents(None, 1, None, None, None, None) == _lib.SILENT_E_INVALID


# ----------------------------------------------------------------------------- the driver: planned tables

TABLE_CASES = [("%s_%dx%d_f%d" % (g, r[0], r[1], n), GEOMETRIES[g], n, r) for g in sorted(GEOMETRIES) for r in REGIONS for n in (1, 3)]
TABLE_CASES += [("max_levels", [(5, 9)] * MAX_LEVELS, 2, (3, 3)), ("reference_f32", REFERENCE, 32, (3, 3))]


@pytest.fixture(scope="module")
def tables():
    lines = [case(n, lv, f, r, visualize=i & 1, mode=1 + i % 3) for i, (n, lv, f, r) in enumerate(TABLE_CASES)]
    lines += [case("no_half", GEOMETRIES["B"], 3, want=13), case("state_only", GEOMETRIES["B"], 3, want=0), case("no_dist", GEOMETRIES["C"], 1, want=14)]
    out = {}
    for l in run(lines):
        f = l.split(" | ")
        out.setdefault(f[0].split(" ")[0], []).append(f)
    return out


@needs_hipcc
@pytest.mark.parametrize("name, levels, n_frames, region", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_the_tables_are_the_restated_geometry(tables, name, levels, n_frames, region):
    rows = tables[name]
    assert rows[0][1] == "0" and len(rows) == len(levels) + 2, rows[0]
    want = geometry(levels, region)
    half = [g["half"] for g in want]
    tiles1, n1 = prefix([-(-h // 64) * -(-w // 64) for h, w in levels])
    tiles2, n2 = prefix([-(-h // 64) * -(-w // 64) for h, w in half])
    tilesc, nc = prefix([-(-(g["cells"][0] * g["cells"][1]) // 1024) for g in want])
    px1, fpx1 = prefix([h * w for h, w in levels])
    px2, fpx2 = prefix([h * w for h, w in half])
    c1, fc1 = prefix([g["cells"][0] * g["cells"][1] for g in want])
    c2, fc2 = prefix([g["cells2"][0] * g["cells2"][1] for g in want])
    for l, (row, g) in enumerate(zip(rows[1:-1], want)):
        assert row[0] == "%s L%d" % (name, l)
        assert row[1] == "cells %d %d half %d %d cells2 %d %d" % (g["cells"] + g["half"] + g["cells2"]), (name, l, row[1])
        assert row[2] == "first %d %d %d %d" % (g["first"] + g["first2"]), (name, l, row[2])
        assert row[3] == "scale %08x %08x %08x %08x" % (g["scale"] + g["scale2"]), (name, l, row[3])
        assert row[4] == "resize %08x %08x" % g["resize"], (name, l, row[4])
        assert row[5] == "tiles %d %d %d" % (tiles1[l], tiles2[l], tilesc[l]), (name, l, row[5])
        assert row[6] == "off %d %d %d %d" % (px1[l], px2[l], c1[l], c2[l]), (name, l, row[6])
    plan = rows[-1]
    assert plan[1] == "blocks %d %d %d" % (n1 * n_frames, n2 * n_frames, nc * n_frames), plan
    assert plan[2] == "cells %d %d" % (fc1 * n_frames, fc2 * n_frames) and plan[3] == "px %d %d" % (fpx1, fpx2), plan
    up = lambda b: -(-b // 256) * 256
    cells, cells2 = fc1 * n_frames, fc2 * n_frames
    offs = prefix([up(cells * 8), up(cells2 * 8), up(cells * 4), up(cells * 4)])
    assert plan[4] == "ws cxy %d cxy2 %d imp %d m %d total %d" % (tuple(offs[0]) + (offs[1],)), plan
    assert offs[1] <= 24 * (cells + cells2) + 4 * 256


@needs_hipcc
def test_outputs_nobody_asked_for_are_not_planned(tables):
    """centroids2_out == NULL: no cell, block or workspace byte of the half map; only the state: the cell chunks alone."""
    def field(name, i):
        return [int(v) for v in tables[name][-1][i].split(" ")[1:]]
    assert field("no_half", 1)[1] == 0 and field("no_half", 2)[1] == 0 and field("no_half", 1)[0] > 0
    assert field("state_only", 1)[:2] == [0, 0] and field("state_only", 1)[2] > 0 and field("state_only", 2)[1] == 0
    assert field("no_dist", 1)[0] == 0 and field("no_dist", 1)[1] > 0
    ws = tables["no_half"][-1][4].split(" ")
    assert int(ws[4]) == int(ws[6]) > 0, ws          # cxy2 is empty: imp starts where it would


# ----------------------------------------------------------------------------- the driver: argument validation

SMALL = [(9, 7)]
REFUSALS = [(case("null_value", SMALL), "NULL pointer"), (case("null_energy", SMALL), "NULL pointer"), (case("null_params", SMALL), "NULL pointer"),
            (case("null_levels", SMALL), "levels is NULL"), (case("n_levels_0", [], n_levels=0), "n_levels"),
            (case("n_levels_above_max", SMALL * (MAX_LEVELS + 1)), "n_levels"), (case("n_frames_0", SMALL, n_frames=0), "n_frames"),
            (case("n_frames_negative", SMALL, n_frames=-3), "n_frames"), (case("region_h_0", SMALL, region=(0, 3)), "region extents"),
            (case("region_w_negative", SMALL, region=(3, -1)), "region extents"), (case("extent_0", SMALL + [(0, 5)]), "extent"),
            (case("extent_negative", [(5, -5)]), "extent"), (case("div_below_1", SMALL, div=0.999), "resize_div"),
            (case("div_0", SMALL, div=0.0), "resize_div"), (case("div_negative", SMALL, div=-2.0), "resize_div"),
            (case("div_nan", SMALL, div="nan"), "resize_div"), (case("div_inf", SMALL, div="inf"), "resize_div"),
            (case("half_h_0", [(9, 7), (1, 7)]), "half extent"), (case("half_w_0", [(9, 1)]), "half extent"),
            (case("half_0_at_div_10", [(9, 12)], div=10.0), "half extent"), (case("recovery_0", SMALL, mode=0), "recovery"),
            (case("recovery_4", SMALL, mode=4), "recovery")]


@needs_hipcc
def test_what_the_tail_refuses():
    out = run([l for l, _ in REFUSALS] + [case("div_1", SMALL, div=1.0), case("smallest", [(2, 2)])])
    head = [l.split(" | ") for l in out if " L" not in l.split(" | ")[0] and " plan" not in l.split(" | ")[0]]
    assert len(head) == len(REFUSALS) + 2
    for f, (line, word) in zip(head, REFUSALS):
        assert f[0] == line.split(" ")[0] and f[1] == "-1" and f[2].startswith("silent_attention_tail: ") and word in f[2], f
    assert [f[1] for f in head[-2:]] == ["0", "0"], head[-2:]          # resize_div = 1 and a 2 x 2 level (half map 1 x 1) are accepted


# ----------------------------------------------------------------------------- the driver: layouts of workload size

@needs_hipcc
def test_the_layout_holds_at_workload_size():
    """32 frames of config 3's six levels -- the largest case -- and of the reference layout, 65535 frames of 4K: the pure planning, and
    the driver's own checks of it (pieces aligned, disjoint, inside the total; 8 + 8 + 4 + 4 bytes per cell)."""
    lines = [case("config3_f32", CONFIG3, 32), case("reference_f32", REFERENCE, 32), case("4K_f65535", [(2160, 3840)], 65535)]
    out = [l.split(" | ") for l in run(lines, "--layout")]
    assert [f[1] for f in out] == ["ok"] * 3, out
    g = geometry(CONFIG3, (3, 3))
    cells = 32 * sum(r["cells"][0] * r["cells"][1] for r in g)
    cells2 = 32 * sum(r["cells2"][0] * r["cells2"][1] for r in g)
    assert out[0][2].startswith("cells %d %d " % (cells, cells2)), out[0]
    total = int(out[0][2].split(" total ")[1])
    assert 16 * cells + 8 * cells2 <= total <= 16 * cells + 8 * cells2 + 4 * 256
