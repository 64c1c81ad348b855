"""bench.py's own contract: a plain run prints the headline alone, ``--steps`` sets the timed steps, ``--dump-outputs`` writes what
the last timed step computed (seeded samples of the maps), and those files are what LineEndPipeline computes on the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "ingest", "latency", "steady_state", "other_workloads", "cpu_baseline", "summary")


class _Outputs(object):
    def __init__(self, res):
        self.res = res

    def outputs(self):
        return self.res


def test_dump_outputs_writes_seeded_samples(tmp_path):
    """Maps larger than DUMP_MAP_ELEMENTS go out as the same seeded sample every time, smaller ones whole; keypoint rows and
    counts as float64; nothing beyond 64 MB."""
    import torch
    from pysilent_amd._runtime import PackedPyramid
    big_n = bench.DUMP_MAP_ELEMENTS + 4321
    big = torch.arange(big_n, dtype=torch.float32) * 0.5
    small = torch.arange(2 * 6 * 5 * 3, dtype=torch.float32) - 7.0
    rows = [np.arange(40, dtype=np.int64).reshape(10, 4), np.zeros((0, 4), np.int64), np.arange(8, dtype=np.int64).reshape(2, 4) + 1000]
    res = {"pyramid": PackedPyramid(big, [(big_n, 1)], 1, 1), "cs": PackedPyramid(small, [(6, 5)], 3, 2),
           "keypoints": rows, "keypoint_counts": np.array([10, 0, 2], np.int64)}
    written = bench.dump_outputs(torch, _Outputs(res), str(tmp_path / "a"))
    bench.dump_outputs(torch, _Outputs(res), str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "a")) == ["cs.npy", "keypoint_counts.npy", "keypoints.npy", "pyramid.npy"]
    total = 0
    for name in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 64 << 20
    pyr = np.load(tmp_path / "a" / "pyramid.npy")
    pos = np.unique(np.random.default_rng(0).integers(0, big_n, bench.DUMP_MAP_ELEMENTS))
    assert pyr.dtype == np.float32 and 0 < pyr.size <= bench.DUMP_MAP_ELEMENTS
    np.testing.assert_array_equal(pyr, pos * 0.5)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "cs.npy"), small.numpy())
    kp = np.load(tmp_path / "a" / "keypoints.npy")
    assert kp.dtype == np.float64
    np.testing.assert_array_equal(kp, np.concatenate(rows).astype(np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "keypoint_counts.npy"), [10.0, 0.0, 2.0])
    assert written == {"pyramid": [pyr.size, big_n], "cs": [small.numel(), small.numel()], "keypoints": [48, 48],
                       "keypoint_counts": [3, 3]}


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("workload,frames", [("config2", 2), ("config3", 1)])
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path, workload, frames):
    """A plain run: K timed steps, the headline keys, none of what --full adds; the dumped files equal a LineEndPipeline of the
    same workload stepped once on the same seeded frames, sampled at the same positions (tuning moves buffers, never results)."""
    import torch
    from pysilent_amd import distributed as D
    out_dir = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", workload, "--frames", str(frames), "--dump-outputs", out_dir],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip())
    assert set(HEADLINE) <= set(line) and not set(FULL_ONLY) & set(line)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert len(p.stdout) < 8192

    wl = bench.WORKLOADS[workload]
    consts = D.broadcast_constants(wl["mode"], wl["n_orient"], device=0)
    pipe = bench.make_pipeline(wl, frames, 0, consts)
    dev = torch.device("cuda", 0)
    pipe.step(bench.make_frames(torch, D, wl, frames, 0, 1, dev))
    want = pipe.outputs()
    assert sorted(os.listdir(out_dir)) == sorted(k + ".npy" for k in want)
    assert line["dump_outputs"]["values_written_of_total"].keys() == want.keys()
    for name, v in want.items():
        got = np.load(os.path.join(out_dir, name + ".npy"))
        if name == "keypoints":
            exp = np.concatenate(v).astype(np.float64)
            pos = bench._sample_positions(len(exp), bench.DUMP_KEYPOINT_ROWS)
            exp = exp if pos is None else exp[pos]
        elif name == "keypoint_counts":
            exp = v.astype(np.float64)
        else:
            exp = v.data.cpu().numpy()
            pos = bench._sample_positions(exp.size, bench.DUMP_MAP_ELEMENTS)
            exp = exp if pos is None else exp[pos]
        assert got.dtype == exp.dtype and got.shape == exp.shape, name
        np.testing.assert_array_equal(got, exp, err_msg=name)
