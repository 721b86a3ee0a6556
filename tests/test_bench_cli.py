"""bench.py's command line: the options a plain run and a `--full` run are driven by, and the
`--dump-outputs` writer (float32 / float64 .npy files under a size bound). No GPU needed."""
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None and a.workload == "homography"


def test_full_and_dump_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "some/dir")
    assert a.full is True and a.dump_outputs == "some/dir"
    assert not a.no_cpu_baseline and not a.no_secondary   # --full runs both legs unless told otherwise


def test_dump_outputs_writes_float_arrays(tmp_path):
    out = tmp_path / "a" / "b"
    mask = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    idx = np.array([3, 2**31 - 1, 0], dtype=np.int32)
    H = np.arange(9, dtype=np.float64).reshape(3, 3) / 7
    d32 = np.array([0.1, 0.2], dtype=np.float32)
    bench.dump_outputs(out, {"mask": mask, "idx": idx, "model": H, "dist": d32})
    got = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert sorted(got) == ["dist", "idx", "mask", "model"]
    assert got["mask"].dtype == np.float32 and np.array_equal(got["mask"], mask)
    assert got["idx"].dtype == np.float64 and np.array_equal(got["idx"], idx)   # exact: |idx| < 2^53
    assert got["model"].dtype == np.float64 and np.array_equal(got["model"], H)
    assert got["dist"].dtype == np.float32 and np.array_equal(got["dist"], d32)


def test_dump_outputs_refuses_more_than_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64)
    with pytest.raises(SystemExit):
        bench.dump_outputs(tmp_path, {"x": np.zeros(17, dtype=np.float32)})
    assert not list(tmp_path.glob("*.npy"))
