"""bench.py --dump-outputs / --full.

A plain run times the steps and prints the headline only; --dump-outputs DIR saves the
last timed step's arrays as float32 .npy, the same from run to run (same arguments =
same games, same Philox actions), so two builds can be compared output for output.
--full adds the event-timed roofline pass (and, without --no-cpu-baseline, the CPU leg).
"""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_outputs_samples_envs_within_budget(tmp_path):
    """All envs when they fit; otherwise one seeded, sorted sample of envs shared by every
    array (envs.npy), the same on every call, float32 on disk, inside the byte budget."""
    import torch

    n = 50
    obs = np.arange(n * 6, dtype=np.int32).reshape(n, 2, 3)
    rew = torch.arange(n, dtype=torch.float64)
    done = np.arange(n) % 2 == 0
    out = {"obs": obs, "reward": rew, "done": done}
    bench.dump_outputs(str(tmp_path / "all"), out)
    assert np.load(tmp_path / "all" / "envs.npy").tolist() == list(range(n))
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "obs.npy"), obs.astype(np.float32))
    per_env = 4 * (6 + 1 + 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, suffix="_x", budget=7 * per_env + 5)
    idx = np.load(tmp_path / "a" / "envs_x.npy")
    assert idx.dtype == np.float64 and len(idx) == 7 and len(set(idx.tolist())) == 7 and idx.tolist() == sorted(idx.tolist())
    i = idx.astype(int)
    total = 0
    for name, v in (("obs", obs), ("reward", rew.numpy()), ("done", done)):
        a, b = np.load(tmp_path / "a" / f"{name}_x.npy"), np.load(tmp_path / "b" / f"{name}_x.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, v[i].astype(np.float32))
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 7 * per_env + 5


def test_full_is_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True


SMALL = ["--gpus", "1", "--envs-per-gpu", "64", "--steps", "6", "--warmup", "2", "--preroll", "40", "--max-steps", "40"]


def _line(capsys, argv):
    assert bench.main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_run_dumps_repeatable_outputs(tmp_path, capsys):
    """Two plain runs with the same arguments write identical float32 arrays of the last
    timed step; the line carries the headline and none of the --full measurements."""
    lines = [_line(capsys, SMALL + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for ln in lines:
        assert ln["steps"] == 6 and ln["ms_per_step"] > 0 and ln["value"] > 0 and ln["engine_error_flags"] == 0
        assert ln["value"] == pytest.approx(64 * 1e3 / ln["ms_per_step"], rel=1e-2)
        assert ln["roofline"] is None and ln["kernels"] == {} and "cpu_baseline" not in ln
        assert "box_write_ceiling" not in ln["window"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["action_mask.npy", "actions.npy", "done.npy", "envs.npy", "obs.npy", "reward.npy"]
    assert names == sorted(os.listdir(tmp_path / "b"))
    shapes = {"obs.npy": (64, 16, 16, 29), "action_mask.npy": (64, 256, 78), "actions.npy": (64, 256, 7),
              "reward.npy": (64,), "done.npy": (64,), "envs.npy": (64,)}
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == shapes[n], (n, a.dtype, a.shape)
        np.testing.assert_array_equal(a, b, err_msg=n)
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert set(np.unique(obs).tolist()) == {0.0, 1.0} and np.load(tmp_path / "a" / "action_mask.npy").any()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_full_adds_the_roofline_pass(capsys):
    ln = _line(capsys, SMALL + ["--full", "--no-cpu-baseline", "--roofline-steps", "4"])
    assert ln["roofline"]["samples"] == 4 and set(ln["kernels"]) >= {"step", "sample"}
    assert ln["window"]["box_write_ceiling"]["GBps"] > 0
