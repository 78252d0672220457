"""bench.py's headline phase on the GPU at a small size: --steps sets the timed moves, and --dump-outputs
writes the last timed move's outputs, identical from run to run with the same arguments."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGV = ["--games", "64", "--size", "9", "--sims", "50", "--blocks", "1", "--steps", "3", "--warmup", "1"]


def _headline(tmp_path, name, extra=()):
    import bench
    out = str(tmp_path / name)
    args = bench.headline_only(bench.parse(ARGV + ["--dump-outputs", out] + list(extra)))
    line = bench.run_phase("selfplay", args, 0, 1, None, None)
    return line, {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_plain_headline_times_the_requested_steps_and_dumps_its_last_move(tmp_path):
    line, a = _headline(tmp_path, "a")
    assert line["steps"] == 3 and len(line["step_ms"]) == 3 and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["ms_per_step"] - 64 * 1e3 / line["value"]) < 1e-6 * line["ms_per_step"]
    assert line["unit"] == "moves/s" and line["higher_is_better"] is True and line["dtype"] == "fp16"
    # a plain run: no leg of its own for the kernels' single-stream times or the live peaks
    assert "single_stream_kernels" not in line and "achievable" not in line["roofline"]
    assert line["dumped_outputs"] == sorted(a) == ["action", "policy", "root_value", "status"]
    assert a["policy"].shape == (64, 81) and all(a[k].shape == (64,) for k in ("action", "root_value", "status"))
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    # what search() and play() return: improved policies that sum to 1, the chosen legal cell, a status code
    assert np.abs(a["policy"].sum(1) - 1).max() < 1e-9 and (a["policy"] >= 0).all()
    assert ((a["action"] >= 0) & (a["action"] < 81) & (a["action"] == np.round(a["action"]))).all()
    assert (a["policy"][np.arange(64), a["action"].astype(int)] > 0).all()
    assert np.isin(a["status"], (-1, 0, 1, 2)).all()
    # the same arguments again: the same inputs, so the same outputs, bit for bit
    _, b = _headline(tmp_path, "b")
    assert sorted(b) == sorted(a) and all(np.array_equal(a[k], b[k]) for k in a)
    # one timed move fewer ends somewhere else: the dump is the LAST timed move's
    _, c = _headline(tmp_path, "c", ["--steps", "2"])
    assert not np.array_equal(a["policy"], c["policy"])
