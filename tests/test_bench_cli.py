"""CPU tests of bench.py's command line: a plain run times the headline (sampling) leg only, --full brings back everything else,
and --dump-outputs writes bounded float32 arrays whose sampled positions are the same in every run."""
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_sampling_leg_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.mode == "sample" and not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None


def test_full_restores_every_leg(monkeypatch):
    assert _parse(monkeypatch, "--full").mode == "both"
    assert _parse(monkeypatch, "--full", "--mode", "train").mode == "train"
    assert _parse(monkeypatch, "--mode", "train").mode == "train"


def test_dump_ops_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--dump-ops", "ops.txt")
    assert _parse(monkeypatch, "--full", "--dump-ops", "ops.txt").dump_ops == "ops.txt"


def test_dump_array_small_is_whole_and_float32():
    t = torch.arange(24, dtype=torch.bfloat16).reshape(2, 3, 4)
    a = bench.dump_array(t)
    assert a.dtype == np.float32 and a.shape == (2, 3, 4) and np.array_equal(a, t.float().numpy())


def test_dump_array_large_is_a_fixed_sample():
    t = torch.randn(5000, dtype=torch.float64)
    a, b = bench.dump_array(t, cap=100), bench.dump_array(t.clone(), cap=100)
    assert a.dtype == np.float32 and a.shape == (100,) and np.array_equal(a, b)
    # the values are elements of t at sorted positions
    g = torch.Generator().manual_seed(20251016)
    idx = torch.randint(0, t.numel(), (100,), generator=g).sort().values
    assert np.array_equal(a, t[idx].float().numpy())


def test_write_outputs_and_budget(tmp_path, monkeypatch):
    arrays = {"x": np.ones((4, 4), np.float32), "loss": np.float32(0.5) * np.ones((), np.float32)}
    bench.write_outputs(str(tmp_path / "out"), arrays)
    assert np.array_equal(np.load(tmp_path / "out" / "x.npy"), arrays["x"])
    assert np.load(tmp_path / "out" / "loss.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 32)
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "big"), arrays)
