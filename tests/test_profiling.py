"""Tracing / profiling hooks: roctx ranges and the torch.profiler step wrapper."""
import os

import torch

from penroz.utils import profiling


def test_trace_range_noop_when_disabled(monkeypatch):
    monkeypatch.setattr(profiling, "ENABLED", False)
    with profiling.trace_range("x"):
        pass


def test_trace_range_with_roctx_library(monkeypatch):
    monkeypatch.setattr(profiling, "ENABLED", True)
    with profiling.trace_range("outer"):
        with profiling.trace_range("inner"):
            profiling.mark("m")
    # the ROCm image ships the roctx library; ranges must not raise either way
    assert profiling.available() in (True, False)


def test_profile_steps_writes_trace_and_table(tmp_path):
    x = torch.randn(64, 64)
    table = profiling.profile_steps(lambda: (x @ x).sum(), 2, str(tmp_path))
    assert os.path.exists(tmp_path / "trace.json")
    assert os.path.exists(tmp_path / "kernels.txt")
    assert "aten::mm" in table or "aten::matmul" in table


def test_executor_phases_are_instrumented():
    import inspect
    from penroz.models import executor, flat_executor
    src = inspect.getsource(executor) + inspect.getsource(flat_executor)  # the block loop + the shared base
    for name in ("forward", "backward.head", "backward.block", "grad_allreduce.wait", "optimizer"):
        assert name in src
