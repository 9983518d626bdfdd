"""Gradient clipping by global norm on the CPU: the check of the bound, the fp64 reference against
torch's ``clip_grad_norm_``, the generic runner's clipped step, the ``PENROZ_MAX_GRAD_NORM``
default, the ``grad_norm`` of the progress records and the ``/train/`` route."""
import math
from unittest.mock import patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel, _make_runner
from penroz.ops import grad_clip as gc
from penroz.serve import app as A

client = TestClient(main.app, raise_server_exceptions=False)
CPU = torch.device("cpu")


# ---------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("v,want", [(None, None), (1, 1.0), (0.5, 0.5), (1e9, 1e9)])
def test_check_accepts(v, want):
    got = gc.check_max_grad_norm(v)
    assert got == want and (got is None or type(got) is float)


@pytest.mark.parametrize("v", [True, 0, -1, float("nan"), float("inf"), "1"])
def test_check_refuses(v):
    with pytest.raises(ValueError, match="max_grad_norm"):
        gc.check_max_grad_norm(v)


# ---------------------------------------------------------------------------------- the reference
def _grads(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) for n in (1, 3, 17, 4096, 70001)]


@pytest.fixture(scope="module")
def grads():
    return _grads()


@pytest.mark.parametrize("max_norm", [1.0, 37.5, 1e4])
def test_reference_clip_matches_torch(grads, max_norm):
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    t_norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    norm, coef = gc.reference_clip(grads, max_norm)
    assert norm.dtype == torch.float64 and coef.dtype == torch.float64
    # torch's norm: fp32 norms per tensor, then the fp32 norm of those — a few fp32 roundings
    assert abs(t_norm.item() - norm.item()) <= 4 * 2.0 ** -24 * norm.item()
    if max_norm > norm.item():
        assert coef.item() == 1.0
    else:
        assert coef.item() < 1.0
    c32 = coef.float()
    for p, g in zip(params, grads):
        torch.testing.assert_close(g * c32, p.grad, rtol=2.0 ** -22, atol=0)
    if max_norm > norm.item():
        assert all(torch.equal(p.grad, g) for p, g in zip(params, grads))


def test_reference_clip_cases_cover_both_sides(grads):
    norm = gc.reference_clip(grads, 1.0)[0].item()
    assert 37.5 < norm < 1e4  # the parametrised bounds lie on both sides of the norm


def test_reference_clip_nonfinite():
    g = torch.ones(10)
    g[3] = float("nan")
    norm, coef = gc.reference_clip(g, 1.0)
    assert math.isnan(norm.item()) and math.isnan(coef.item())
    g[3] = float("inf")
    norm, coef = gc.reference_clip(g, 1.0)
    assert norm.item() == float("inf") and coef.item() == 0.0


@pytest.mark.parametrize("max_norm", [1.0, 1e4])
def test_cpu_grad_clip_coef_is_the_reference_rounded(grads, max_norm):
    flat = torch.cat(grads)
    out = gc.grad_clip_coef(flat, max_norm)
    norm, coef = gc.reference_clip(flat, max_norm)
    assert out.dtype == torch.float32 and out.shape == (2,)
    assert out[0].item() == norm.float().item() and out[1].item() == coef.float().item()
    buf = torch.empty(2)
    assert gc.grad_clip_coef(flat, max_norm, out=buf) is buf and torch.equal(buf, out)
    assert torch.equal(gc.grad_clip_coef(torch.empty(0), 2.0), torch.tensor([0.0, 1.0]))


# ---------------------------------------------------------------------------------- the generic runner
def _model():
    torch.manual_seed(0)
    return NeuralNetworkModel("clip", Mapper(bench.gpt2_layers(V=64, C=32, L=1, H=2, P=32), {"sgd": {"lr": 0.1}}))


def _batch():
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(0, 64, (2, 16), generator=gen)
    return x, torch.roll(x, -1, 1)


def _runner_step(max_norm):
    """One step through the runner -> (parameters, the runner)."""
    m = _model()
    runner = _make_runner(m, "generic", CPU, False, max_norm)
    x, y = _batch()
    runner.zero_grad()
    runner.micro_step(x, y, 1.0, first=True, last=True, capture=False)
    runner.step()
    return [p.detach().clone() for p in m.parameters()], runner


def _manual_step(max_norm):
    """The same backward, then torch's clip (None: none), then the optimizer -> (parameters, norm)."""
    m = _model()
    x, y = _batch()
    m.optimizer.zero_grad()
    _, loss = m(x, y, skip_softmax=True)
    loss.backward()
    norm = torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in m.parameters()])).item()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)
    m.optimizer.step()
    return [p.detach().clone() for p in m.parameters()], norm


@pytest.fixture(scope="module")
def unclipped():
    return _manual_step(None)


def test_generic_runner_clips_like_torch(unclipped, monkeypatch):
    monkeypatch.delenv("PENROZ_MAX_GRAD_NORM", raising=False)
    plain, norm = unclipped
    m = 0.5 * norm
    got, runner = _runner_step(m)
    want, _ = _manual_step(m)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert any(not torch.equal(a, b) for a, b in zip(got, plain))
    assert runner.grad_norm().item() == pytest.approx(norm, rel=1e-6)
    # a bound far above the norm: coef == 1.0, the unclipped step's bits
    got, runner = _runner_step(1e9)
    assert all(torch.equal(a, b) for a, b in zip(got, plain))
    # off: the unclipped step, and no norm
    got, runner = _runner_step(None)
    assert all(torch.equal(a, b) for a, b in zip(got, plain)) and runner.grad_norm() is None


def test_env_default(unclipped, monkeypatch):
    plain, norm = unclipped
    assert norm > 0.5  # the bound below clips
    monkeypatch.setenv("PENROZ_MAX_GRAD_NORM", "0.5")
    got, runner = _runner_step(None)
    want, _ = _manual_step(0.5)
    assert runner.max_grad_norm == 0.5
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    got, runner = _runner_step(0.25 * norm)  # the argument wins
    assert runner.max_grad_norm == 0.25 * norm
    monkeypatch.setenv("PENROZ_MAX_GRAD_NORM", "")
    assert _make_runner(_model(), "generic", CPU, False).max_grad_norm is None
    for bad in ("abc", "0", "-1", "nan", "inf"):
        monkeypatch.setenv("PENROZ_MAX_GRAD_NORM", bad)
        with pytest.raises(ValueError):
            _make_runner(_model(), "generic", CPU, False)


def test_invalid_argument_is_refused(monkeypatch):
    monkeypatch.delenv("PENROZ_MAX_GRAD_NORM", raising=False)
    for bad in (True, 0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _make_runner(_model(), "generic", CPU, False, bad)


# ---------------------------------------------------------------------------------- progress records
@pytest.fixture
def sandbox(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data").mkdir()
    (tmp_path / "shm").mkdir()
    monkeypatch.setenv("PENROZ_DATA_FOLDER", str(tmp_path / "data"))
    monkeypatch.setenv("PENROZ_SHM_PATH", str(tmp_path / "shm"))
    monkeypatch.delenv("PENROZ_MAX_GRAD_NORM", raising=False)
    import penroz.utils.loaders as loaders
    monkeypatch.setattr(loaders, "DATA_FOLDER", str(tmp_path / "data"))
    monkeypatch.setattr(NeuralNetworkModel, "SHM_PATH", str(tmp_path / "shm"))
    return tmp_path


def _train(model_id, **kw):
    from penroz.utils import loaders
    torch.manual_seed(0)
    m = NeuralNetworkModel(model_id, Mapper(bench.gpt2_layers(V=64, C=32, L=2, H=2, P=32),
                                            {"adamw": {"lr": 3e-3, "betas": [0.9, 0.95]}}))
    loaders.synthetic_shards("ds", 1, 4096, 64)
    m.train_model("ds", 0, 3, 4, 16, 2, **kw)
    return m


def test_progress_records_carry_grad_norm(sandbox):
    m = _train("clipped", max_grad_norm=1.0)
    assert len(m.progress) == 3
    for rec in m.progress:
        assert math.isfinite(rec["grad_norm"]) and rec["grad_norm"] > 0 and isinstance(rec["grad_norm"], float)
    assert not hasattr(m, "max_grad_norm")  # it belongs to the call
    m = _train("plain")
    assert len(m.progress) == 3 and all("grad_norm" not in rec for rec in m.progress)
    with pytest.raises(ValueError):
        _train("bad", max_grad_norm=-1)


# ---------------------------------------------------------------------------------- /train/
BODY = {"model_id": "gc", "device": "cpu", "dataset_id": "d", "shard": 0, "epochs": 1, "batch_size": 2,
        "block_size": 8, "step_size": 1}


@pytest.fixture
def ran_tasks():
    """``/train/`` with the launcher mocked; the launch coroutine the route hands to ``create_task``
    runs to its end (on a loop of its own: the route's is busy answering) before the route returns."""
    import asyncio
    import threading

    def run(coro):
        t = threading.Thread(target=asyncio.run, args=(coro,))
        t.start()
        t.join()
    with patch.object(A.launcher, "launch_single_node_ddp", return_value=0) as launch, \
            patch.object(A, "_evict"), patch.object(A, "create_task", side_effect=run) as ct:
        launch.create_task = ct
        yield launch


@pytest.mark.parametrize("bad", [-1, 0, True])
def test_train_route_refuses_invalid_bound(ran_tasks, bad):
    r = client.put("/train/", json={**BODY, "max_grad_norm": bad})
    assert r.status_code == 400 and "max_grad_norm" in r.json()["detail"]
    ran_tasks.create_task.assert_not_called()
    ran_tasks.assert_not_called()


def _launched_args(launch, body):
    r = client.put("/train/", json=body)
    assert r.status_code == 202
    launch.assert_called_once()
    args = launch.call_args[0]
    assert args[:3] == ("gc", "cpu", NeuralNetworkModel.train_model_on_device)
    return args[3:]


def test_train_route_passes_bound_last(ran_tasks):
    args = _launched_args(ran_tasks, {**BODY, "max_grad_norm": 2.0})
    assert args == ("gc", "cpu", "d", 0, 1, 2, 8, 1, 2.0) and type(args[-1]) is float


def test_train_route_without_bound_passes_todays_arguments(ran_tasks):
    assert _launched_args(ran_tasks, BODY) == ("gc", "cpu", "d", 0, 1, 2, 8, 1)
    ran_tasks.reset_mock()
    assert _launched_args(ran_tasks, {**BODY, "max_grad_norm": None}) == ("gc", "cpu", "d", 0, 1, 2, 8, 1)


def test_run_training_job_arguments():
    with patch.object(A.launcher, "launch_single_node_ddp", return_value=0) as launch, patch.object(A, "_evict"):
        A.run_training_job("m", "cpu", "d", 0, 1, 2, 8, 1)
        assert launch.call_args[0][3:] == ("m", "cpu", "d", 0, 1, 2, 8, 1)
        A.run_training_job("m", "cpu", "d", 0, 1, 2, 8, 1, max_grad_norm=0.5)
        assert launch.call_args[0][3:] == ("m", "cpu", "d", 0, 1, 2, 8, 1, 0.5)


def test_evaluate_does_not_know_the_bound():
    assert "max_grad_norm" in A.TrainingRequest.model_fields
    assert "max_grad_norm" not in A.EvaluateRequest.model_fields
