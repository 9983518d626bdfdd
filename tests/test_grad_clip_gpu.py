"""Gradient clipping by global norm on the MI355X: the two kernels of ``grad_norm.hip`` against the
fp64 formula, the flat Adam kernels' device-side gradient scale, the clipped optimizer schedule of
both fused executors, two data-parallel ranks, and the clipped loss curve against the reference
engine.

Bound of the kernel checks: ``norm`` and ``coef`` within 2⁻²³ relative of the fp64 formula on the
same data. Any-order fp64 summation of n ≤ 2²³ exact non-negative terms errs by at most
n·2⁻⁵³ ≈ 1e-9 relative, far below the single final rounding to fp32 (2⁻²⁴); 2⁻²³ leaves room for
``sqrt`` and the division. The inputs mix magnitudes 1e-30 … 3e19, on which an fp32 accumulation
under- or overflows: ``test_inputs_tell_fp32_accumulation_from_fp64`` shows that it misses the
bound, so the inputs separate right from wrong.
"""
import math
import os
import socket
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import torch.distributed as dist
import torch.multiprocessing as mp

import adam_reference as A
import bench
from adam_reference import HYPER_SETS, make_inputs
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel, _make_runner
from penroz.ops import _ext, fused as Fu, grad_clip as gc

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
REL = 2.0 ** -23
CHUNK = 16384
SIZES = [0, 1, 3, 4, 5, 1023, CHUNK, CHUNK + 1, 262147, 256 * CHUNK + 5]
MAGNITUDES = (1e-30, 1e-3, 1.0, 3e19)


def _data(n: int) -> torch.Tensor:
    """Seeded normal values, each times a magnitude drawn from MAGNITUDES (fp32, CPU)."""
    gen = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(n, generator=gen)
    which = torch.randint(0, len(MAGNITUDES), (n,), generator=gen)
    return x * torch.tensor(MAGNITUDES, dtype=torch.float32)[which]


_DATA: dict = {}


def _case(n: int):
    """(data on the CPU, fp64 norm, fp64 coef for max_norm = 1), computed once per size."""
    if n not in _DATA:
        x = _data(n)
        norm, coef = gc.reference_clip(x, 1.0)
        _DATA[n] = (x, norm.item(), coef.item())
    return _DATA[n]


def _within(got: float, want: float) -> bool:
    return got == want or abs(got - want) <= REL * abs(want)


# ---------------------------------------------------------------------------------- kernels
def test_extension_has_the_kernels():
    k = _ext.kernels()
    assert k.grad_sumsq_chunks(0) == 0 and k.grad_sumsq_chunks(CHUNK) == 1 and k.grad_sumsq_chunks(CHUNK + 1) == 2


@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coef_match_fp64(n):
    x, norm, coef = _case(n)
    out = gc.grad_clip_coef(x.to(DEV), 1.0)
    torch.cuda.synchronize()
    got_norm, got_coef = out.double().tolist()
    print(f"n={n}: norm {got_norm!r} vs {norm!r} (rel {abs(got_norm - norm) / norm if norm else 0.0:.3g}), "
          f"coef {got_coef!r} vs {coef!r} (rel {abs(got_coef - coef) / coef:.3g})")
    assert out.dtype == torch.float32 and out.shape == (2,)
    assert _within(got_norm, norm), (got_norm, norm)
    assert _within(got_coef, coef), (got_coef, coef)
    if n == 0:
        assert (got_norm, got_coef) == (0.0, 1.0)


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 1023])
def test_inputs_tell_fp32_accumulation_from_fp64(n):
    """(CPU) The same sum accumulated in fp32 misses the bound on these inputs (from 1023 elements
    on every magnitude occurs): the squares of the 3e19 values overflow."""
    x, norm, coef = _case(n)
    bad_norm = (x * x).sum(dtype=torch.float32).sqrt().item()
    assert not _within(bad_norm, norm)
    small = x[x.abs() < 1e-20]  # and those of the 1e-30 values underflow to nothing
    assert small.numel() and (small * small).sum(dtype=torch.float32).item() == 0.0
    assert gc.reference_clip(small, 1.0)[0].item() > 0.0


@pytest.mark.parametrize("n", [5, CHUNK + 1, 256 * CHUNK + 5])
def test_runs_are_bitwise_equal_and_any_bound_works(n):
    x, norm, _ = _case(n)
    xd = x.to(DEV)
    a = gc.grad_clip_coef(xd, 1.0).clone()
    b = gc.grad_clip_coef(xd, 1.0, out=torch.empty(2, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for max_norm in (0.5 * norm, 2.0 * norm + 1.0):
        out = gc.grad_clip_coef(xd, max_norm).double().tolist()
        want = gc.reference_clip(x, max_norm)[1].item()
        assert _within(out[1], want), (max_norm, out, want)
    assert gc.grad_clip_coef(xd, 2.0 * norm + 1.0)[1].item() == 1.0


@pytest.mark.parametrize("n", [3, 1023, 262147])
def test_nonfinite_gradients(n):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    i = int(torch.randint(0, n, (1,), generator=gen))
    x[i] = float("nan")
    norm, coef = gc.grad_clip_coef(x.to(DEV), 1.0).tolist()
    assert math.isnan(norm) and math.isnan(coef)
    x[i] = float("inf")
    assert gc.grad_clip_coef(x.to(DEV), 1.0).tolist() == [float("inf"), 0.0]
    x[i] = float("-inf")
    assert gc.grad_clip_coef(x.to(DEV), 1.0).tolist() == [float("inf"), 0.0]


def test_misaligned_and_bf16_are_refused():
    x = torch.randn(1025, device=DEV)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        gc.grad_clip_coef(x[1:], 1.0)
    with pytest.raises(RuntimeError, match="fp32"):
        gc.grad_clip_coef(x.to(BF), 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        gc.grad_clip_coef(x[::2], 1.0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- Adam with scale_dev
def _args(h):
    return (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], h["grad_scale"], h["maximize"])


COEF = 0.37


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
@pytest.mark.parametrize("si", range(len(HYPER_SETS)))
@pytest.mark.parametrize("n", [1, 5, 1023, 262147])
def test_flat_step_with_device_scale(n, si, decoupled):
    h = HYPER_SETS[si]
    fn = Fu.adamw_step if decoupled else Fu.adam_step
    inputs = make_inputs(n, h["step"])
    scale_dev = torch.tensor([COEF], dtype=torch.float32, device=DEV)

    def run(sd, hyper=h):
        p, g, m, v = (t.to(DEV).clone() for t in inputs)
        sh = torch.full((n,), 13.0, dtype=BF, device=DEV)
        fn(p, g, m, v, sh, *_args(hyper), scale_dev=sd)
        torch.cuda.synchronize()
        return p, m, v, sh, g

    p, m, v, sh, g = run(scale_dev)
    # the reference's scale: grad_scale · coef, coef being the number the device tensor holds
    h_eff = dict(h, grad_scale=h["grad_scale"] * scale_dev.double().item())
    ref, sc = A.scales(*inputs, h_eff, decoupled)
    A.assert_within((p, m, v), ref, sc, A.k_for(h_eff, decoupled, inputs), f"scale_dev n={n} set {si}")
    assert torch.equal(sh, p.to(BF)), "shadow != the kernel's own p rounded to bf16"
    assert torch.equal(g.cpu(), inputs[1]), "the flat step must not write the gradient"
    # 1.0 on the device: the bits of the step without a device scale
    base = run(None)
    one = run(torch.ones(1, dtype=torch.float32, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(base, one))
    # the scale is read when the kernel runs: the same call after fill_(0.5), nothing new from the
    # host, gives the step at half the gradient scale (a power of two: bitwise the host-scaled step)
    scale_dev.fill_(0.5)
    half = run(scale_dev)
    want = run(None, dict(h, grad_scale=h["grad_scale"] * 0.5))
    assert all(torch.equal(a, b) for a, b in zip(half, want))
    assert not torch.equal(half[1], m)


def test_non_flat_paths_refuse_a_device_scale():
    from penroz.models.optim import FusedAdamW
    p = torch.nn.Parameter(torch.randn(8, device=DEV))
    p.grad = torch.randn(8, device=DEV)
    opt = FusedAdamW([p], lr=1e-3)
    with pytest.raises(RuntimeError, match="scale_dev"):
        opt.step(scale_dev=torch.ones(1, device=DEV))
    with pytest.raises(RuntimeError, match="scale_dev"):
        Fu.adamw_step(p.data, p.grad, torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), None,
                      1e-3, 0.9, 0.999, 1e-8, 0.01, 1, scale_dev=torch.ones(2, device=DEV))


# ---------------------------------------------------------------------------------- executors
def _executor(kind: str):
    torch.manual_seed(11)
    if kind == "gpt":
        from penroz.models.executor import GPTExecutor as Ex
        layers, V, shape = bench.gpt2_layers(V=512, C=128, L=2, H=2, P=128), 512, (4, 128)
    else:
        from penroz.models.gemma_executor import GemmaExecutor as Ex
        layers, V, shape = bench.gemma3_1b_layers(2), 262144, (2, 128)
    model = NeuralNetworkModel("clip_" + kind, Mapper(layers, {"adamw": {"lr": 1e-3, "betas": [0.9, 0.95]}}))
    model.to(DEV)
    ex = Ex(model, DEV)
    ex.setup_training(False)
    gen = torch.Generator().manual_seed(5)
    batches = []
    for _ in range(2):
        b = torch.randint(0, V, (shape[0], shape[1] + 1), generator=gen)
        batches.append((b[:, :-1].contiguous().to(DEV), b[:, 1:].contiguous().to(DEV)))
    return model, ex, batches


def _backward(ex, batches, micro: int, fuse: bool):
    ex.zero_grad()
    for i in range(micro):
        x, y = batches[i]
        ex.train_micro_step(x, y, 1.0 / micro, sync=i == micro - 1, fuse_optimizer=fuse and i == micro - 1)


def _sample(n: int) -> torch.Tensor | None:
    """Element indices for the fp64 comparison of a large flat buffer (None: all of it). The step is
    elementwise once the coefficient is known, so a sample checks each element it holds exactly; the
    bitwise checks below cover every element."""
    if n <= 4_000_000:
        return None
    gen = torch.Generator().manual_seed(9)
    edge = torch.cat([torch.arange(0, 65536), torch.arange(n - 65536, n)])
    return torch.cat([edge, torch.randint(0, n, (2_000_000,), generator=gen)])


@pytest.mark.parametrize("kind,micro", [("gpt", 1), ("gpt", 2), ("gemma", 1)])
def test_executor_clipped_step(kind, micro):
    model, ex, batches = _executor(kind)
    opt = model.optimizer
    _backward(ex, batches, micro, fuse=False)  # a probing backward: the bound is half its norm
    bound = 0.5 * ex.flat_grad.double().norm().item()
    assert bound > 0
    ex.set_grad_clip(bound)
    _backward(ex, batches, micro, fuse=True)
    assert ex.opt_overlap_mode() == "after-backward-clipped"
    assert not ex._opt_done and all(float(opt.state[p]["step"]) == 0 for p in opt._flat["params"])
    f = opt._flat
    p0, g0, m0, v0 = (t.clone() for t in (ex.flat, ex.flat_grad, f["m"], f["v"]))
    ex.optimizer_step()
    torch.cuda.synchronize()
    # (norm, coef) against fp64 on the cloned gradient
    norm, coef = (t.item() for t in gc.reference_clip(g0, bound))
    got_norm, got_coef = ex.last_grad_norm.double().item(), ex.last_clip_coef.double().item()
    print(f"{kind} x{micro}: norm {got_norm!r} vs {norm!r}, coef {got_coef!r} vs {coef!r}")
    assert ex.last_grad_norm.is_cuda and ex.last_clip_coef.is_cuda
    assert _within(got_norm, norm) and _within(got_coef, coef) and 0.4 < got_coef < 0.6
    # the step against fp64 on the clones with that coefficient
    g = opt.param_groups[0]
    h = dict(lr=g["lr"], b1=g["betas"][0], b2=g["betas"][1], eps=g["eps"], wd=g["weight_decay"], step=1,
             grad_scale=got_coef, maximize=False)
    idx = _sample(p0.numel())
    pick = (lambda t: t.cpu()) if idx is None else (lambda t: t[idx.to(DEV)].cpu())
    inputs = tuple(pick(t) for t in (p0, g0, m0, v0))
    ref, sc = A.scales(*inputs, h, True)
    A.assert_within(tuple(pick(t) for t in (ex.flat, f["m"], f["v"])), ref, sc, A.k_for(h, True, inputs),
                    f"{kind} x{micro} clipped step")
    assert all(float(opt.state[p]["step"]) == 1 for p in f["params"])
    assert torch.equal(ex.shadow, ex.flat.to(BF)), "shadow != bf16(flat)"
    assert torch.equal(ex.flat_grad.view(torch.int32), g0.view(torch.int32)), "the clipped step wrote the gradient"
    assert not torch.equal(ex.flat, p0)


@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_executor_bound_above_the_norm_is_the_plain_step(kind):
    model, ex, batches = _executor(kind)
    opt = model.optimizer
    ex.set_grad_clip(1e9)
    _backward(ex, batches, 1, fuse=True)
    assert ex.opt_overlap_mode() == "after-backward-clipped" and not ex._opt_done
    f = opt._flat
    p0, g0, m0, v0 = (t.clone() for t in (ex.flat, ex.flat_grad, f["m"], f["v"]))
    ex.optimizer_step()
    g = opt.param_groups[0]
    Fu.adamw_step(p0, g0, m0, v0, None, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], 1)
    torch.cuda.synchronize()
    assert ex.last_clip_coef.item() == 1.0
    assert torch.equal(ex.flat, p0) and torch.equal(f["m"], m0) and torch.equal(f["v"], v0)
    # off again: the executor's own schedule is back
    ex.set_grad_clip(None)
    assert ex.last_grad_norm is None and ex.opt_overlap_mode() != "after-backward-clipped"
    _backward(ex, batches, 1, fuse=True)
    assert ex._opt_done and ex.opt_overlap_mode() == "per-segment-in-backward"
    ex.optimizer_step()
    torch.cuda.synchronize()


def test_clipped_step_adds_no_host_synchronisation():
    def sync_warnings(bound):
        model, ex, batches = _executor("gpt")
        ex.set_grad_clip(bound)
        _backward(ex, batches, 1, fuse=False)
        _backward(ex, batches, 1, fuse=False)
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                ex.optimizer_step()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return sorted({str(w.message) for w in rec})
    plain, clipped = sync_warnings(None), sync_warnings(1.0)
    assert set(clipped) <= set(plain), [w for w in clipped if w not in plain]


# ---------------------------------------------------------------------------------- progress records
def test_fused_training_records_grad_norm(tmp_path, monkeypatch):
    """train_model on the fused engine: the norm reaches the progress records through the pinned
    copy that is read one epoch later."""
    from penroz.utils import loaders
    monkeypatch.chdir(tmp_path)
    (tmp_path / "data").mkdir()
    (tmp_path / "shm").mkdir()
    monkeypatch.setattr(loaders, "DATA_FOLDER", str(tmp_path / "data"))
    monkeypatch.setattr(NeuralNetworkModel, "SHM_PATH", str(tmp_path / "shm"))
    monkeypatch.delenv("PENROZ_MAX_GRAD_NORM", raising=False)
    monkeypatch.delenv("PENROZ_ENGINE", raising=False)
    loaders.synthetic_shards("ds", 1, 16384, 512)
    torch.manual_seed(0)
    m = NeuralNetworkModel("rec", Mapper(bench.gpt2_layers(V=512, C=128, L=2, H=2, P=128),
                                         {"adamw": {"lr": 1e-3, "betas": [0.9, 0.95]}}))
    m.to(DEV)
    assert m._engine(DEV) == "fused"
    m.train_model("ds", 0, 3, 4, 128, 2, max_grad_norm=0.25)
    assert len(m.progress) == 3
    norms = [rec["grad_norm"] for rec in m.progress]
    assert all(isinstance(v, float) and math.isfinite(v) and v > 0.25 for v in norms), norms
    assert m._executor.opt_overlap_mode() == "after-backward-clipped"
    m.train_model("ds", 0, 2, 4, 128, 2)
    assert len(m.progress) == 2 and all("grad_norm" not in rec for rec in m.progress)
    assert m._executor.opt_overlap_mode() != "after-backward-clipped"


# ---------------------------------------------------------------------------------- two ranks, one GPU
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_model():
    torch.manual_seed(123)
    m = NeuralNetworkModel("clip_ddp", Mapper(bench.gpt2_layers(V=512, C=128, L=2, H=2, P=128),
                                              {"adamw": {"lr": 1e-3, "betas": [0.9, 0.95]}}))
    m.to(DEV)
    return m


def _ddp_batch(rank):
    g = torch.Generator().manual_seed(1000 + rank)
    b = torch.randint(0, 512, (4, 129), generator=g)
    return b[:, :-1].contiguous(), b[:, 1:].contiguous()


def _ddp_worker(rank, world, port, out, bucket_mb, bound):
    # the per-bucket optimizer inside the backward is forced on: clipping must still hold it back
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", PENROZ_BUCKET_MB=str(bucket_mb), PENROZ_OVERLAP_OPT="1",
                      PENROZ_OPT_PER_BUCKET="1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import penroz.parallel.reducer as R
    R.DEFAULT_BUCKET_MB = R.GLOO_BUCKET_MB = bucket_mb  # several buckets for this small model
    from penroz.models.executor import GPTExecutor
    model = _ddp_model()
    ex = GPTExecutor(model, DEV)
    ex.set_grad_clip(bound)
    ex.setup_training(True)
    assert ex.reducer is not None and len(ex.reducer.buckets) > 1
    x, y = _ddp_batch(rank)
    ex.zero_grad()
    ex.train_micro_step(x.to(DEV), y.to(DEV), 1.0, sync=True, fuse_optimizer=True)
    assert ex.opt_overlap_mode() == "after-backward-clipped" and not ex._opt_done
    ex.optimizer_step()
    torch.cuda.synchronize()
    torch.save({"norm": ex.last_grad_norm.cpu(), "coef": ex.last_clip_coef.cpu(), "flat": ex.flat.cpu()},
               f"{out}/rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_like_one_process(tmp_path):
    from penroz.models.executor import GPTExecutor
    model = _ddp_model()
    ex = GPTExecutor(model, DEV)
    ex.setup_training(False)
    (x0, y0), (x1, y1) = _ddp_batch(0), _ddp_batch(1)
    x, y = torch.cat([x0, x1]).to(DEV), torch.cat([y0, y1]).to(DEV)
    ex.zero_grad()
    ex.train_micro_step(x, y, 1.0, sync=True)
    bound = 0.5 * ex.flat_grad.double().norm().item()
    ex.set_grad_clip(bound)
    ex.zero_grad()
    ex.train_micro_step(x, y, 1.0, sync=True, fuse_optimizer=True)
    ex.optimizer_step()
    torch.cuda.synchronize()
    ref_norm, ref_coef, ref_p = ex.last_grad_norm.item(), ex.last_clip_coef.item(), ex.flat.cpu()
    mp.spawn(_ddp_worker, args=(2, _port(), str(tmp_path), 0.05, bound), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for key in ("norm", "coef", "flat"):
        assert torch.equal(r0[key], r1[key]), f"ranks disagree on {key}"
    assert abs(r0["norm"].item() - ref_norm) < 1e-3 * ref_norm, (r0["norm"].item(), ref_norm)
    assert 0.4 < r0["coef"].item() < 0.6 and 0.4 < ref_coef < 0.6
    diff = (r0["flat"] - ref_p).abs()
    assert diff.max() <= 2.1e-3 and (diff > 1e-5).float().mean() < 1e-3, (diff.max(), (diff > 1e-5).float().mean())


# ---------------------------------------------------------------------------------- loss curve
def _curve(engine, steps, data):
    torch.manual_seed(0)
    m = NeuralNetworkModel("p", Mapper(bench.gpt2_layers(V=50304, C=384, L=6, H=6, P=256),
                                       {"adamw": {"lr": 6e-4, "betas": [0.9, 0.95], "eps": 1e-8}})).cuda()
    try:
        runner = _make_runner(m, engine, DEV, False, 1.0)
        m.train()
        losses, norms = [], []
        for i in range(steps):
            x, y = data[i % len(data)]
            runner.zero_grad()
            losses.append(runner.micro_step(x, y, 1.0, True, True, False))
            runner.step()
            norms.append(runner.grad_norm().detach().clone())
        return [float(v) for v in losses], [float(v) for v in norms]
    finally:
        _ext.FORCE_TORCH = False


def test_clipped_loss_curve_matches_reference_engine():
    g = torch.Generator(device="cuda").manual_seed(2)
    base = torch.randint(0, 2000, (4, 257), device="cuda", generator=g)  # a small, learnable corpus
    data = [(base[:, :-1].contiguous(), base[:, 1:].contiguous())]
    fused, fused_norms = _curve("fused", 40, data)
    eager, eager_norms = _curve("reference", 40, data)
    print("loss every 5 steps  fused:", [round(v, 3) for v in fused[::5]], " reference:", [round(v, 3) for v in eager[::5]])
    print("norm every 5 steps  fused:", [round(v, 3) for v in fused_norms[::5]], " reference:",
          [round(v, 3) for v in eager_norms[::5]])
    for i in range(0, 40, 5):
        assert abs(fused[i] - eager[i]) < 0.05 * max(1.0, eager[i]) + 0.05, (i, fused[i], eager[i])
    assert fused[-1] < fused[0] - 1.0 and eager[-1] < eager[0] - 1.0  # both actually train
    assert max(fused_norms) > 1.0  # the bound was in force
