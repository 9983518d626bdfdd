"""Gradient clipping by global L2 norm.

Definition (exactly ``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0,
error_if_nonfinite=False)``):

    norm  = sqrt(Σ over every parameter gradient element g²)
    coef  = min(1, max_norm / (norm + 1e-6))
    g_eff = g · coef

The gradients are the ones the optimizer step is about to consume: accumulated over the step's
micro-steps with their ``1/num_steps`` scale, and after the data-parallel all-reduce, so every rank
holds the same gradient and computes the same norm without a further collective. A NaN gradient
gives ``norm = coef = NaN``; an infinite one ``norm = inf, coef = 0`` (the step then produces NaN
exactly as torch's does). ``max_grad_norm`` is a finite number > 0, or None for off.

GPU: ``csrc/kernels/grad_norm.hip``. ``grad_sumsq`` writes one fp64 partial sum per chunk of 16 384
floats of the flat gradient buffer, ``grad_clip_finish`` folds them into ``(norm, coef)`` fp32 [2]
on the device, in a fixed order (bitwise reproducible, no atomics). The fused Adam kernels read the
coefficient from there (``scale_dev``), so the host never learns it and the step has no
synchronisation. On the CPU, or under the ``reference`` engine, the same formula runs in torch
fp64.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels


def check_max_grad_norm(v) -> float | None:
    """``max_grad_norm`` as a float, or None for off. ValueError unless it is None or a finite
    number > 0 (a bool is not a number here)."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"max_grad_norm must be a finite number > 0 or None, got {v!r}")
    f = float(v)
    if not (math.isfinite(f) and f > 0.0):
        raise ValueError(f"max_grad_norm must be a finite number > 0 or None, got {v!r}")
    return f


def reference_clip(grads, max_norm: float) -> tuple[Tensor, Tensor]:
    """(norm, coef) as fp64 scalars (on the gradients' device) of a tensor or a list of tensors:
    the module docstring's definition, every element squared and summed in fp64."""
    if isinstance(grads, Tensor):
        grads = [grads]
    grads = list(grads)
    dev = grads[0].device if grads else torch.device("cpu")
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for g in grads:
        total = total + g.detach().double().square().sum()
    norm = total.sqrt()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)  # (clamp keeps a NaN)
    return norm, coef


_WORKSPACE: dict = {}


def _workspace(device: torch.device, chunks: int) -> Tensor:
    """The fp64 partial sums, one buffer per (device, size): a step allocates nothing."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), chunks)
    ws = _WORKSPACE.get(key)
    if ws is None:
        ws = _WORKSPACE[key] = torch.empty(max(chunks, 1), dtype=torch.float64, device=device)
    return ws


def grad_clip_coef(flat_grad: Tensor, max_norm: float, out: Tensor | None = None) -> Tensor:
    """``out`` = (norm, coef) fp32 [2] of the flat gradient buffer, on its device; two launches on
    the current stream, no host synchronisation. GPU: fp32, contiguous, 1-d, base 16-B aligned
    (anything else is refused, not launched)."""
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=flat_grad.device)
    if use_kernels(flat_grad):
        k = kernels()
        if flat_grad.dim() != 1:
            raise ValueError(f"grad_clip_coef: the gradient must be 1-d, got {tuple(flat_grad.shape)}")
        chunks = k.grad_sumsq_chunks(flat_grad.numel())
        part = _workspace(flat_grad.device, chunks)
        k.grad_sumsq(flat_grad, part)
        k.grad_clip_finish(part, chunks, float(max_norm), out)
        return out
    norm, coef = reference_clip(flat_grad, float(max_norm))
    out.copy_(torch.stack([norm, coef]))
    return out
