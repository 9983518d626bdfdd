"""Next-token selection (greedy / temperature / top-k / top-p / min-p) and int8 KV quantisation.

Reference semantics (``neural_net_model.py:393-405``): temperature 0 → argmax of the last
position; ``top_k`` → softmax over the top-k logits / T then multinomial; otherwise softmax
over logits / T then multinomial.  (The reference's top-k runs over every position and its
non-softmax-model path crashes — bugs 2 and 5 of SURVEY §7.4 — both fixed here.)

Nucleus and min-p (beyond the reference): with S the set the top-k stage keeps (the whole row
without top-k), ``w_i = exp((x_i - max_S x) / T)`` and ``Z = sum_S w_i``,
``top_p`` in (0, 1] keeps i iff the mass of the STRICTLY larger logits is ``< top_p * Z`` — equal
logits stay or go together, the maximum always stays (HF's ``TopPLogitsWarper`` except that HF
splits a tie at the cut by sort position) — and ``min_p`` in [0, 1) keeps i iff ``w_i >= min_p``
(HF's ``MinPLogitsWarper``; a logit bound ``x_i >= max + T ln(min_p)``).  Order: temperature,
top-k, top-p, min-p, then the draw over the renormalised kept set.  ``top_p`` 1 / None and
``min_p`` 0 / None mean no filter, and temperature 0 ignores both.

GPU: ``csrc/kernels/sampling.hip`` — temperature scale, top-k by a radix-select threshold, top-p by
the same select over fixed-point mass bins, softmax and inverse-CDF draw from one uniform per row,
all on the device (no sort, no host round trip). Three paths, chosen per call by ``plan_sample``
(``csrc/kernels/host_plan.h``; ``kernels().sample_plan(dtype, B, V, temperature, top_k, filtered)``
returns the choice):

* two-stage (``sample_part_kernel`` + ``sample_merge_kernel``): a row is split into parts of 4096
  logits, one workgroup each, and one workgroup per row merges the parts' candidates. bf16 / fp32
  rows with ``V % 8 == 0`` and ``V`` <= 256 Ki, greedy or ``top_k`` <= 64 — at every batch size by
  default (``PENROZ_SAMPLE_TWO_STAGE_MIN_ROWS`` = 1), and always where the row is too wide for
  registers;
* register-resident (``sample_reg_kernel``): one workgroup per row, the row read once into
  registers. The other ``V % 8 == 0`` rows that fit: bf16 up to 64 Ki logits (40 Ki with a top-p /
  min-p filter), fp32 up to 32 Ki — so ``top_k`` = 0 or > 64, or fewer rows than the switch above;
* streaming (``sample_kernel``): one workgroup per row, several passes over the row in memory.
  Everything else: ``V % 8 != 0``, fp16, and rows too wide for the other two.
``kv_quantize``: per-token absmax/127 int8 (``kv_cache.py:114-125``), written straight into
the preallocated cache slot.
"""
from __future__ import annotations

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels


def _check_filters(top_p: float | None, min_p: float | None) -> tuple[float, float]:
    """(top_p, min_p) as numbers, 1.0 / 0.0 when off; ValueError outside (0, 1] / [0, 1)."""
    tp = 1.0 if top_p is None else float(top_p)
    mp = 0.0 if min_p is None else float(min_p)
    if not 0.0 < tp <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if not 0.0 <= mp < 1.0:
        raise ValueError(f"min_p must be in [0, 1), got {min_p}")
    return tp, mp


def reference_sample(logits: Tensor, temperature: float, top_k: int | None, uniform: Tensor,
                     top_p: float | None = None, min_p: float | None = None) -> Tensor:
    """logits [B, V] -> token ids [B, 1] using the given uniforms [B] (inverse-CDF draw)."""
    tp, mp = _check_filters(top_p, min_p)
    lf = logits.float()
    if temperature == 0.0:
        return lf.argmax(dim=-1, keepdim=True)
    lf = lf / temperature
    if top_k is not None and top_k < lf.shape[-1]:
        vals, idx = lf.topk(top_k, dim=-1)
    else:
        vals, idx = lf.sort(dim=-1, descending=True)
    probs = torch.softmax(vals, dim=-1)
    if tp < 1.0 or mp > 0.0:
        # vals is sorted descending, so both filters keep a prefix. Mass strictly above entry j =
        # the exclusive prefix sum at the FIRST entry of j's run of equal values.
        w = torch.exp(vals - vals[:, :1])
        keep = torch.ones_like(w, dtype=torch.bool)
        if tp < 1.0:
            excl = w.cumsum(-1) - w
            first = torch.searchsorted((-vals).contiguous(), (-vals).contiguous(), right=False)
            keep &= excl.gather(1, first) < tp * w.sum(-1, keepdim=True)
        if mp > 0.0:
            keep &= w >= mp
        keep[:, 0] = True
        probs = torch.where(keep, w, torch.zeros_like(w))
    cdf = probs.cumsum(-1)
    choice = torch.searchsorted(cdf, (uniform.float() * cdf[:, -1]).unsqueeze(-1).contiguous())
    choice = choice.clamp(max=vals.shape[-1] - 1)
    return idx.gather(1, choice)


def sample(logits: Tensor, temperature: float, top_k: int | None, generator: torch.Generator | None = None,
           device_rng: bool = False, top_p: float | None = None, min_p: float | None = None) -> Tensor:
    """logits [B, V] -> [B, 1] int64 next-token ids. ``device_rng``: draw the uniforms on the
    device (required inside a captured HIP graph; the host-drawn default matches CPU runs).
    ``top_p`` / ``min_p``: nucleus and min-p filters after top-k (module docstring)."""
    B = logits.shape[0]
    tp, mp = _check_filters(top_p, min_p)
    if temperature == 0.0:
        if use_kernels(logits):
            return kernels().sample_tokens(logits.contiguous(), None, 0.0, 0)
        return logits.argmax(dim=-1, keepdim=True)
    if device_rng:
        uniform = torch.rand(B, device=logits.device)
    else:
        uniform = torch.rand(B, generator=generator, device="cpu").to(logits.device)
    if use_kernels(logits):
        k = 0 if top_k is None or top_k >= logits.shape[-1] else int(top_k)
        if tp < 1.0 or mp > 0.0:
            return kernels().sample_tokens(logits.contiguous(), uniform, float(temperature), k, tp, mp)
        return kernels().sample_tokens(logits.contiguous(), uniform, float(temperature), k)
    return reference_sample(logits, temperature, top_k, uniform, top_p, min_p)


def reference_quantize(x: Tensor) -> tuple[Tensor, Tensor]:
    """x [..., D] -> (int8 [..., D], scale [..., 1]) per-token absmax / 127."""
    abs_max = x.abs().amax(dim=-1, keepdim=True)
    scale = abs_max / 127.0
    scale = torch.where(scale == 0, torch.ones_like(scale), scale)
    q = (x / scale).round().clamp(-128, 127).to(torch.int8)
    return q, scale


def kv_quantize_into(x: Tensor, q_out: Tensor, s_out: Tensor, pos: int) -> None:
    """x [B, T, Hkv, D] -> q_out[:, :, pos:pos+T] (int8 [B,Hkv,cap,D]), s_out[:, :, pos:pos+T] (f32)."""
    if use_kernels(x):
        kernels().kv_quantize(x.contiguous(), q_out, s_out, int(pos))
        return
    T = x.shape[1]
    q, s = reference_quantize(x.float().transpose(1, 2))
    q_out[:, :, pos:pos + T] = q
    s_out[:, :, pos:pos + T] = s.squeeze(-1)


def kv_store_into(x: Tensor, out: Tensor, pos: int) -> None:
    """x [B, T, Hkv, D] -> out[:, :, pos:pos+T] (layout [B, Hkv, cap, D])."""
    out[:, :, pos:pos + x.shape[1]] = x.transpose(1, 2).to(out.dtype)
