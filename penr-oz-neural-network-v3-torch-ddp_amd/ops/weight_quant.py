"""Weight-only int8 quantisation for the batch 1-4 decode GEMVs (csrc/kernels/decode_gemv_q8.hip).

Symmetric, one fp32 scale per output row: ``scale[n] = absmax(w[n]) / 127``, ``q = round(w / scale)``
in [-127, 127]. The quantiser is plain torch and runs once per weight version (the copies are cached
on their modules, keyed on the source weights' identity and version); the decode step reads ``q`` and
``scale`` in place of the bf16 weight, half the bytes per token. ``linear_q8_reference`` and its two
compositions are the CPU implementation and the oracle of the GPU kernels: they see the same
quantised operand, so they differ from the kernels by rounding order only.
"""
from __future__ import annotations

import os

import torch
from torch import Tensor

MODES = ("int8",)
_ROWS_PER_PASS = 4096  # the quotient is taken in fp64, a slab of rows at a time


def resolve(weight_quant: str | None) -> str | None:
    """The decode weight format a generate call asks for: ``"int8"`` or None (bf16). ``None`` is the
    process default ``PENROZ_DECODE_WEIGHTS`` ("" or "int8"), ``""`` is bf16 whatever the default.
    Anything else raises ValueError."""
    if weight_quant is None:
        weight_quant = os.environ.get("PENROZ_DECODE_WEIGHTS", "")
        what = "PENROZ_DECODE_WEIGHTS"
    else:
        what = "weight_quant"
    if weight_quant == "":
        return None
    if weight_quant not in MODES:
        raise ValueError(f"{what} must be one of {MODES} (or empty for bf16 weights), got {weight_quant!r}")
    return weight_quant


@torch.no_grad()
def quantize_rows_int8(w: Tensor) -> tuple[Tensor, Tensor]:
    """(q int8 [N, K] contiguous, scale fp32 [N]) of a float weight [N, K]. An all-zero row gets scale
    1 and q = 0. The quotient w / scale is taken in fp64, so ``|w - q·scale| <= scale / 2`` holds up to
    fp64 rounding (an fp32 quotient near 127 is off by up to 2^-18 of a step, enough to round a
    near-tie the wrong way)."""
    assert w.dim() == 2 and w.is_floating_point(), "float weight [N, K]"
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.empty(wf.shape, dtype=torch.int8, device=wf.device)
    for r0 in range(0, wf.shape[0], _ROWS_PER_PASS):
        r1 = min(wf.shape[0], r0 + _ROWS_PER_PASS)
        t = wf[r0:r1].double() / scale[r0:r1].double().unsqueeze(1)
        q[r0:r1] = t.round_().clamp_(-127, 127).to(torch.int8)
    return q, scale


def dequantize_rows(q: Tensor, scale: Tensor) -> Tensor:
    """fp32 [N, K]: q · scale per row."""
    return q.float() * scale.float().unsqueeze(1)


def _gelu(y: Tensor, act: int) -> Tensor:
    if act == 0:
        return y
    return torch.nn.functional.gelu(y, approximate="none" if act == 1 else "tanh")


def linear_q8_reference(x: Tensor, q: Tensor, scale: Tensor, bias: Tensor | None = None, act: int = 0) -> Tensor:
    """act(x · (q·scale)ᵀ + bias) in fp32; act 0 none, 1 GELU (erf), 2 GELU (tanh)."""
    y = x.float() @ dequantize_rows(q, scale).t()
    if bias is not None:
        y = y + bias.float()
    return _gelu(y, act)


def gated_q8_reference(x: Tensor, q: Tensor, scale: Tensor, kind: int) -> Tensor:
    """act(x·Wgᵀ) ⊙ (x·Wuᵀ) of a packed [gate; up] operand [2I, K] in fp32; kind 0 gelu, 1 gelu_tanh,
    2 silu (the decode programs' numbering)."""
    y = linear_q8_reference(x, q, scale)
    inter = q.shape[0] // 2
    g, u = y[:, :inter], y[:, inter:]
    g = torch.nn.functional.silu(g) if kind == 2 else _gelu(g, 1 if kind == 0 else 2)
    return g * u


def rope_q8_reference(x: Tensor, q: Tensor, scale: Tensor, cos: Tensor, sin: Tensor, D: int, nrot: int) -> Tensor:
    """The QKV rows x · (q·scale)ᵀ with one position's rotation (cos / sin [D/2], rotate-half pairs
    j, j + D/2) applied to the first ``nrot`` heads of size D, in fp32."""
    y = linear_q8_reference(x, q, scale).view(x.shape[0], -1, D)
    lo, hi = y[:, :nrot, :D // 2], y[:, :nrot, D // 2:]
    c, s = cos.float().view(1, 1, -1), sin.float().view(1, 1, -1)
    rot = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=2)
    return torch.cat([rot, y[:, nrot:]], dim=1).reshape(x.shape[0], -1)


def cached_q8(owner, slot: str, sources: tuple[Tensor, ...], build=None) -> tuple[Tensor, Tensor]:
    """The quantised copy of ``owner``'s weight, built once per weight version and kept in the
    module's ``__dict__`` under ``slot`` (as ``_packed_gate_up`` keeps the packed gate|up weight), so
    every decoder of the model shares one copy and an in-place update builds a new one. ``sources``
    are the parameters it derives from; ``build()`` returns the float weight to quantise (default:
    the one source)."""
    key = tuple(v for s in sources for v in (s.data_ptr(), s._version))
    hit = owner.__dict__.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        qs = quantize_rows_int8(build() if build is not None else sources[0])
    owner.__dict__[slot] = (key, qs)
    return qs


def linear_q8(lin) -> tuple[Tensor, Tensor]:
    """(q, scale) of an ``nn.Linear``'s weight, cached on the module."""
    return cached_q8(lin, "_q8_weight", (lin.weight,))
