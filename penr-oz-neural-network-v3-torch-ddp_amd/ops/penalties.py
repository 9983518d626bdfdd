"""Repetition, presence and frequency penalties on the logits, before the sampler.

Definition (vLLM's ``apply_penalties``; the repetition part is HF's
``RepetitionPenaltyLogitsProcessor``). For row ``b`` and token ``v``, with ``x`` the raw logit
(before temperature), ``in_prompt`` whether ``v`` occurs anywhere in the row's prompt — the whole
input context of the call, tokens beyond the block size included — and ``c`` how often ``v`` has
been generated so far in this call and row:

1. repetition, if ``in_prompt or c > 0``, with ``r = repetition_penalty > 0``:
   ``y = x / r`` when ``x > 0``, else ``y = x * r`` (once per distinct token, however often seen);
2. presence and frequency, if ``c > 0``: ``y = y - (presence_penalty + frequency_penalty * c)``, the
   bracket formed first. Prompt tokens do not count here.

Every operation is fp32 and rounded on its own; the result is rounded once to the logits' dtype.
Order: penalties, then temperature, top-k, top-p, min-p and the draw (``ops/sampling.py``); greedy
decoding takes the argmax of the penalised row. The parameters are shared by all rows of a call,
the counts are per row. ``repetition_penalty`` 1.0 / None and the other two 0.0 / None are neutral;
with all three neutral nothing runs at all.

GPU: ``csrc/kernels/logit_penalty.hip``. The state is a count table ``cnt`` int32 [B, V] (bit 31:
in the prompt; low bits: the generated count), the list ``uniq`` / ``n_uniq`` of the tokens whose
entry is non-zero, and ``params`` fp32 [3] on the device, so a captured decode graph replays with
other values. Both kernels walk the list, never the row: a step costs what the distinct tokens
seen cost, not what the vocabulary would.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels


def check_penalties(repetition_penalty: float | None, presence_penalty: float | None,
                    frequency_penalty: float | None) -> tuple[float, float, float] | None:
    """(repetition, presence, frequency) as numbers, or None when all three are neutral (1.0 / 0.0
    / 0.0 or None). ValueError unless repetition is finite and > 0 and the other two are finite."""
    r = 1.0 if repetition_penalty is None else float(repetition_penalty)
    p = 0.0 if presence_penalty is None else float(presence_penalty)
    f = 0.0 if frequency_penalty is None else float(frequency_penalty)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty}")
    if not math.isfinite(p):
        raise ValueError(f"presence_penalty must be finite, got {presence_penalty}")
    if not math.isfinite(f):
        raise ValueError(f"frequency_penalty must be finite, got {frequency_penalty}")
    if r == 1.0 and p == 0.0 and f == 0.0:
        return None
    return r, p, f


def reference_penalise(logits: Tensor, in_prompt: Tensor, out_count: Tensor, r: float, p: float, f: float) -> Tensor:
    """logits [B, V], in_prompt [B, V] bool, out_count [B, V] int -> the penalised logits, same
    dtype: the module docstring's definition in plain torch, fp32, rounded once."""
    x = logits.float()
    par = torch.tensor([r, p, f], dtype=torch.float32, device=x.device)
    gen = out_count > 0
    y = torch.where(in_prompt | gen, torch.where(x > 0, x / par[0], x * par[0]), x)
    y = torch.where(gen, y - (par[1] + par[2] * out_count.float()), y)
    return y.to(logits.dtype)


class PenaltyState:
    """The penalties' per-row bookkeeping over one generate call, and their application.

    ``set_params`` → ``begin(prompt)`` once per call → ``apply(logits, None)`` for the first
    sampling → ``apply(logits, previous tokens)`` for every later one, so each generated token is
    counted exactly once. GPU logits go through the kernels and are modified in place (the same
    tensor is returned); anything else runs ``reference_penalise`` on dense ``in_prompt`` /
    ``out_count`` tensors. Buffers are allocated when the vocabulary size is first known — the
    first ``apply`` — and kept: their addresses may be held by a captured graph, in which ``apply``
    launches one kernel and allocates nothing.
    """

    def __init__(self):
        self.values: tuple[float, float, float] = (1.0, 0.0, 0.0)
        self._prompt: Tensor | None = None  # begin() before the buffers exist: registered by the first apply
        self._shape: tuple | None = None    # (backend, B, V, device)
        # kernel backend
        self.cnt = self.uniq = self.n_uniq = self.params = None
        # dense backend
        self.in_prompt = self.out_count = None

    # ------------------------------------------------------------------ parameters
    def set_params(self, r: float, p: float, f: float) -> None:
        self.values = (float(r), float(p), float(f))
        if self.params is not None:
            self.params.copy_(torch.tensor(self.values, dtype=torch.float32))

    # ------------------------------------------------------------------ a call
    def begin(self, prompt: Tensor) -> None:
        """Start a call: forget the previous one, mark the tokens of ``prompt`` [B, T] (or [T])."""
        prompt = prompt.detach().long()
        if prompt.ndim == 1:
            prompt = prompt.unsqueeze(0)
        if self._shape is None or self._shape[1] != prompt.shape[0]:
            self._prompt, self._shape = prompt, None  # the first apply knows V
            return
        self._register(prompt)

    def _register(self, prompt: Tensor) -> None:
        backend, B, V, device = self._shape
        prompt = prompt.to(device).contiguous()
        if prompt.numel():
            lo, hi = (int(v) for v in torch.stack(prompt.aminmax()).tolist())  # once per call, on the host
            if lo < 0 or hi >= V:
                raise ValueError(f"prompt token ids must be in [0, {V}), got {lo}..{hi}")
        if backend == "kernel":
            kernels().penalty_begin(self.cnt, self.uniq, self.n_uniq, prompt)
        else:
            self.in_prompt.zero_()
            self.out_count.zero_()
            if prompt.numel():
                self.in_prompt.scatter_(1, prompt, True)
        self._prompt = None

    def _allocate(self, logits: Tensor) -> None:
        B, V = logits.shape
        backend = "kernel" if use_kernels(logits) else "dense"
        shape = (backend, B, V, logits.device)
        if shape == self._shape:
            return
        prompt = self._prompt
        if prompt is None:
            raise RuntimeError("PenaltyState.apply: begin() has not run for these logits' shape "
                               f"{tuple(logits.shape)} on {logits.device}")
        assert not (logits.is_cuda and torch.cuda.is_current_stream_capturing()), \
            "the penalty state must exist before a graph capture"
        self.cnt = self.uniq = self.n_uniq = self.params = self.in_prompt = self.out_count = None
        if backend == "kernel":
            self.cnt = torch.zeros(B, V, dtype=torch.int32, device=logits.device)
            self.uniq = torch.zeros(B, V, dtype=torch.int32, device=logits.device)
            self.n_uniq = torch.zeros(B, dtype=torch.int32, device=logits.device)
            self.params = torch.tensor(self.values, dtype=torch.float32, device=logits.device)
        else:
            self.in_prompt = torch.zeros(B, V, dtype=torch.bool, device=logits.device)
            self.out_count = torch.zeros(B, V, dtype=torch.long, device=logits.device)
        self._shape = shape
        self._register(prompt)

    @property
    def ready(self) -> bool:
        """Buffers exist and ``begin`` has been applied to them (what a graph capture needs)."""
        return self._shape is not None and self._prompt is None

    def apply(self, logits: Tensor, new_tok: Tensor | None) -> Tensor:
        """Count ``new_tok`` [B, 1] (the tokens the previous step sampled; None: none yet), then
        penalise ``logits`` [B, V]. Kernel backend: ``logits`` must be contiguous, is modified in
        place and returned."""
        if self._prompt is not None or self._shape is None or self._shape[1:] != (*logits.shape, logits.device):
            self._allocate(logits)
        if self._shape[0] == "kernel":
            if new_tok is not None:  # (a column sliced out of a context is strided; a decoder's idx is not)
                new_tok = new_tok.reshape(-1).contiguous()
            kernels().penalty_apply(logits, self.cnt, self.uniq, self.n_uniq, self.params, new_tok)
            return logits
        if new_tok is not None:
            tok = new_tok.reshape(-1, 1).to(self.out_count.device)
            self.out_count.scatter_add_(1, tok, torch.ones_like(tok))
        return reference_penalise(logits, self.in_prompt, self.out_count, *self.values)

    def dense(self) -> tuple[Tensor, Tensor]:
        """(in_prompt [B, V] bool, out_count [B, V] int64) on either backend."""
        if not self.ready:
            raise RuntimeError("PenaltyState.dense: no call has begun on allocated buffers")
        if self._shape[0] == "kernel":
            return self.cnt < 0, (self.cnt & 0x7FFFFFFF).long()
        return self.in_prompt.clone(), self.out_count.clone()
