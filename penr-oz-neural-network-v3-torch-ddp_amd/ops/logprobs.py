"""Per-token log-probabilities of the tokens a generate call returns.

Definition. For row ``b``, let ``x`` be the logits the sampler receives: after the penalties when they
are on (``ops/penalties.py``), before temperature, top-k, top-p and min-p. Let ``t`` be the token the
sampler then chose.

* ``lse = log Σ_v exp(x_v)`` over the whole row;
* ``token_logprob = x_t − lse``;
* ``top_logprobs(n)`` is the ``min(n, V)`` entries with the largest ``x_v``, each as ``(v, x_v − lse)``,
  ordered by ``x_v`` descending and, among equal logits, by ``v`` ascending. Comparison is exact, on the
  stored values.

The distribution is the model's own (penalised) one at temperature 1: it does not depend on how the
token was drawn, and the sampled token need not be among the top ``n``. Logits are assumed finite.

``logprobs`` is None (off) or an integer ``0 <= n <= 20``; 0 returns only the chosen tokens'
log-probabilities. Anything else is a ValueError (a 422 from the API), raised before any forward pass.

``reference_logprobs`` is the definition in plain torch, fp64 rounded once to fp32: what runs on the
CPU, and what the kernel is held to. GPU: ``csrc/kernels/token_logprobs.hip`` — a part kernel over
4096-logit parts of every row and a merge kernel per row, ``n`` and the token read on the device, so a
captured decode step (``models/graph_decode.py``) replays with another ``n``.
"""
from __future__ import annotations

import gc
import operator

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels

MAX_LOGPROBS = 20  # (csrc/kernels/host_plan.h kLogprobMaxN: the top slots of the burst buffers)


def check_logprobs(n) -> int | None:
    """``n`` as an int, or None (off). ValueError unless it is an integer in [0, 20]."""
    if n is None:
        return None
    try:
        if isinstance(n, bool):
            raise TypeError
        v = operator.index(n)
    except TypeError:
        raise ValueError(f"logprobs must be None or an integer in [0, {MAX_LOGPROBS}], got {n!r}") from None
    if not 0 <= v <= MAX_LOGPROBS:
        raise ValueError(f"logprobs must be in [0, {MAX_LOGPROBS}], got {n}")
    return v


def reference_logprobs(logits: Tensor, tokens: Tensor, n: int) -> tuple[Tensor, Tensor, Tensor]:
    """logits [B, V], tokens [B] or [B, 1], n -> (lp fp32 [B], top_id int64 [B, min(n, V)], top_lp fp32
    [B, min(n, V)]): the module docstring's definition in fp64, rounded once to fp32."""
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    tok = tokens.reshape(-1, 1).to(x.device).long()
    lp = (x.gather(1, tok) - lse).squeeze(1).float()
    k = min(int(n), x.shape[1])
    order = torch.sort(x, dim=-1, descending=True, stable=True)  # stable: equal logits keep ascending ids
    top_id = order.indices[:, :k].contiguous()
    top_lp = (order.values[:, :k] - lse).float()
    return lp, top_id, top_lp


def token_logprobs(logits: Tensor, tokens: Tensor, n: int) -> tuple[Tensor, Tensor, Tensor]:
    """``reference_logprobs``' result for the logits an eager step handed its sampler: the kernels
    for GPU logits, the reference otherwise."""
    if use_kernels(logits):
        return kernels().token_logprobs(logits.contiguous(), tokens.reshape(-1).contiguous(), int(n))
    return reference_logprobs(logits, tokens, n)


class LogprobState:
    """A decoder's log-probability buffers: ``n_t`` int32 [1] (read on the device), the burst's
    ``lp`` fp32 [rows, cap], ``top_id`` int32 / ``top_lp`` fp32 [rows, cap, 20] and the kernels'
    workspace. ``step`` runs after the sampler and the counter advance and fills column
    ``step_t - 1``; top slots from ``n`` on hold id -1 and -inf. Everything is allocated outside a
    graph capture: the burst buffers here, the workspace (whose size follows V) by the first
    ``step``, which a decoder's warm-up step makes before it captures."""

    def __init__(self, rows: int, cap: int, device):
        self.n = 0
        self.n_t = torch.zeros(1, dtype=torch.int32, device=device)
        self.lp = torch.zeros(rows, cap, dtype=torch.float32, device=device)
        self.top_id = torch.full((rows, cap, MAX_LOGPROBS), -1, dtype=torch.int32, device=device)
        self.top_lp = torch.full((rows, cap, MAX_LOGPROBS), float("-inf"), dtype=torch.float32, device=device)
        self.workspace: Tensor | None = None
        self._slots = torch.arange(MAX_LOGPROBS, device=device)

    def set_n(self, n: int) -> None:
        self.n = int(n)
        self.n_t.fill_(self.n)

    def _workspace(self, logits: Tensor) -> Tensor:
        need = logits.shape[0] * kernels().token_logprobs_plan(logits.shape[1])[1]
        if self.workspace is None or self.workspace.numel() < need:
            assert not torch.cuda.is_current_stream_capturing(), "the log-probability workspace must exist before a graph capture"
            self.workspace = torch.empty(need, dtype=torch.float32, device=logits.device)
        return self.workspace

    def step(self, logits: Tensor, idx: Tensor, step_t: Tensor) -> None:
        """logits [rows, V]: what the sampler read; idx [rows, 1]: the tokens it wrote; step_t int64
        [1]: the burst's step counter, already advanced."""
        if use_kernels(logits):
            kernels().token_logprobs_step(logits, idx.view(-1), step_t, self.n_t, self.lp, self.top_id,
                                          self.top_lp, self._workspace(logits))
            return
        # the same definition in capturable torch ops (fp32): no kernel extension on this device
        x = logits.float()
        lse = torch.logsumexp(x, dim=-1, keepdim=True)
        col = step_t - 1
        self.lp.index_copy_(1, col, x.gather(1, idx.view(-1, 1)) - lse)
        k = min(MAX_LOGPROBS, x.shape[1])
        order = torch.sort(x, dim=-1, descending=True, stable=True)
        used = (self._slots[:k] < self.n_t).unsqueeze(0)
        ids = torch.where(used, order.indices[:, :k], -1).to(torch.int32)
        lps = torch.where(used, order.values[:, :k] - lse, float("-inf"))
        if k < MAX_LOGPROBS:
            ids = torch.nn.functional.pad(ids, (0, MAX_LOGPROBS - k), value=-1)
            lps = torch.nn.functional.pad(lps, (0, MAX_LOGPROBS - k), value=float("-inf"))
        self.top_id.index_copy_(1, col, ids.unsqueeze(1))
        self.top_lp.index_copy_(1, col, lps.unsqueeze(1))

    def burst(self, n_steps: int) -> tuple[Tensor, Tensor, Tensor]:
        """The first ``n_steps`` columns: (lp [rows, n_steps], top_id and top_lp [rows, n_steps, 20])."""
        return self.lp[:, :n_steps], self.top_id[:, :n_steps], self.top_lp[:, :n_steps]


def step_logprobs(state: LogprobState, logits: Tensor, idx: Tensor, step_t: Tensor) -> None:
    """The decode step's call (``GraphDecoder._step`` goes through this module attribute)."""
    state.step(logits, idx, step_t)


def to_lists(lp: Tensor, top_id: Tensor, top_lp: Tensor, n: int) -> tuple[list, list]:
    """One block of steps on the host, copied once: lp [rows, k], top_id / top_lp [rows, k, >= min(n, V)]
    -> (lp as [rows][k] floats, tops as [rows][k] lists of [id, logprob], unused slots dropped).
    The cyclic garbage collector pauses meanwhile: 64 rows x 128 steps x 20 pairs are 164 k small
    lists that hold no cycle, and its passes over them cost several times what building them does."""
    lps = lp.tolist()
    ids, vals = top_id[..., :n].tolist(), top_lp[..., :n].tolist()
    gc_on = gc.isenabled()
    gc.disable()
    try:
        tops =[[[[i, v] for i, v in zip(si, sv) if i >= 0] for si, sv in zip(ri, rv)] for ri, rv in zip(ids, vals)]
    finally:
        if gc_on:
            gc.enable()
    return lps, tops
