"""Log-probabilities of given tokens: how likely a text is under the model (perplexity, ranking
continuations, ``loglikelihood`` / ``is_greedy`` requests, ``echo`` + ``logprobs``).

Definition. ``h [N, C]`` are the rows entering the lm_head (the output of the last layer before the
final ``nn.Linear``), ``W [V, C]`` and the optional ``bias [V]`` that linear's parameters, ``targets
[N]`` int64 in ``[0, V)``. With ``x = h · Wᵀ (+ bias)`` computed from the stored operand values
**without rounding the logits to bf16**:

* ``token_logprob[i] = x[i, targets[i]] − logsumexp(x[i, :])``;
* ``top_token[i] = argmax_v x[i, v]``, the lowest id among equal maxima;
* ``top_logprob[i] = max_v x[i, v] − logsumexp(x[i, :])``.

With ``1 <= n <= 20`` (``top_n``, the option ``prompt_top_logprobs``):

* ``top_n[i]`` = the ``min(n, V)`` pairs ``(v, x[i, v] − logsumexp(x[i, :]))`` with the largest ``x[i, v]``, ordered
  by logit descending, by token id ascending among equal logits (the order ``ops/logprobs.py`` gives generated
  tokens), as ``ids int64 [N, n]`` and ``logprobs fp32 [N, n]`` with ``−1`` / ``−inf`` past ``min(n, V)``. Entry 0
  is ``(top_token[i], top_logprob[i])``.

This differs from the module path (``nn.Linear`` under autocast, ``ops/logprobs.py``), which rounds
the logits to bf16 before any softmax: the values here are those of the unrounded logits.

For a token sequence ``s`` of length ``L`` with ``2 <= L <= block_size``, position ``i`` in ``1 .. L − 1``
is scored from the hidden row at position ``i − 1`` with target ``s[i]``; position 0 has no score and is
``None`` in lists (``NeuralNetworkModel.score_tokens``).

``reference_score`` and ``reference_top_n`` are the definition in fp64. ``score_rows`` is what runs: for bf16 GPU operands of a
shape the launcher takes, ``csrc/kernels/lmhead_lse.hip`` — an MFMA kernel that sweeps ``h · Wᵀ`` tile by
tile and reduces every tile in registers (running maximum, Σexp, best column, target logit; with ``top_n``
the row's n best columns, selected in the same sweep), so no ``[N, V]`` tensor exists; otherwise the same maths in fp32 torch over chunks of rows, which never holds
more than one bounded ``[chunk, V]`` block.
"""
from __future__ import annotations

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels

CHUNK_ELEMS = 1 << 24  # the torch path's [chunk, V] fp32 block: at most 64 MiB
MAX_TOP_N = 20  # the kernel's list capacity (kLmheadTopCap, csrc/kernels/host_plan.h); ops/logprobs.py's limit too


def check_prompt_logprobs(value, *, speculate=None, stream: bool = False) -> bool:
    """``value`` as a bool (None: off). ValueError unless it is None or a bool, and for what the option
    does not compose with: ``speculate`` and streaming."""
    if value is None:
        return False
    if not isinstance(value, bool):
        raise ValueError(f"prompt_logprobs must be None or a bool, got {value!r}")
    if value and speculate:
        raise ValueError("prompt_logprobs does not compose with speculate")
    if value and stream:
        raise ValueError("prompt_logprobs does not stream: the prompt's scores come with the finished call")
    return value


def check_prompt_top_logprobs(value, *, prompt_logprobs: bool) -> int:
    """``value`` as n in 0..20 (None and 0: off). ValueError unless it is None or such an int (no bool), and
    for an n > 0 without ``prompt_logprobs`` — whose own check has already refused ``speculate`` and streams."""
    if value is None:
        return 0
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= MAX_TOP_N:
        raise ValueError(f"prompt_top_logprobs must be None or an int in [0, {MAX_TOP_N}], got {value!r}")
    if value and not prompt_logprobs:
        raise ValueError("prompt_top_logprobs needs prompt_logprobs: true (the most likely tokens come with the prompt's scores)")
    return value


def check_sequences(sequences, block_size: int, vocab: int | None) -> list[list[int]]:
    """``sequences`` as a list of lists of ints. ValueError unless it is a non-empty list of lists of
    ``2 <= L <= block_size`` token ids in ``[0, V)``, and for a model that shows no vocabulary."""
    if vocab is None:
        raise ValueError("prompt_logprobs needs a model whose layer list ends with the vocabulary projection "
                         "(a linear layer, then at most a softmax)")
    if not isinstance(sequences, (list, tuple)) or len(sequences) == 0:
        raise ValueError("the sequences to score must be a non-empty list of token id lists")
    out = []
    for b, row in enumerate(sequences):
        if not isinstance(row, (list, tuple)):
            raise ValueError(f"sequence {b} must be a list of token ids, got {type(row).__name__}")
        if not 2 <= len(row) <= int(block_size):
            raise ValueError(f"sequence {b}: a scored sequence has 2 to block_size ({block_size}) tokens, got {len(row)}")
        for t in row:
            if isinstance(t, bool) or not isinstance(t, int):
                raise ValueError(f"sequence {b} must hold integer token ids, got {t!r}")
            if not 0 <= t < vocab:
                raise ValueError(f"sequence {b}: token id {t} is outside [0, {vocab})")
        out.append([int(t) for t in row])
    return out


def _lowest_argmax(x: Tensor, best: Tensor) -> Tensor:
    """The lowest column id holding each row's maximum ``best`` (argmax alone leaves ties open)."""
    ids = torch.arange(x.shape[1], device=x.device)
    return torch.where(x == best.unsqueeze(1), ids, x.shape[1]).amin(dim=-1)


def reference_score(h: Tensor, W: Tensor, bias: Tensor | None, targets: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """The module docstring's definition in fp64: (token_logprob fp64 [N], top_token int64 [N],
    top_logprob fp64 [N]), on the operands' device."""
    x = h.double() @ W.double().T
    if bias is not None:
        x = x + bias.double()
    lse = torch.logsumexp(x, dim=-1)
    best = x.max(dim=-1).values
    top = _lowest_argmax(x, best)
    xt = x.gather(1, targets.to(x.device).long().reshape(-1, 1)).squeeze(1)
    return xt - lse, top, best - lse


def _top_n_of(x: Tensor, lse: Tensor, n: int) -> tuple[Tensor, Tensor]:
    """The definition's ``top_n`` of logits ``x [rows, V]``: (ids int64 [rows, n], x − lse in x's type [rows, n]).
    A stable descending sort keeps equal logits in ascending id order."""
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :n]
    ids = torch.full((x.shape[0], n), -1, dtype=torch.int64, device=x.device)
    lps = torch.full((x.shape[0], n), float("-inf"), dtype=x.dtype, device=x.device)
    ids[:, :order.shape[1]] = order
    lps[:, :order.shape[1]] = x.gather(1, order) - lse.unsqueeze(1)
    return ids, lps


def reference_top_n(h: Tensor, W: Tensor, bias: Tensor | None, n: int) -> tuple[Tensor, Tensor]:
    """The module docstring's ``top_n`` in fp64: (ids int64 [N, n], logprobs fp64 [N, n]), on the operands' device."""
    x = h.double() @ W.double().T
    if bias is not None:
        x = x + bias.double()
    return _top_n_of(x, torch.logsumexp(x, dim=-1), n)


def kernel_takes(h: Tensor, W: Tensor, bias: Tensor | None = None) -> bool:
    """Whether ``lmhead_lse``'s launcher accepts these operands once they are contiguous — every check it
    makes: bf16 GPU rows of a planned shape, a device bias [V], 16-B aligned data, and h and a column tile
    of W each below 4 GiB (the kernel's 32-bit byte offsets)."""
    if not (use_kernels(h) and W.is_cuda and h.dtype == torch.bfloat16 and W.dtype == torch.bfloat16):
        return False
    if h.dim() != 2 or W.dim() != 2 or h.shape[0] < 1 or h.shape[1] != W.shape[1]:
        return False
    if bias is not None and not (bias.is_cuda and bias.dim() == 1 and bias.numel() == W.shape[0]):
        return False
    if any(t.is_contiguous() and t.data_ptr() % 16 for t in (h, W)) or h.numel() * 2 >= 2 ** 32:
        return False  # (C <= 16384 keeps a 128-row tile of contiguous W far below 4 GiB)
    return kernels().lmhead_lse_plan(h.shape[0], W.shape[0], h.shape[1])[0] != 0


def score_rows(h: Tensor, W: Tensor, bias: Tensor | None, targets: Tensor, top_n: int = 0) -> tuple[Tensor, ...]:
    """(token_logprob fp32 [N], top_token int64 [N], top_logprob fp32 [N]) of the definition: the kernel for
    operands ``kernel_takes`` admits, otherwise fp32 torch over chunks of rows. ``top_n`` n in 1..20 appends
    the definition's ``top_n``: (ids int64 [N, n], logprobs fp32 [N, n])."""
    if isinstance(top_n, bool) or not 0 <= top_n <= MAX_TOP_N:
        raise ValueError(f"top_n must be an int in [0, {MAX_TOP_N}], got {top_n!r}")
    targets = targets.to(h.device).long().reshape(-1)
    bias = None if bias is None else bias.to(h.device)
    if kernel_takes(h, W, bias):
        if top_n:
            return kernels().lmhead_lse(h.contiguous(), W.contiguous(), bias, targets.contiguous(), top_n=top_n)
        return kernels().lmhead_lse(h.contiguous(), W.contiguous(), bias, targets.contiguous())
    N, V = h.shape[0], W.shape[0]
    n_ids = torch.empty(N, top_n, dtype=torch.int64, device=h.device)
    n_lps = torch.empty(N, top_n, dtype=torch.float32, device=h.device)
    lp = torch.empty(N, dtype=torch.float32, device=h.device)
    top_lp = torch.empty_like(lp)
    top = torch.empty(N, dtype=torch.int64, device=h.device)
    Wf = W.float().T
    step = max(1, CHUNK_ELEMS // max(1, V))
    for a in range(0, N, step):
        x = h[a:a + step].float() @ Wf
        if bias is not None:
            x += bias.float()
        lse = torch.logsumexp(x, dim=-1)
        best = x.max(dim=-1).values
        top[a:a + step] = _lowest_argmax(x, best)
        lp[a:a + step] = x.gather(1, targets[a:a + step].unsqueeze(1)).squeeze(1) - lse
        top_lp[a:a + step] = best - lse
        if top_n:
            n_ids[a:a + step], n_lps[a:a + step] = _top_n_of(x, lse, top_n)
    return (lp, top, top_lp, n_ids, n_lps) if top_n else (lp, top, top_lp)


def to_dicts(lens: list[int], lp: Tensor, top: Tensor, top_lp: Tensor, n_ids: Tensor | None = None,
             n_lps: Tensor | None = None) -> list[dict]:
    """The scored rows of sequences of ``lens`` tokens (``len − 1`` rows each, concatenated) as one dict
    per sequence: ``token_logprobs``, ``top_tokens``, ``top_logprobs``, each ``len`` long with None first.
    With ``score_rows``' ``top_n`` pair also ``"top_n"``: None, then per position the ``[id, logprob]`` pairs
    of its most likely tokens, best first (``min(n, V)`` of them)."""
    lps, tops, top_lps = lp.tolist(), top.tolist(), top_lp.tolist()
    pairs = None if n_ids is None else [[[i, p] for i, p in zip(ids, ps) if i >= 0]
                                        for ids, ps in zip(n_ids.tolist(), n_lps.tolist())]
    out, a = [], 0
    for n in lens:
        b = a + n - 1
        out.append({"token_logprobs": [None] + lps[a:b], "top_tokens": [None] + tops[a:b],
                    "top_logprobs": [None] + top_lps[a:b]})
        if pairs is not None:
            out[-1]["top_n"] = [None] + pairs[a:b]
        a = b
    return out
