"""Logit bias, banned and allowed tokens, and ``min_tokens``: one rewrite of the logits in front of the
sampler that constrains which tokens may come out.

Inputs. ``logit_bias`` is ``{token id: bias}`` (integer-like string keys are accepted, as JSON delivers
them), each bias finite and in [-100, 100]; ``banned_token_ids`` a list of ids; ``allowed_token_ids`` a
list of ids of any length, at least one; ``min_tokens`` an integer with 0 <= ``min_tokens`` <=
``max_new_tokens``. Every id is an int, not a bool, in ``[0, V)``. ``None``, ``{}``, ``[]`` and ``0`` are
neutral for ``logit_bias``, ``banned_token_ids`` and ``min_tokens``; ``allowed_token_ids=None`` is off and
``[]`` is an error. Anything else raises ``ValueError`` before any forward pass (``/generate`` answers 400).

Definition. Let ``t`` be the index, in this call and counting from 0, of the token about to be sampled
(the same for every row) and ``x`` the logit after the penalties (``ops/penalties.py``). Token ``v`` is
*masked* at step ``t`` if ``v`` is banned, or an allowed set is given and ``v`` is not in it, or
``t < min_tokens`` and ``v`` is an end token: ``stop_token``, or the single id of a one-token sequence in
``stop``. Longer stop sequences are not affected by ``min_tokens``: this is vLLM's rule, whose
``min_tokens`` suppresses EOS and ``stop_token_ids`` and nothing else. The sampler and the
log-probabilities then receive

    y = FLOOR                                    if v is masked,
    y = round_to_dtype(float32(x) + bias[v])     otherwise (bias[v] = 0 without an entry).

``FLOOR`` is -2^100 for bf16 and fp32 logits and -2^15 for fp16: a finite power of two, exact in the
dtype, and deliberately not -inf.
* ``token_logprobs.hip`` computes ``expf(r - m)`` per part of 4096 logits and the two-stage sampler works
  per part of a row: a part that is -inf throughout would make that ``exp(-inf - -inf)``, NaN. A finite
  floor underflows to a weight of exactly 0 in every existing kernel, without touching them.
* ``/generate``'s JSON stays free of ``-Infinity``: a masked token's reported log-probability is about
  -1.3e30, and such entries appear in ``top_logprobs`` only when fewer than n tokens remain unmasked.
``FLOOR / temperature`` has to stay finite in fp32, so a non-zero temperature below 1e-6 is refused while
any of the four is active.

Order: penalties, then this rewrite, then temperature, top-k, top-p, min-p and the draw
(``ops/sampling.py``); greedy decoding takes the argmax of ``y``. The values are shared by all rows of a
call. A call in which nothing would stay unmasked at some step — the allowed set (or the vocabulary)
minus the banned ids, minus the end tokens when ``min_tokens`` > 0, is empty — is refused.

Canonical form (``check_logit_bias``): one *entry* ``(id, bias, until)`` per token id, ascending by id, at
most 1024; it means FLOOR while ``t < until``, or when ``bias`` is -inf (a banned id, which wins over its
``logit_bias`` value), and ``+bias`` otherwise. An end token carries ``until = min_tokens`` and its
``logit_bias`` value, or 0. Entries for ids outside the allowed set are dropped: those ids are masked
anyway. The allowed set is a bitmask of ceil(V / 32) 32-bit words. So no logit has two writers: entries
touch only allowed ids, the mask only the others. Everything neutral gives None — off — and then nothing
runs at all.

GPU: ``csrc/kernels/logit_bias.hip``, one launch. The entries, the mask and ``base_t`` (the ``t`` of a
burst's first step; the captured step adds its own counter) live on the device, so a captured decode
graph replays with other values, another set and another ``min_tokens``.
"""
from __future__ import annotations

import math
import re
from typing import NamedTuple

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels

MAX_ENTRIES = 1024
MAX_BIAS = 100.0
MIN_TEMPERATURE = 1e-6


class Canonical(NamedTuple):
    """``check_logit_bias``' result: the entries as parallel tuples (ascending, distinct ids), the allowed
    ids ascending (None: no allowed set) and the vocabulary size they were checked against (None: not
    known yet, ids checked against 2^31 only)."""
    ids: tuple
    bias: tuple
    until: tuple
    allowed: tuple | None
    V: int | None

    @property
    def entries(self) -> list:
        return list(zip(self.ids, self.bias, self.until))

    def mask_words(self, V: int | None = None) -> Tensor:
        """The allowed set as int32 [ceil(V / 32)]: bit ``v % 32`` of word ``v // 32`` set for allowed ``v``."""
        V = self.V if V is None else int(V)
        words = torch.zeros((V + 31) // 32, dtype=torch.int64)
        ids = torch.tensor(self.allowed, dtype=torch.int64)
        words.index_put_((ids >> 5,), torch.ones_like(ids) << (ids & 31), accumulate=True)  # (distinct ids: a sum is an or)
        return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def floor_of(dtype: torch.dtype) -> float:
    """FLOOR of the module docstring for logits of ``dtype``."""
    return -(2.0 ** 15) if dtype == torch.float16 else -(2.0 ** 100)


def _token_id(what: str, v, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{what} must hold integer token ids, got {v!r}")
    if not 0 <= v < hi:
        raise ValueError(f"{what}: token id {v} is outside [0, {hi})")
    return int(v)


def _id_list(what: str, ids, hi: int) -> list[int]:
    if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple)):
        raise ValueError(f"{what} must be a list of token ids, got {type(ids).__name__}")
    return [_token_id(what, v, hi) for v in ids]


def check_logit_bias(logit_bias, banned_token_ids, allowed_token_ids, min_tokens, end_tokens, V: int | None,
                     max_new_tokens: int, temperature: float | None = None) -> Canonical | None:
    """The canonical form of the module docstring, or None when everything is neutral. ``end_tokens``: the
    ``stop_token`` and the ids of the one-token stop sequences (ids outside the vocabulary never come out
    and are left aside); ``V`` None: the vocabulary is not known yet, ids are checked against 2^31.
    ``temperature``, where given, is refused between 0 and 1e-6 while anything is active. ValueError for
    whatever the module docstring does not allow."""
    hi = 2 ** 31 if V is None else int(V)
    bias: dict[int, float] = {}
    if logit_bias is not None:
        if not isinstance(logit_bias, dict):
            raise ValueError(f"logit_bias must map token ids to biases, got {type(logit_bias).__name__}")
        for k, b in logit_bias.items():
            if isinstance(k, str) and re.fullmatch(r"\s*[+-]?\d+\s*", k):
                k = int(k)
            k = _token_id("logit_bias", k, hi)
            if isinstance(b, bool) or not isinstance(b, (int, float)):
                raise ValueError(f"logit_bias[{k}] must be a number, got {b!r}")
            if not (math.isfinite(b) and -MAX_BIAS <= b <= MAX_BIAS):
                raise ValueError(f"logit_bias[{k}] must be finite and in [-{MAX_BIAS:g}, {MAX_BIAS:g}], got {b}")
            if k in bias:
                raise ValueError(f"logit_bias names token id {k} twice")
            bias[k] = float(b)
    banned = set() if banned_token_ids is None else set(_id_list("banned_token_ids", banned_token_ids, hi))
    allowed = None
    if allowed_token_ids is not None:
        allowed = set(_id_list("allowed_token_ids", allowed_token_ids, hi))
        if not allowed:
            raise ValueError("allowed_token_ids must hold at least one token id (None: no restriction)")
    if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int):
        raise ValueError(f"max_new_tokens must be an integer, got {max_new_tokens!r}")
    m = 0 if min_tokens is None else min_tokens
    if isinstance(m, bool) or not isinstance(m, int):
        raise ValueError(f"min_tokens must be an integer, got {min_tokens!r}")
    if not 0 <= m <= max_new_tokens:
        raise ValueError(f"min_tokens must be in [0, max_new_tokens = {max_new_tokens}], got {m}")
    ends = set()
    if m > 0:
        ends = {int(e) for e in (end_tokens or ()) if isinstance(e, int) and not isinstance(e, bool) and 0 <= e < hi}
    bias = {k: b for k, b in bias.items() if b != 0.0}
    if allowed is None and not (bias or banned or ends):
        return None
    if temperature is not None and temperature != 0 and abs(temperature) < MIN_TEMPERATURE:
        raise ValueError(f"logit_bias / banned_token_ids / allowed_token_ids / min_tokens need temperature 0 or at "
                         f"least {MIN_TEMPERATURE:g} (FLOOR / temperature must stay finite), got {temperature}")
    blocked = banned | ends
    left = len(allowed - blocked) if allowed is not None else (None if V is None else hi - len(blocked))
    if left is not None and left <= 0:
        raise ValueError("no token would stay unmasked: the allowed set (or the vocabulary) minus the banned ids"
                         + (", minus the end tokens while min_tokens holds," if ends else "") + " is empty")
    entries = []
    for v in sorted(banned | ends | set(bias)):
        if allowed is not None and v not in allowed:
            continue  # masked anyway: the mask writes it
        if v in banned:
            entries.append((v, -math.inf, 0))
        else:
            entries.append((v, bias.get(v, 0.0), m if v in ends else 0))
    if len(entries) > MAX_ENTRIES:
        raise ValueError(f"logit_bias, banned_token_ids and the end tokens together take at most {MAX_ENTRIES} "
                         f"entries, got {len(entries)}")
    ids, bs, us = (tuple(c) for c in zip(*entries)) if entries else ((), (), ())
    return Canonical(ids, bs, us, None if allowed is None else tuple(sorted(allowed)), None if V is None else hi)


def end_tokens_of(stop_token, stop) -> list[int]:
    """The end tokens ``min_tokens`` suppresses: ``stop_token`` and every one-token sequence of ``stop``
    (``ops.stopping.check_stop``'s result, or None)."""
    ends = [stop_token] if isinstance(stop_token, int) and not isinstance(stop_token, bool) else []
    return ends + [s[0] for s in (stop or []) if len(s) == 1]


def reference_bias(logits: Tensor, canonical: Canonical | None, t) -> Tensor:
    """logits [B, V] -> what the sampler receives at step ``t`` (an int, or a one-element integer tensor
    on the logits' device, which is never read on the host), same dtype: the module docstring's
    definition in plain torch (the add in fp32, rounded once). The input is left as it is."""
    out = logits.clone()
    if canonical is None:
        return out
    V = logits.shape[-1]
    floor = torch.tensor(floor_of(logits.dtype), dtype=logits.dtype, device=logits.device)
    if canonical.ids:
        ids = torch.tensor(canonical.ids, dtype=torch.long, device=logits.device)
        b = torch.tensor(canonical.bias, dtype=torch.float32, device=logits.device)
        until = torch.tensor(canonical.until, dtype=torch.long, device=logits.device)
        masked = (b == -math.inf) | ((t if isinstance(t, Tensor) else int(t)) < until)
        summed = (logits[:, ids].float() + torch.where(masked, torch.zeros_like(b), b)).to(logits.dtype)
        out[:, ids] = torch.where(masked, floor, summed)
    if canonical.allowed is not None:
        keep = torch.zeros(V, dtype=torch.bool, device=logits.device)
        keep[torch.tensor(canonical.allowed, dtype=torch.long, device=logits.device)] = True
        out[:, ~keep] = floor
    return out


class BiasState:
    """The canonical form on the logits' device, and its application, over the generate calls of one
    decoder (or one eager call).

    ``set(canonical)`` once per generate call → ``apply(logits, t)`` for an eager sampling of the call's
    token ``t`` → ``step(logits, step_t)`` inside the captured step, where ``t`` is ``base_t`` (written by
    the decoder for each burst) plus the burst's own counter. GPU logits go through the kernel and are
    modified in place (the same tensor is returned); anything else runs ``reference_bias``. The entry
    buffers are allocated here and the mask by the first ``set`` that needs it — outside any capture — and
    kept: a captured graph holds their addresses, and ``step`` launches one kernel and allocates nothing.
    """

    def __init__(self, device):
        self.device = torch.device(device)
        self.canonical: Canonical | None = None
        self.ids = torch.zeros(MAX_ENTRIES, dtype=torch.int32, device=self.device)
        self.bias = torch.zeros(MAX_ENTRIES, dtype=torch.float32, device=self.device)
        self.until = torch.zeros(MAX_ENTRIES, dtype=torch.int32, device=self.device)
        self.n_entries = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.base_t = torch.zeros(1, dtype=torch.long, device=self.device)
        self.allow: Tensor | None = None  # int32 [ceil(V / 32)], once an allowed set has been given
        self.allow_on = False

    @property
    def form(self) -> str:
        """"off", "entries" or "mask": the launch form of the canonical form last set."""
        return "off" if self.canonical is None else "mask" if self.allow_on else "entries"

    def set(self, canonical: Canonical | None) -> None:
        """``check_logit_bias``' result, checked against the vocabulary (None: nothing is applied)."""
        self.canonical = canonical
        self.allow_on = canonical is not None and canonical.allowed is not None
        if canonical is None:
            self.n_entries.zero_()
            return
        assert canonical.V is not None and len(canonical.ids) <= MAX_ENTRIES, "check_logit_bias with V comes first"
        n = len(canonical.ids)
        pad = [0] * (MAX_ENTRIES - n)
        self.ids.copy_(torch.tensor(list(canonical.ids) + pad, dtype=torch.int32))
        self.bias.copy_(torch.tensor(list(canonical.bias) + pad, dtype=torch.float32))
        self.until.copy_(torch.tensor(list(canonical.until) + pad, dtype=torch.int32))
        self.n_entries.fill_(n)
        if self.allow_on:
            words = canonical.mask_words()
            if self.allow is None or self.allow.numel() != words.numel():
                assert not (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()), \
                    "the allowed mask must exist before a graph capture"
                self.allow = torch.zeros_like(words, device=self.device)
            self.allow.copy_(words)

    def _check(self, logits: Tensor) -> None:
        if self.canonical.V != logits.shape[-1]:
            raise ValueError(f"logit bias: checked against a vocabulary of {self.canonical.V}, the logits have "
                             f"{logits.shape[-1]}")

    def apply(self, logits: Tensor, t: int) -> Tensor:
        """An eager sampling of the call's token ``t``: fills ``base_t`` and rewrites ``logits`` [B, V]
        (kernel: contiguous, in place, the same tensor is returned)."""
        if self.canonical is None:
            return logits
        self._check(logits)
        self.base_t.fill_(int(t))
        if use_kernels(logits):
            kernels().logit_bias_apply(logits, self.ids, self.bias, self.until, self.n_entries, self.allow,
                                       self.allow_on, self.base_t, None)
            return logits
        return reference_bias(logits, self.canonical, int(t))

    def step(self, logits: Tensor, step_t: Tensor) -> Tensor:
        """The captured step's form: ``t = base_t + step_t``, both read on the device. One launch,
        nothing allocated."""
        if self.canonical is None:
            return logits
        self._check(logits)
        if use_kernels(logits):
            kernels().logit_bias_apply(logits, self.ids, self.bias, self.until, self.n_entries, self.allow,
                                       self.allow_on, self.base_t, step_t)
            return logits
        return reference_bias(logits, self.canonical, self.base_t + step_t.to(self.base_t.device))  # (t stays on the device)
