"""``n``: several independent samples of one prompt, and the attention that serves them.

``n = k`` (2 <= k <= 64) on one prompt ``p`` means the call ``generate_batch([p] * k, ...)``: there are k rows,
row r draws from the sampler's stream of row r, and all rows are at the same position in every step. The
distribution and the return shape are the replicated call's; the bits of the logits may differ, because the
attention sums in another order. ``n`` of None or 1 is neutral: the call, the step, the return values and the
graphs are exactly what they are without it.

The replicated call prefills the prompt k times, stores its K/V k times and reads it k times per decode step.
On the GPU (``models/graph_decode.py``, ``GraphDecoder(shared_prefix=True)``) an ``n`` call prefills row 0 alone
into a batch-1 *prefix* cache, gives every row a *suffix* cache for the tokens it generates, and attends with
``csrc/kernels/shared_prefix_attn.hip``: every prefix key is read once per KV head and scored against all rows
on the matrix cores. Row r's keys are the prefix keys followed by row r's own suffix keys
(``reference_attention``). A row's bits depend on its own query, the prefix, its suffix, the prefix length and
the number of prefix key ranges S, which sets the order of the sums. Under the int8 KV cache
(``TURBO_QUANT_KV_CACHE=1``) the same step runs over int8 caches with per-token scales
(``csrc/kernels/shared_prefix_attn_q8.hip``, ``reference_attention_q8``). At equal S they do not depend on the
row count or on the other rows; the launch plan chooses S from the row count (with the heads and the
capacity), so calls with different ``n`` may run different S and round a row differently. Elsewhere — the CPU, ``PENROZ_GRAPH_DECODE=0``, a model without a decode program, fp32
parameters, a shape the kernel's plan refuses, ``PENROZ_SHARED_PREFIX=0`` — the replicated
call runs, which is the same thing by definition; logged once per process.

An ``n`` call takes one prompt row, does not stream, does not speculate, is ``generate_batch``'s (the other
generate methods return one row), and never slides its window: ``len(prompt) + max_new_tokens <= block_size``,
for the reason a ragged call does not (the re-prefill is a whole-batch operation on one cache).

``share_prefix=True`` (``generate_batch`` of 2..64 prompt rows) is the general case: the rows are DIFFERENT prompts
that begin with the same tokens. The call returns what the same call without the option returns — row b is the
one-row generation from prompt b (ops/ragged.py); same distribution, same return shape, the bits of the logits may
differ. ``split_prompts`` cuts the rows at ``P = min(longest common prefix, min(len_b) - 1)``, so every row keeps a
remainder of at least one token and draws its first token from its own logits. On the GPU the prefix is prefilled
once into the batch-1 prefix cache, the remainders — right-padded with each row's own last token — run as one
pass whose attention is the prefill form of the kernel (``reference_prefill_attention``), and the decode steps run
the rows at their own lengths over that prefix and their own suffixes. ``n`` is the special case of equal rows
(whose remainder is empty, so its first token comes from the prefix pass). Where ``n`` falls back, and when
``P == 0``, the plain call runs. There is no threshold on ``P``: the option is the caller's statement that the
prefix is worth sharing (profiles/shared_prefix_batch.md shows where it is not). Not with ``n``, ``speculate`` or
``stream``; ``max(len_b) + max_new_tokens <= block_size``.
"""
from __future__ import annotations

import logging
import math
import os

import torch
from torch import Tensor

log = logging.getLogger(__name__)

MAX_N = 64  # the decode step's most rows


def enabled() -> bool:
    """``PENROZ_SHARED_PREFIX=0``: the A/B switch — every ``n`` call runs replicated."""
    return os.environ.get("PENROZ_SHARED_PREFIX", "1") != "0"


def check_n(n, *, rows: int | None = None, prompt_len: int | None = None, max_new_tokens: int | None = None,
            block_size: int | None = None, stream: bool = False, speculate: int | None = None,
            single: bool = False) -> int | None:
    """k in 2..64, or None for neutral (None, 1). ``rows``, ``prompt_len``, ``block_size``, ``stream``: the call's
    shape where it is known; ``single``: the caller returns one row (``generate_tokens*``). ValueError for
    what an ``n`` call does not take."""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_N:
        raise ValueError(f"n must be None or an integer in [1, {MAX_N}], got {n!r}")
    if n == 1:
        return None
    if single:
        raise ValueError("n samples are n rows: generate_tokens and generate_tokens_stream return one row; use "
                         "generate_batch")
    if stream:
        raise ValueError("n samples are returned together: not together with stream")
    if speculate:
        raise ValueError("n does not compose with speculate (one greedy sequence)")
    if rows is not None and rows != 1:
        raise ValueError(f"n samples one prompt, got {rows} prompt rows")
    if None not in (prompt_len, max_new_tokens, block_size) and prompt_len + max_new_tokens > block_size:
        raise ValueError(f"an n call does not slide its window: prompt ({prompt_len}) + max_new_tokens "
                         f"({max_new_tokens}) must be <= block_size ({block_size})")
    return int(n)


def check_share_prefix(share_prefix, *, n=None, rows: int | None = None, prompt_len: int | None = None,
                       max_new_tokens: int | None = None, block_size: int | None = None, stream: bool = False,
                       speculate: int | None = None, single: bool = False) -> bool:
    """True, or False for neutral (None, False). ``rows`` / ``prompt_len`` (the longest row's) / ``block_size`` /
    ``stream``: the call's shape where it is known; ``single``: the caller returns one row. ValueError for what
    a ``share_prefix`` call does not take."""
    if share_prefix is None or share_prefix is False:
        return False
    if share_prefix is not True:
        raise ValueError(f"share_prefix must be None or a boolean, got {share_prefix!r}")
    if single:
        raise ValueError("share_prefix is a batch's option: generate_tokens and generate_tokens_stream return one "
                         "row; use generate_batch")
    if stream:
        raise ValueError("share_prefix returns its rows together: not together with stream")
    if n is not None and n != 1:
        raise ValueError("share_prefix takes different prompts, n one prompt: not both")
    if speculate:
        raise ValueError("share_prefix does not compose with speculate (one greedy sequence)")
    if rows is not None and not 2 <= rows <= MAX_N:
        raise ValueError(f"share_prefix takes 2 to {MAX_N} prompt rows, got {rows}")
    if None not in (prompt_len, max_new_tokens, block_size) and prompt_len + max_new_tokens > block_size:
        raise ValueError(f"a share_prefix call does not slide its window: the longest prompt ({prompt_len}) + "
                         f"max_new_tokens ({max_new_tokens}) must be <= block_size ({block_size})")
    return True


def split_prompts(prompts: list[list[int]]) -> int:
    """P, where a ``share_prefix`` call cuts its rows: the longest common prefix, but at most ``min(len_b) - 1`` —
    every row keeps a remainder of at least one token. 0: nothing to share."""
    shortest = min(len(p) for p in prompts)
    common = 0
    while common < shortest and all(p[common] == prompts[0][common] for p in prompts):
        common += 1
    return max(0, min(common, shortest - 1))


def suffix_capacity(remainder: int, max_new_tokens: int) -> int:
    """Slots of a ``share_prefix`` call's suffix caches: the longest remainder and the new tokens, in 64-key tiles."""
    return -(-(remainder + max(max_new_tokens, 1)) // 64) * 64


_fallback_logged = False


def log_fallback(why: str) -> None:
    """Once per process: an ``n`` call runs as the replicated call ``[prompt] * n``."""
    global _fallback_logged
    if _fallback_logged:
        return
    _fallback_logged = True
    log.info(f"n samples of one prompt run as the replicated batch ({why}): the same call by definition")


def log_batch_fallback(why: str) -> None:
    """Once per process: a ``share_prefix`` call runs as the plain call."""
    global _batch_fallback_logged
    if _batch_fallback_logged:
        return
    _batch_fallback_logged = True
    log.info(f"share_prefix runs as the plain batch ({why}): the same call by definition")


_batch_fallback_logged = False


def reference_prefill_attention(q: Tensor, kp: Tensor, vp: Tensor, ks: Tensor, vs: Tensor, prefix_len: int,
                                scale: float | None = None) -> Tensor:
    """The prefill form's definition, in fp64: q [R, Tq, H, D]; prefix caches [1, Hkv, capP, D], the first
    ``prefix_len`` slots used; suffix caches [R, Hkv, capS, D] with the call's K/V in slots 0..Tq-1 already.
    Query t of row r, head h: softmax over the prefix keys followed by row r's suffix slots 0..t.
    -> [R, Tq, H, D] fp64."""
    R, Tq, H, D = q.shape
    Hkv = kp.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    k = torch.cat([kp[:, :, :prefix_len].expand(R, -1, -1, -1), ks[:, :, :Tq]], dim=2).double()
    v = torch.cat([vp[:, :, :prefix_len].expand(R, -1, -1, -1), vs[:, :, :Tq]], dim=2).double()
    k = k.repeat_interleave(H // Hkv, dim=1)
    v = v.repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("rthd,rhkd->rhtk", q.double(), k) * scale
    key = torch.arange(prefix_len + Tq, device=q.device)
    hidden = key[None, :] > prefix_len + torch.arange(Tq, device=q.device)[:, None]
    s = s.masked_fill(hidden, float("-inf"))
    return torch.einsum("rhtk,rhkd->rthd", torch.softmax(s, dim=-1), v)


def reference_attention(q: Tensor, kp: Tensor, vp: Tensor, ks: Tensor, vs: Tensor, prefix_len: int,
                        suffix_len: int, scale: float | None = None) -> Tensor:
    """The definition, in fp64: q [R, H, D]; prefix caches [1, Hkv, capP, D], the first ``prefix_len`` slots
    used; suffix caches [R, Hkv, capS, D], the first ``suffix_len`` used (this step's K/V at slot
    ``suffix_len - 1`` already). Row r, head h: softmax over the prefix keys followed by row r's suffix keys of
    KV head h // (H / Hkv). -> [R, H, D] fp64."""
    R, H, D = q.shape
    Hkv = kp.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    k = torch.cat([kp[:, :, :prefix_len].expand(R, -1, -1, -1), ks[:, :, :suffix_len]], dim=2).double()
    v = torch.cat([vp[:, :, :prefix_len].expand(R, -1, -1, -1), vs[:, :, :suffix_len]], dim=2).double()
    k = k.repeat_interleave(H // Hkv, dim=1)
    v = v.repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("rhd,rhkd->rhk", q.double(), k) * scale
    return torch.einsum("rhk,rhkd->rhd", torch.softmax(s, dim=-1), v)


def _dequantize(x: Tensor, scale: Tensor) -> Tensor:
    return x.double() * scale.double()[..., None]


def _quantize_rows(x: Tensor) -> tuple[Tensor, Tensor]:
    """x [R, T, Hkv, D] -> (int8 [R, Hkv, T, D], fp32 scales [R, Hkv, T]): the cache's quantiser, on fp32 as the
    kernels compute it."""
    from penroz.ops.sampling import reference_quantize
    xq, s = reference_quantize(x.float().transpose(1, 2))
    return xq, s.squeeze(-1)


def reference_attention_q8(q: Tensor, k_new: Tensor, v_new: Tensor, prefix: tuple, suffix: tuple, prefix_len: int,
                           suffix_len: int, scale: float | None = None):
    """The int8 decode form's definition, in fp64: ``prefix`` = (kp, vp int8 [1, Hkv, capP, D], scales [1, Hkv,
    capP]), ``suffix`` = (ks, vs int8 [R, Hkv, capS, D], scales [R, Hkv, capS]) holding slots ``0..suffix_len - 2``;
    the step's bf16 ``k_new`` / ``v_new [R, Hkv, D]`` are quantised (``reference_quantize``) into slot
    ``suffix_len - 1``, everything is dequantised and ``reference_attention`` runs. The suffix caches are not
    written. -> ([R, H, D] fp64, (int8 K row, K scale, int8 V row, V scale) of the new slot)."""
    kp, vp, kps, vps = prefix
    ks, vs, kss, vss = suffix
    qk, sk = _quantize_rows(k_new.unsqueeze(1))
    qv, sv = _quantize_rows(v_new.unsqueeze(1))
    ksd, vsd = _dequantize(ks, kss), _dequantize(vs, vss)
    ksd[:, :, suffix_len - 1] = _dequantize(qk, sk)[:, :, 0]
    vsd[:, :, suffix_len - 1] = _dequantize(qv, sv)[:, :, 0]
    out = reference_attention(q, _dequantize(kp, kps), _dequantize(vp, vps), ksd, vsd, prefix_len, suffix_len, scale)
    return out, (qk[:, :, 0], sk[:, :, 0], qv[:, :, 0], sv[:, :, 0])


def reference_prefill_attention_q8(q: Tensor, k_new: Tensor, v_new: Tensor, prefix: tuple, suffix: tuple,
                                   prefix_len: int, scale: float | None = None):
    """The int8 prefill form's definition, in fp64: the rows' bf16 ``k_new`` / ``v_new [R, Tq, Hkv, D]`` are quantised
    into suffix slots ``0..Tq-1``, dequantised, and ``reference_prefill_attention`` runs over the dequantised prefix
    and those slots (``suffix`` gives the shapes; it is not written).
    -> ([R, Tq, H, D] fp64, (int8 K [R, Hkv, Tq, D], K scales [R, Hkv, Tq], int8 V, V scales))."""
    kp, vp, kps, vps = prefix
    qk, sk = _quantize_rows(k_new)
    qv, sv = _quantize_rows(v_new)
    out = reference_prefill_attention(q, _dequantize(kp, kps), _dequantize(vp, vps), _dequantize(qk, sk),
                                      _dequantize(qv, sv), prefix_len, scale)
    return out, (qk, sk, qv, sv)
