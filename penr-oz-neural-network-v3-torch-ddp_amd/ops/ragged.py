"""Ragged batches: prompts of different lengths generated in one call.

Definition. ``input_context`` is a non-empty list of non-empty lists of token ids in ``[0, V)``, row
``b`` of length ``len_b``; anything else raises ``ValueError`` before any forward pass (``/generate``
answers 400). Row ``b`` of a ragged call is the generation a one-row call would make from prompt ``b``
alone: its prompt sits at positions ``0 .. len_b - 1``, its generated token ``i`` at position
``len_b + i``, and that token's attention covers row ``b``'s own ``len_b + i`` keys and nothing else.
How the rows share a step is an implementation detail: padding must not influence any logit.
``min_tokens`` and the sampler's hash keep counting generated tokens — the same index for every row —
and ``stop_token`` keeps ``generate_batch``'s rule, by generated-token index: the call ends behind the
first generated column in which every row holds it.

A ragged call never slides its window: ``max(len_b) + max_new_tokens <= block_size`` is required. Rows
would reach the window at different steps, and the sliding-window re-prefill is a whole-batch
operation, so there is no re-prefill inside a ragged call.

A batch whose rows are all the same length is not ragged (``ragged_lengths`` returns None): it takes
the rectangular path exactly, with the same tensors, decoder, graphs and tokens.

GPU (``models/graph_decode.py``, ``GraphDecoder(ragged=True)``): prefill stays eager — the prompts are
right-padded to ``Lmax`` (``pad_prompts``) and run through the module forward once with the decoder's
cache attached; causality keeps the real tokens from seeing the pads behind them, and row ``b``'s first
token comes from the logits at position ``len_b - 1``. The K/V written for pad slots lie at or beyond
``len_b``: the captured step, which runs every row at its own position and cache length
(``StaticKVCache.pos_t`` / ``len_t`` are ``[rows]``), never reads them and overwrites them one by one.
The pad value is the row's own last prompt token, so the set of tokens "in the prompt" that the
repetition penalty sees is the true prompt's.

``reference_generate`` is the plain reference: the rows one at a time through the one-row path. It is
also what a ragged call runs wherever the ragged captured step does not apply (CPU,
``PENROZ_GRAPH_DECODE=0``, a model without a decode program — fp32 parameters and
``PENROZ_DECODE_PROGRAM=0`` included — or a row count the decoder does not take); that is logged once
per process.
"""
from __future__ import annotations

import logging

log = logging.getLogger(__name__)


def _is_row(row) -> bool:
    return isinstance(row, (list, tuple)) and not isinstance(row, (str, bytes))


def ragged_lengths(input_context) -> list[int] | None:
    """The rows' lengths when ``input_context`` is a list of lists whose lengths differ; None for
    everything the rectangular path takes (one flat row, equal lengths) or rejects itself."""
    if not _is_row(input_context) or len(input_context) < 2 or not all(_is_row(r) for r in input_context):
        return None
    lens = [len(r) for r in input_context]
    return lens if len(set(lens)) > 1 else None


def check_prompts(input_context, block_size: int, max_new_tokens: int, vocab: int | None = None) -> list[list[int]]:
    """``input_context`` as a list of lists of ints. ValueError unless it is a non-empty list of
    non-empty lists of token ids in [0, V) (V None: in [0, 2^31)) with
    ``max(len_b) + max_new_tokens <= block_size``."""
    if not _is_row(input_context) or len(input_context) == 0:
        raise ValueError("a batch of prompts must be a non-empty list of token id lists")
    hi = 2 ** 31 if vocab is None else int(vocab)
    out = []
    for b, row in enumerate(input_context):
        if not _is_row(row):
            raise ValueError(f"prompt {b} must be a list of token ids, got {type(row).__name__}")
        if len(row) == 0:
            raise ValueError(f"prompt {b} is empty: every row needs at least one token")
        ids = []
        for t in row:
            if isinstance(t, bool) or not isinstance(t, int):
                raise ValueError(f"prompt {b} must hold integer token ids, got {t!r}")
            if not 0 <= t < hi:
                raise ValueError(f"prompt {b}: token id {t} is outside [0, {hi})")
            ids.append(int(t))
        out.append(ids)
    lmax = max(len(r) for r in out)
    if lmax + int(max_new_tokens) > int(block_size):
        raise ValueError(f"a ragged batch does not slide its window: the longest prompt ({lmax}) + max_new_tokens "
                         f"({max_new_tokens}) must be <= block_size ({block_size})")
    return out


def pad_prompts(prompts: list[list[int]]) -> list[list[int]]:
    """The prompts right-padded to the longest, each row with its own last token (the repetition
    penalty's "in the prompt" set of a row is then its true prompt's)."""
    lmax = max(len(r) for r in prompts)
    return [list(r) + [r[-1]] * (lmax - len(r)) for r in prompts]


def assemble(prompts: list[list[int]], generated: list[list[int]]) -> list[list[int]]:
    """Per-row contexts: each row's own prompt followed by its generated tokens."""
    return [list(p) + list(g) for p, g in zip(prompts, generated)]


def reference_generate(model, prompts, block_size: int, max_new_tokens: int, temperature=1.0, top_k=None,
                       stop_token=None, **kwargs):
    """The definition in plain code: ``generate_batch`` of every row alone, assembled. Returns what
    ``generate_batch`` returns: the contexts, or ``(contexts, infos)`` with ``logprobs`` or ``stop``.
    ``stop_token`` follows ``generate_batch``'s rule — every row cut behind the first generated column
    in which all rows hold it — so the one-row calls run without it (and ``min_tokens`` then does not
    suppress it here)."""
    prompts = check_prompts(prompts, block_size, max_new_tokens, model._vocab_size())
    with_infos = kwargs.get("logprobs") is not None or bool(kwargs.get("stop"))
    contexts, infos = [], []
    for p in prompts:
        res = model.generate_batch([p], block_size, max_new_tokens, temperature, top_k, None, **kwargs)
        ctx, info = (res[0][0], res[1][0]) if with_infos else (res[0], {})
        contexts.append(ctx)
        infos.append(info)
    if stop_token is not None:
        gen = [c[len(p):] for c, p in zip(contexts, prompts)]
        n = min(len(g) for g in gen)
        hit = next((j for j in range(n) if all(g[j] == stop_token for g in gen)), None)
        if hit is not None:
            contexts = [c[:len(p) + hit + 1] for c, p in zip(contexts, prompts)]
            for info in infos:
                for key in ("token_logprobs", "top_logprobs"):
                    if key in info:
                        del info[key][hit + 1:]
    return (contexts, infos) if with_infos else contexts


_fallback_logged = False


def log_fallback(why: str) -> None:
    """Once per process: a ragged call runs its rows one at a time instead of the ragged captured step."""
    global _fallback_logged
    if _fallback_logged:
        return
    _fallback_logged = True
    log.info(f"ragged batch: rows generated one at a time ({why})")
