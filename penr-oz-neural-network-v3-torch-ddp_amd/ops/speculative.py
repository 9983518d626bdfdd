"""Prompt-lookup speculative decoding for one greedy sequence: the definition, in plain Python.

A replayed decode step is bound by its launches, not by bytes, and rows 2-4 of its GEMVs are nearly free. A
speculative step guesses the next ``k`` tokens from the sequence's own history (``draft``), runs ``k + 1``
rows — consecutive positions of the one sequence — through one step, and keeps the longest prefix of the guess
that the model's own argmax confirms (``accept``). No second model; exact for greedy decoding: whatever the
drafts were, the tokens emitted are the plain greedy loop's (``reference_generate``).

``speculate: k`` with k in 1..3; None and 0 are off. Greedy, one row, no streaming and no option that rewrites
logits or reads them back (``check_speculate``); ``stop_token`` is allowed, the host cuts at its first
occurrence. ``len(prompt) + max_new_tokens + k <= block_size``: the step's last draft row needs a cache slot
and a position inside the window, and a speculative call never slides its window.

GPU (``models/graph_decode.py``, ``GraphDecoder(speculate=k)``): the step is the decode program on ``k + 1``
rows at positions ``n - 1 .. n - 1 + k`` of a batch-1 cache, the greedy sampler on those rows, and
``spec_advance`` (``csrc/kernels/spec_decode.hip``), which does on the device what ``advance`` does here.
Rejected drafts need no clean-up: their cache slots lie at or beyond the new ``n - 1`` and are rewritten by
the next step before the cache length covers them. Elsewhere (CPU, ``PENROZ_GRAPH_DECODE=0``, a model without
a decode program) the call runs the plain path, whose result is the same by definition; logged once.
"""
from __future__ import annotations

import logging

log = logging.getLogger(__name__)

MAX_K = 3       # a verify step has k + 1 <= 4 rows: the decode GEMVs' regime
MAX_NGRAM = 3   # the longest suffix the draft looks up

# the options a speculative call does not compose with, by the names the public methods give them
EXCLUDED = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logprobs", "stop", "logit_bias",
            "banned_token_ids", "allowed_token_ids", "min_tokens")


def draft(hist, k: int, max_ngram: int = MAX_NGRAM) -> list[int]:
    """The next ``k`` tokens guessed from ``hist`` (n >= 1 tokens) alone: for m = min(max_ngram, n - 1) down to
    1, the starts j in 0 .. n - m - 1 with hist[j:j+m] == hist[n-m:]; the first m with a match, its largest j;
    the draft is what followed that match, continued through the draft itself (a loop extends periodically).
    No match, or n == 1: k copies of the last token."""
    hist = list(hist)
    n = len(hist)
    if n < 1:
        raise ValueError("draft needs at least one token of history")
    for m in range(min(max_ngram, n - 1), 0, -1):
        tail = hist[n - m:]
        starts = [j for j in range(0, n - m) if hist[j:j + m] == tail]
        if starts:
            j, virt = starts[-1], list(hist)
            for i in range(k):
                virt.append(virt[j + m + i])
            return virt[n:]
    return [hist[n - 1]] * k


def accept(drafts, cand) -> int:
    """``cand[i]``: the model's argmax at row i (row 0 was fed the last known token, row i >= 1 ``drafts[i-1]``).
    Returns a, the number of leading i in 1..k with drafts[i-1] == cand[i-1]; the step emits cand[0..a]."""
    a = 0
    while a < len(drafts) and drafts[a] == cand[a]:
        a += 1
    return a


def advance(hist, drafts, cand, emitted: int, limit: int, capacity: int):
    """One step's bookkeeping, as ``spec_advance`` does it on the device: ``hist`` (a list, extended in place)
    gains ``min(a + 1, limit - emitted, capacity - k - n)`` tokens of ``cand`` — the last bound keeps the next
    step's draft rows inside the cache — and the result is ``(emitted tokens, drafts accepted among them)``;
    (0, 0) for a frozen step, which changes nothing."""
    k, n = len(drafts), len(hist)
    e = min(accept(drafts, cand) + 1, limit - emitted, capacity - k - n)
    if e <= 0:
        return 0, 0
    hist.extend(cand[:e])
    return e, e - 1


def reference_generate(next_token_fn, prompt, max_new: int, k: int, stats: dict | None = None,
                       max_ngram: int = MAX_NGRAM) -> list[int]:
    """The plain loop over ``draft`` and ``accept``: ``next_token_fn(tokens) -> token`` is the model's greedy
    choice behind ``tokens``. Returns prompt + max_new tokens — for any deterministic ``next_token_fn`` what the
    plain greedy loop returns. ``stats`` (a dict) receives {"steps", "drafted", "accepted"}."""
    hist = list(prompt)
    emitted = steps = accepted = 0
    while emitted < max_new:
        d = draft(hist, k, max_ngram)
        cand = [next_token_fn(hist + d[:i]) for i in range(k + 1)]
        e = min(accept(d, cand) + 1, max_new - emitted)
        hist.extend(cand[:e])
        emitted, steps, accepted = emitted + e, steps + 1, accepted + e - 1
    if stats is not None:
        stats.update(steps=steps, drafted=steps * k, accepted=accepted)
    return hist


def check_speculate(speculate, *, temperature: float, active=(), rows: int | None = None,
                    prompt_len: int | None = None, max_new_tokens: int | None = None, block_size: int | None = None,
                    stream: bool = False) -> int | None:
    """k in 1..3, or None for off (None, 0). ``active``: the names of the call's other options that are on
    (a neutral value is off); ``rows``, ``prompt_len``, ``block_size``, ``stream``: the call's shape where it is
    known. ValueError for what a speculative call does not take."""
    if speculate is None or (speculate == 0 and not isinstance(speculate, bool)):
        return None
    if isinstance(speculate, bool) or not isinstance(speculate, int) or not 1 <= speculate <= MAX_K:
        raise ValueError(f"speculate must be None, 0 or an integer in [1, {MAX_K}], got {speculate!r}")
    k = int(speculate)
    if temperature != 0:
        raise ValueError(f"speculate needs greedy decoding (temperature 0), got temperature {temperature}")
    for name in EXCLUDED:
        if name in active:
            raise ValueError(f"speculate does not compose with {name}")
    if stream:
        raise ValueError("speculate does not stream: a step emits up to k + 1 tokens at once")
    if rows is not None and rows != 1:
        raise ValueError(f"speculate takes one sequence, got {rows} rows")
    if None not in (prompt_len, max_new_tokens, block_size) and prompt_len + max_new_tokens + k > block_size:
        raise ValueError(f"a speculative call does not slide its window: prompt ({prompt_len}) + max_new_tokens "
                         f"({max_new_tokens}) + speculate ({k}) must be <= block_size ({block_size})")
    return k


_fallback_logged = False


def log_fallback(why: str) -> None:
    """Once per process: a speculative call runs the plain path (the same tokens by definition)."""
    global _fallback_logged
    if _fallback_logged:
        return
    _fallback_logged = True
    log.info(f"speculate: the call runs the plain decode path ({why})")
