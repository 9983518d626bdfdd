"""What a generate call was asked for, checked once (``check_options`` -> ``DecodeOptions``), and the
state one call keeps while it runs (``DecodeCall``).

The public generate methods take their options as keywords; everything behind them — the token
loops of models/model.py, the captured step of models/graph_decode.py, ``/generate``'s early 400 —
takes the checked object. The checks themselves live with their features (ops/sampling.py,
ops/weight_quant.py, ops/penalties.py, ops/logprobs.py, ops/stopping.py, ops/logit_bias.py); this
module is the one place that calls them, in one order.
"""
from __future__ import annotations

import inspect
from dataclasses import dataclass, field

from torch import Tensor

from penroz.ops import logit_bias as bias_ops
from penroz.ops import logprobs as lp_ops
from penroz.ops import penalties as pen_ops
from penroz.ops import sampling as samp_ops
from penroz.ops import speculative as spec_ops
from penroz.ops import stopping as stop_ops
from penroz.ops import weight_quant as wq_ops


@dataclass(frozen=True)
class DecodeOptions:
    """The canonical form of a call's options; every neutral value (None, {}, [], 0, 1.0 / 0.0 / 0.0)
    gives the same object as leaving the option out. ``describe()`` speaks only for an object that
    ``check_options`` made: the log line names the values as they were given (a neutral penalty that was
    spelled out, say), which the canonical fields no longer show, so the checker keeps its wording in
    ``asked``, outside equality; an object built directly describes itself as ""."""
    temperature: float = 1.0
    top_k: int | None = None
    top_p: float | None = None
    min_p: float | None = None
    weight_quant: str | None = None  # as ``ops.weight_quant.resolve`` returned it
    penalties: tuple[float, float, float] | None = None  # ``check_penalties``' (repetition, presence, frequency)
    logprobs: int | None = None
    stop: list[list[int]] | None = None  # ``check_stop``'s
    stop_token: int | None = None
    bias: bias_ops.Canonical | None = None  # ``check_logit_bias``', with ``min_tokens`` folded into its entries
    min_tokens: int = 0
    speculate: int | None = None  # ``check_speculate``'s k in 1..3 (ops/speculative.py); None: off
    asked: str = field(default="", compare=False, repr=False)  # the options as given, in the words of the log line

    def describe(self) -> str:
        """What stands between "Generating at most N" and "tokens" in the generate call's log line."""
        return self.asked


NOT_LOADED = object()  # ``check_options``' V while the vocabulary is not known yet


def check_options(V: int | None, max_new_tokens: int, temperature: float, top_k: int | None,
                  stop_token: int | None = None, *, top_p: float | None = None, min_p: float | None = None,
                  weight_quant: str | None = None, repetition_penalty: float | None = None,
                  presence_penalty: float | None = None, frequency_penalty: float | None = None,
                  logprobs: int | None = None, stop: list | None = None, logit_bias: dict | None = None,
                  banned_token_ids: list | None = None, allowed_token_ids: list | None = None,
                  min_tokens: int | None = None, speculate: int | None = None,
                  call_shape: dict | None = None) -> DecodeOptions:
    """Every check of a generate call, once each, in this order; ValueError for the first that fails.
    ``call_shape`` is no option of the call: what the caller knows of its shape (``rows``, ``prompt_len``,
    ``block_size``, ``stream``), which ``speculate`` is checked against (ops/speculative.py).
    ``V``: the model's vocabulary size, which token ids are checked against. None: the model's layer list
    does not show one, and the options that rewrite logits by id are refused. ``NOT_LOADED`` (the service,
    before it loads the model): not known yet, ids are checked against 2^31 only."""
    loaded = V is not NOT_LOADED
    V = V if loaded else None
    samp_ops._check_filters(top_p, min_p)
    quant = wq_ops.resolve(weight_quant)
    penalties = pen_ops.check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
    n = lp_ops.check_logprobs(logprobs)
    seqs = stop_ops.check_stop(stop, V)
    if seqs is not None and stop_token is not None:
        raise ValueError("give stop_token or stop, not both (a stop_token s is the stop sequence [s])")
    bias = bias_ops.check_logit_bias(logit_bias, banned_token_ids, allowed_token_ids, min_tokens,
                                     bias_ops.end_tokens_of(stop_token, seqs), V, max_new_tokens, temperature)
    if bias is not None and V is None and loaded:
        raise ValueError("logit_bias / banned_token_ids / allowed_token_ids / min_tokens need a model whose "
                         "layer list ends with the vocabulary projection")
    active = [name for name, v, off in (("repetition_penalty", repetition_penalty, 1.0), ("presence_penalty", presence_penalty, 0.0),
                                        ("frequency_penalty", frequency_penalty, 0.0)) if v is not None and float(v) != off]
    active += [name for name, on in (("logprobs", n is not None), ("stop", seqs is not None), ("logit_bias", bool(logit_bias)),
                                     ("banned_token_ids", bool(banned_token_ids)), ("allowed_token_ids", allowed_token_ids is not None),
                                     ("min_tokens", bool(min_tokens))) if on]
    k = spec_ops.check_speculate(speculate, temperature=temperature, active=active, max_new_tokens=max_new_tokens,
                                 **(call_shape or {}))
    asked = "" if top_k is None else f" top {top_k}"
    asked += "" if top_p is None else f" top_p {top_p}"
    asked += "" if min_p is None else f" min_p {min_p}"
    for name, v in (("repetition", repetition_penalty), ("presence", presence_penalty), ("frequency", frequency_penalty)):
        asked += "" if v is None else f" {name}_penalty {v}"
    asked += "" if logprobs is None else f" logprobs {logprobs}"
    asked += "" if not stop else f" stop {len(stop)} sequences"
    if bias is not None:
        asked += f" logit bias {len(bias.ids)} entries"
        asked += "" if bias.allowed is None else f" {len(bias.allowed)} allowed ids"
        asked += "" if not min_tokens else f" min_tokens {min_tokens}"
    asked += "" if k is None else f" speculate {k}"
    return DecodeOptions(temperature, top_k, top_p, min_p, quant, penalties, n, seqs, stop_token, bias,
                         min_tokens or 0, k, asked)


# the option keywords of the public generate methods: ``check_options``' own, by name
KEYWORDS = tuple(name for name, p in inspect.signature(check_options).parameters.items()
                 if p.kind is p.KEYWORD_ONLY and name != "call_shape")


class DecodeCall:
    """One generate call's state: its ``PenaltyState`` / ``StopState`` / ``BiasState`` (None where the
    option is off), the log-probability count, and ``produced``, the tokens the call has made so far.

    With a ``decoder`` (models/graph_decode.py) the states are the decoder's, as its ``configure(opts)``
    made and loaded them, so the captured step and the eager steps of one call share them; without one
    they are made and loaded here. ``begin(context)`` once per call, then ``apply`` per eager step.
    """

    def __init__(self, opts: DecodeOptions, rows: int, device, decoder=None):
        self.opts, self.logprobs, self.produced = opts, opts.logprobs, 0
        self.penalties = self.stop = self.bias = None
        if decoder is not None:
            self.penalties = decoder.penalties if opts.penalties is not None else None
            self.stop = decoder.stop if opts.stop is not None else None
            self.bias = decoder.bias if opts.bias is not None else None
            return
        if opts.penalties is not None:
            self.penalties = pen_ops.PenaltyState()
            self.penalties.set_params(*opts.penalties)
        if opts.stop is not None:
            self.stop = stop_ops.StopState(rows, device)
            self.stop.set_stop(opts.stop)
        if opts.bias is not None:
            self.bias = bias_ops.BiasState(device)
            self.bias.set(opts.bias)

    def begin(self, context: Tensor) -> None:
        """Start the call: the penalties mark the whole prompt [rows, T], the stop check forgets the last call."""
        if self.penalties is not None:
            self.penalties.begin(context)
        if self.stop is not None:
            self.stop.begin()

    def apply(self, last: Tensor, penalty_new: Tensor | None):
        """An eager step from its logits ``last`` [rows, V] to its tokens [rows, 1], in the captured step's
        order: the penalties (which first count ``penalty_new`` [rows, 1], the tokens the previous step
        sampled; None on a call's first step), the logit bias with ``t = produced``, the sampler, the
        log-probabilities of the token as sampled, and the stop check, which gives a row that finished
        before its finishing token. With ``logprobs`` n: (tokens, ``ops.logprobs.token_logprobs``).
        Counts the token in ``produced``; a graph burst's tokens are the caller's to add."""
        if self.penalties is not None:
            last = self.penalties.apply(last.contiguous(), penalty_new)
        if self.bias is not None:
            last = self.bias.apply(last.contiguous(), self.produced)
        o = self.opts
        nxt = samp_ops.sample(last, o.temperature, o.top_k, top_p=o.top_p, min_p=o.min_p)
        lps = None if self.logprobs is None else lp_ops.token_logprobs(last, nxt, self.logprobs)
        if self.stop is not None:
            nxt = self.stop.observe(nxt)
        self.produced += 1
        return nxt if lps is None else (nxt, lps)
