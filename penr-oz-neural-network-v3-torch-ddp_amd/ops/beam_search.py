"""Beam search: ``num_beams = W`` hypotheses of one prompt, kept and re-parented inside the decode step.

Options: ``num_beams`` W in 2..8 and ``length_penalty`` (finite, default 1.0); one prompt, ``max_new_tokens = T``.

State: W live beams, each with a cumulative log-probability ``c_b``; a history of (token, parent) per step and
beam slot; a finished list of at most W entries. Step t = 1..T runs over ``R_in`` rows of logits (1 at the first
step — the prompt pass's row, with ``c = [0]`` — W afterwards):

* ``l_b(v) = x_b[v] - logsumexp(x_b)`` over the bf16 logits the lm_head produced (ops/logprobs.py's definition;
  the kernel computes it in fp32 with a fixed reduction order, the reference here in fp64);
* the candidates are ``s(b, v) = c_b + l_b(v)``; the 2W best are taken under the total order (s descending, b
  ascending, v ascending) and walked in that order: a candidate with ``v == stop_token`` becomes a finished
  hypothesis — beam b's tokens plus v, scored ``s * inv_norm[t]`` — and any other one the next live beam in the
  next free slot, until W slots are filled. A beam has at most one stop candidate, so 2W candidates always suffice;
  without a ``stop_token`` nothing finishes;
* the finished list keeps the W best by (score descending, earlier step first, lower walk rank first);
* ``inv_norm[t] = fp32(t ** -length_penalty)``, computed here in fp64 and rounded once; t counts the generated
  tokens, the stop token included. The step reads it from a device table: another ``length_penalty`` replays the
  same graph and the kernel has no ``powf``.

All T steps run; there is no early stopping. The result is finished ∪ live hypotheses, the live ones scored
``c_b * inv_norm[T]``, sorted by score descending (a finished one in front of a live one of equal score); the W
best are returned, each ``{"tokens", "cum_logprob", "score", "finished"}`` with ``tokens`` the generated ones.

On the GPU (models/graph_decode.py, ``GraphDecoder(beam=W)``) the call is the shared-prefix step of an ``n`` call —
the prompt prefilled once into the batch-1 prefix cache, a suffix cache per beam — with the sampler replaced by
``beam_step`` and ``beam_reorder`` appended (csrc/kernels/beam_search.hip): the selection, the walk, the counter
advance and the re-parenting of the suffix caches all happen on the device, the bursts replay without a host
synchronisation, and the history, ``c`` and the finished list are read once at the end (``BeamState``). Elsewhere —
wherever an ``n`` call falls back — ``reference_generate`` runs over the module path on W replicated rows, the
plain cache reordered with ``index_select``; logged once per process.

A beam call is refused (``check_beams``) with more than one prompt, when ``len(prompt) + T > block_size`` (it never
slides its window: ``n``'s rule), with ``temperature != 1``, ``top_k``, ``top_p``, ``min_p``, penalties, logit bias /
banned / allowed ids / ``min_tokens``, ``stop``, ``logprobs``, ``prompt_logprobs``, ``speculate``, ``n``,
``share_prefix``, ``stream`` or a batch method.
"""
from __future__ import annotations

import logging
import math

import numpy as np
import torch
from torch import Tensor

from penroz.ops import _ext

log = logging.getLogger(__name__)

MIN_BEAMS, MAX_BEAMS = 2, 8
_CTL, _CUM, _PARENT, _FIN_F, _FIN_I, _HIST = 0, 8, 16, 24, 40, 72  # word offsets in BeamState.buf


def check_beams(num_beams, length_penalty=None, *, temperature=1.0, top_k=None, top_p=None, min_p=None,
                active=(), speculate=None, n=None, share_prefix=False, prompt_logprobs=False, rows: int | None = None,
                prompt_len: int | None = None, max_new_tokens: int | None = None, block_size: int | None = None,
                stream: bool = False, batch: bool = False) -> tuple[int, float] | None:
    """(W, length_penalty), or None for no beam search (``num_beams`` None). ``active``: the names of the call's
    other logit-rewriting / reporting options that are on. ValueError for what a beam call does not take."""
    if length_penalty is not None and (isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float))
                                       or not math.isfinite(length_penalty)):
        raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}")
    if num_beams is None:
        return None
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not MIN_BEAMS <= num_beams <= MAX_BEAMS:
        raise ValueError(f"num_beams must be None or an integer in [{MIN_BEAMS}, {MAX_BEAMS}], got {num_beams!r}")
    if batch:
        raise ValueError("beam search takes one prompt and returns its beams: use generate_tokens, not a batch")
    if stream:
        raise ValueError("beams are ranked when the call ends: not together with stream")
    if rows is not None and rows != 1:
        raise ValueError(f"beam search takes one prompt, got {rows} prompt rows")
    if float(temperature) != 1.0 or top_k is not None or (top_p is not None and top_p < 1.0) or (min_p is not None and min_p > 0.0):
        raise ValueError("beam search ranks exact log-probabilities: temperature must be 1 and top_k / top_p / min_p off")
    off = list(active) + [name for name, on in (("speculate", speculate), ("n", n), ("share_prefix", share_prefix),
                                                ("prompt_logprobs", prompt_logprobs)) if on]
    if off:
        raise ValueError(f"beam search does not compose with {', '.join(off)}")
    if None not in (prompt_len, max_new_tokens, block_size) and prompt_len + max_new_tokens > block_size:
        raise ValueError(f"a beam call does not slide its window: prompt ({prompt_len}) + max_new_tokens "
                         f"({max_new_tokens}) must be <= block_size ({block_size})")
    return int(num_beams), float(1.0 if length_penalty is None else length_penalty)


def inv_norm_table(steps: int, length_penalty: float) -> np.ndarray:
    """fp32 [steps + 1]: entry t is ``t ** -length_penalty`` (fp64, rounded once); entry 0 is unused."""
    with np.errstate(over="ignore"):
        return np.array([0.0] + [float(t) ** -float(length_penalty) for t in range(1, steps + 1)], dtype=np.float64).astype(np.float32)


def _insert_finished(fin: list, entry: tuple, W: int) -> None:
    """``fin`` stays sorted by (score descending, earlier entry first) and at most W long."""
    pos = len(fin)
    while pos > 0 and fin[pos - 1][0] < entry[0]:
        pos -= 1
    if pos < W:
        fin.insert(pos, entry)
        del fin[W:]


def reference_step(logits: Tensor, cum, W: int, t: int, stop_token: int | None, inv_norm: np.ndarray, finished: list):
    """Step t on ``logits`` [R_in, V] and the rows' ``cum`` (floats): fp64 log-softmax, the definition's order.
    -> (tokens [W], parents [W], cum [W], ranked): the next live beams and the 2W candidates walked, as
    (s, b, v) best first; ``finished`` gains this step's stop candidates as (score, s, t, parent, rank, token)."""
    x = logits.detach().double().cpu()
    s = torch.as_tensor(list(cum), dtype=torch.float64)[:, None] + torch.log_softmax(x, dim=-1)
    V = s.shape[1]
    order = torch.sort(s.flatten(), descending=True, stable=True)  # stable: ties stay (b, v) ascending
    ranked = [(float(sv), int(i) // V, int(i) % V) for sv, i in zip(order.values[:2 * W], order.indices[:2 * W])]
    tokens, parents, new_cum = [], [], []
    for rank, (sv, b, v) in enumerate(ranked):
        if stop_token is not None and v == stop_token:
            _insert_finished(finished, (sv * float(inv_norm[t]), sv, t, b, rank, v), W)
        elif len(tokens) < W:
            tokens.append(v), parents.append(b), new_cum.append(sv)
    return tokens, parents, new_cum, ranked


def backtrack(hist, t: int, slot: int) -> list[int]:
    """The tokens of the beam in ``slot`` after step t (1-based), from ``hist[step][slot] = (token, parent)``."""
    out = []
    for step in range(t - 1, -1, -1):
        tok, slot = hist[step][slot]
        out.append(int(tok))
    return out[::-1]


def assemble(hist, cum, finished, W: int, T: int, inv_norm) -> list[dict]:
    """finished ∪ live -> the W best, best first."""
    beams = [{"tokens": backtrack(hist, t - 1, b) + [int(v)], "cum_logprob": float(s), "score": float(score), "finished": True}
             for score, s, t, b, _, v in finished]
    beams += [{"tokens": backtrack(hist, T, j), "cum_logprob": float(cum[j]), "score": float(cum[j]) * float(inv_norm[T]),
               "finished": False} for j in range(W)]
    return sorted(beams, key=lambda e: -e["score"])[:W]  # (stable: finished first, then slot order, among equals)


def reference_generate(next_logits, W: int, T: int, stop_token: int | None = None, length_penalty: float = 1.0) -> list[dict]:
    """The definition as a loop. ``next_logits(tokens, parents)``: the logits [R, V] behind each live beam —
    ``tokens`` their generated tokens (``[[]]`` at the first step, for the prompt's one row), ``parents`` the slot
    each came from in the previous call (None at the first; a caller with a KV cache reorders it by them)."""
    inv_norm = inv_norm_table(T, length_penalty)
    hist, finished, cum, seqs, parents = [], [], [0.0], [[]], None
    for t in range(1, T + 1):
        tokens, parents, cum, _ = reference_step(next_logits(seqs, parents), cum, W, t, stop_token, inv_norm, finished)
        hist.append(list(zip(tokens, parents)))
        seqs = [seqs[b] + [v] for v, b in zip(tokens, parents)]
    return assemble(hist, cum, finished, W, T, inv_norm)


class BeamState:
    """The device buffers of a beam call of width W and at most ``steps_cap`` steps: one int32 buffer — control
    words [8] (step, T, R_in, stop token or -1, finished count, suffix slots, -, -), ``cum`` fp32 [8], ``parent``
    [8], the finished list (fp32 [W, 2] score and s; int32 [W, 4] step, parent, walk rank, token) and ``hist``
    [steps_cap, W, 2] — so a call's result is one read; the ``inv_norm`` table and the step's workspace beside it."""

    def __init__(self, W: int, steps_cap: int, V: int, device):
        self.W, self.steps_cap, self.V = int(W), int(steps_cap), int(V)
        _, ws = _ext.kernels().beam_step_plan(V, W)
        self.buf = torch.zeros(_HIST + 2 * W * steps_cap, dtype=torch.int32, device=device)
        f32 = lambda a, n: self.buf[a:a + n].view(torch.float32)
        self.ctl, self.cum, self.parent = self.buf[_CTL:_CTL + 8], f32(_CUM, 8), self.buf[_PARENT:_PARENT + 8]
        self.fin_f, self.fin_i, self.hist = f32(_FIN_F, 2 * W), self.buf[_FIN_I:_FIN_I + 4 * W], self.buf[_HIST:]
        self.slots = self.buf[5:6]  # suffix cache slots written so far: beam_reorder's length
        self.inv_norm = torch.zeros(steps_cap + 1, dtype=torch.float32, device=device)
        self.ws = torch.empty(W * ws, dtype=torch.float32, device=device)
        self.T, self._inv_host = 0, None

    def begin(self, T: int, stop_token: int | None, length_penalty: float, rows: int = 1, cum=None, step: int = 0):
        """A call's start: step 0 of T, ``rows`` input rows with ``cum`` (default: one row, c = 0)."""
        assert 1 <= T <= self.steps_cap and 1 <= rows <= self.W, (T, self.steps_cap, rows)
        head = np.zeros(_HIST, dtype=np.int32)
        head[:4] = (step, T, rows, -1 if stop_token is None else int(stop_token))
        if cum is not None:
            head[_CUM:_CUM + rows] = np.asarray(cum, dtype=np.float32).view(np.int32)
        self.buf[:_HIST].copy_(torch.from_numpy(head))
        self.T, self._inv_host = int(T), inv_norm_table(T, length_penalty)
        self.inv_norm[:T + 1].copy_(torch.from_numpy(self._inv_host))

    def step(self, logits: Tensor, idx: Tensor, advance: tuple | None = None) -> None:
        """One ``beam_step`` on ``logits`` [>= R_in, V]: the next tokens into ``idx`` (int64 [W] or [W, 1]).
        ``advance`` = (pos_t, len_t, step_t): a decode step's counters, advanced by one with the slot count."""
        _ext.kernels().beam_step(logits, self.ctl, self.cum, self.inv_norm, idx.view(-1), self.parent, self.hist,
                                 self.fin_f, self.fin_i, self.ws, self.W, self.steps_cap, *(advance or ()))

    def snapshot(self) -> Tensor:
        return self.buf[:_HIST + 2 * self.W * self.T].clone()

    def restore(self, snap: Tensor) -> None:
        self.buf[:snap.numel()].copy_(snap)

    def read(self) -> dict:
        """One copy to the host -> {"step", "finished": [(score, s, t, parent, rank, token)], "cum", "parent", "hist"}."""
        W, T = self.W, self.T
        host = self.buf[:_HIST + 2 * W * T].cpu().numpy()
        fl = host.view(np.float32)
        nf = int(host[4])
        fin = [(float(fl[_FIN_F + 2 * j]), float(fl[_FIN_F + 2 * j + 1]), *(int(e) for e in host[_FIN_I + 4 * j:_FIN_I + 4 * j + 4]))
               for j in range(nf)]
        return {"step": int(host[0]), "finished": fin, "cum": fl[_CUM:_CUM + W].tolist(),
                "parent": host[_PARENT:_PARENT + W].tolist(), "hist": host[_HIST:].reshape(T, W, 2).tolist()}

    def beams(self) -> list[dict]:
        got = self.read()
        assert got["step"] == self.T, (got["step"], self.T)
        return assemble(got["hist"], got["cum"], got["finished"], self.W, self.T, self._inv_host)


class ReorderTable:
    """``beam_reorder``'s layer table for these suffix caches (per layer [W, Hkv, cap, D] bf16); keeps them alive.
    With ``k_scales`` / ``v_scales`` (per layer fp32 [W, Hkv, cap]) the caches are the int8 KV cache's, and their
    scale planes are re-parented in the same launch."""

    def __init__(self, ks: list[Tensor], vs: list[Tensor], k_scales: list[Tensor] | None = None,
                 v_scales: list[Tensor] | None = None):
        self.caches = (list(ks), list(vs), list(k_scales or ()), list(v_scales or ()))
        scales = (list(k_scales), list(v_scales)) if k_scales is not None else ()
        self.host, self.workgroups = _ext.kernels().beam_reorder_table(list(ks), list(vs), *scales)
        self.dev = self.host.to(ks[0].device)

    def apply(self, parent: Tensor, n_t: Tensor) -> None:
        """Row r of every cache <- row ``parent[r]`` (int32 [W]) for slots [0, ``n_t[0]``) (int32 [1]), in place."""
        _ext.kernels().beam_reorder(self.host, self.dev, parent, n_t)


_fallback_logged = False


def log_fallback(why: str) -> None:
    """Once per process: a beam call runs ``reference_generate`` over the module path."""
    global _fallback_logged
    if _fallback_logged:
        return
    _fallback_logged = True
    log.info(f"beam search runs the reference loop on replicated rows ({why}): the same definition")
