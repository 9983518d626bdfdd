"""Stop sequences: lists of token ids that end a row's generation, checked where the tokens are made.

Definition. ``stop`` is a list of 1 to 16 sequences, each a list of 1 to 8 token ids in ``[0, V)``;
anything else raises ``ValueError`` before any forward pass (``/generate`` answers 400). ``None`` or
``[]`` means off. For row ``b`` let ``g_1 … g_t`` be the tokens generated in this call — the prompt
never takes part, so a match lies wholly inside the generated tokens. Row ``b`` finishes at the
smallest ``t`` such that some sequence ``s`` of length ``L <= t`` equals ``g_{t-L+1} … g_t``; if several
sequences end at that ``t``, the lowest index in ``stop`` is reported. The finishing token ``g_t`` is
kept: like ``stop_token``, the returned text includes the stop sequence. A finished row is frozen:
every later token of that row, in the next step's input and in the burst buffer, is overwritten with
``g_t`` (the other rows' steps stay fed with a valid id), and the row's state no longer changes. Rows
are independent: a row's tokens up to its finish are exactly what the same call without ``stop``
produces with the same seed. The call ends when every row has finished, or at ``max_new_tokens``.

GPU: ``csrc/kernels/stop_check.hip``. The stop set (``seqs`` int32 [16, 8], ``seq_len`` int32 [16],
``n_seqs`` int32 [1]) and the per-row state (``tail`` int32 [B, 8]: the last 8 generated tokens, -1
where there is none yet; ``n_gen``; ``done``: 0 running, else 1 + the index of the matching sequence;
``finish_at``: the ``t`` above; int32 [B] each) live on the device, so a captured decode graph replays
with another set, and the host reads ``done`` / ``finish_at`` once per burst, with the tokens.
"""
from __future__ import annotations

import torch
from torch import Tensor

from penroz.ops._ext import use_kernels, kernels

MAX_SEQS = 16
MAX_LEN = 8


def check_stop(stop, V: int | None = None) -> list[list[int]] | None:
    """``stop`` as a list of lists of ints, or None when it is off (None or empty). ValueError unless
    it is 1..16 sequences of 1..8 token ids, each in [0, V) (V None: in [0, 2^31))."""
    if stop is None:
        return None
    if isinstance(stop, (str, bytes)) or not isinstance(stop, (list, tuple)):
        raise ValueError(f"stop must be a list of token id sequences, got {type(stop).__name__}")
    if len(stop) == 0:
        return None
    if len(stop) > MAX_SEQS:
        raise ValueError(f"stop takes at most {MAX_SEQS} sequences, got {len(stop)}")
    hi = 2 ** 31 if V is None else int(V)
    out = []
    for i, seq in enumerate(stop):
        if isinstance(seq, (str, bytes)) or not isinstance(seq, (list, tuple)):
            raise ValueError(f"stop[{i}] must be a list of token ids, got {type(seq).__name__}")
        if not 1 <= len(seq) <= MAX_LEN:
            raise ValueError(f"stop[{i}] must hold 1 to {MAX_LEN} token ids, got {len(seq)}")
        ids = []
        for t in seq:
            if isinstance(t, bool) or not isinstance(t, int):
                raise ValueError(f"stop[{i}] must hold integer token ids, got {t!r}")
            if not 0 <= t < hi:
                raise ValueError(f"stop[{i}]: token id {t} is outside [0, {hi})")
            ids.append(int(t))
        out.append(ids)
    return out


def reference_stop(generated, stop) -> tuple[list[int], list[int]]:
    """generated [B, T] (tensor or nested lists) -> (finish_at [B], which [B]): the module docstring's
    definition in plain Python. A row that no sequence ends has 0 and -1."""
    rows = generated.tolist() if isinstance(generated, Tensor) else [list(r) for r in generated]
    seqs = check_stop(stop) or []
    finish_at, which = [], []
    for g in rows:
        at, idx = 0, -1
        for t in range(1, len(g) + 1):
            hit = [i for i, s in enumerate(seqs) if len(s) <= t and g[t - len(s):t] == s]
            if hit:
                at, idx = t, hit[0]
                break
        finish_at.append(at)
        which.append(idx)
    return finish_at, which


class StopState:
    """The stop sequences' per-row bookkeeping over one generate call.

    ``set_stop(seqs)`` → ``begin()`` once per call → every generated token passes once, in generation
    order, through ``observe(tok)`` (an eager step) or ``step(idx, out, step_t)`` (the captured step's
    last launch) → ``read()``. The buffers are allocated here, before any capture, and kept: a captured
    graph holds their addresses. On the GPU the kernels run; elsewhere the same state is kept in dense
    torch ops.
    """

    def __init__(self, rows: int, device):
        self.rows, self.device = int(rows), torch.device(device)
        self.stop: list[list[int]] = []
        i32 = dict(dtype=torch.int32, device=self.device)
        self.seqs = torch.zeros(MAX_SEQS, MAX_LEN, **i32)
        self.seq_len = torch.zeros(MAX_SEQS, **i32)
        self.n_seqs = torch.zeros(1, **i32)
        self.tail = torch.full((self.rows, MAX_LEN), -1, **i32)
        self.n_gen = torch.zeros(self.rows, **i32)
        self.done = torch.zeros(self.rows, **i32)
        self.finish_at = torch.zeros(self.rows, **i32)

    def _set(self):
        return self.seqs, self.seq_len, self.n_seqs

    def _state(self):
        return self.tail, self.n_gen, self.done, self.finish_at

    # ------------------------------------------------------------------ the stop set
    def set_stop(self, stop: list[list[int]] | None) -> None:
        """``check_stop``'s result (None: no sequence, nothing ever matches)."""
        self.stop = [list(s) for s in (stop or [])]
        assert len(self.stop) <= MAX_SEQS and all(1 <= len(s) <= MAX_LEN for s in self.stop), "check_stop comes first"
        seqs = torch.zeros(MAX_SEQS, MAX_LEN, dtype=torch.int32)
        lens = torch.zeros(MAX_SEQS, dtype=torch.int32)
        for i, s in enumerate(self.stop):
            seqs[i, :len(s)] = torch.tensor(s, dtype=torch.int32)
            lens[i] = len(s)
        self.seqs.copy_(seqs)
        self.seq_len.copy_(lens)
        self.n_seqs.fill_(len(self.stop))

    # ------------------------------------------------------------------ a call
    def begin(self) -> None:
        """Start a call: forget the previous one."""
        if use_kernels(self.tail):
            kernels().stop_begin(*self._state())
            return
        self.tail.fill_(-1)
        for t in (self.n_gen, self.done, self.finish_at):
            t.zero_()

    def observe(self, tok: Tensor) -> Tensor:
        """One generated token per row, ``tok`` int64 [B] or [B, 1], modified in place and returned:
        running rows are checked, rows that finished before get their finishing token."""
        assert tok.dtype == torch.long and tok.numel() == self.rows, (tok.dtype, tuple(tok.shape), self.rows)
        if use_kernels(self.tail):
            flat = tok if tok.is_contiguous() else tok.contiguous()
            kernels().stop_observe(*self._set(), *self._state(), flat)
            if flat is not tok:
                tok.copy_(flat)
            return tok
        self._observe_dense(tok.view(-1) if tok.is_contiguous() else tok.reshape(-1), tok)
        return tok

    def step(self, idx: Tensor, out: Tensor, step_t: Tensor) -> None:
        """The captured step's form, after the sampler and the counter advance: ``idx`` [B, 1] holds the
        tokens just chosen and column ``step_t - 1`` of ``out`` [B, cap] is this step's; both are
        rewritten for the rows that finished before. Launches one kernel, allocates nothing."""
        if use_kernels(self.tail):
            kernels().stop_step(*self._set(), *self._state(), idx, out, step_t)
            return
        self.observe(idx)
        out.index_copy_(1, (step_t - 1).to(out.device), idx.view(-1, 1))

    def _observe_dense(self, flat: Tensor, tok: Tensor) -> None:
        was_done = self.done != 0
        new = flat.to(device=self.device, dtype=torch.int32)
        frozen = self.tail[:, -1]
        shifted = torch.cat((self.tail[:, 1:], new.unsqueeze(1)), dim=1)
        n = self.n_gen + 1
        win = torch.full_like(self.done, MAX_SEQS)
        for s in range(len(self.stop) - 1, -1, -1):  # downwards: the lowest index is written last
            L = len(self.stop[s])
            hit = (shifted[:, MAX_LEN - L:] == self.seqs[s, :L]).all(dim=1) & (n >= L)
            win = torch.where(hit, torch.full_like(win, s), win)
        fin = ~was_done & (win < MAX_SEQS)
        run = ~was_done
        self.tail.copy_(torch.where(run.unsqueeze(1), shifted, self.tail))
        self.n_gen.copy_(torch.where(run, n, self.n_gen))
        self.done.copy_(torch.where(fin, win + 1, self.done))
        self.finish_at.copy_(torch.where(fin, n, self.finish_at))
        tok.copy_(torch.where(was_done, frozen, new).to(device=tok.device, dtype=tok.dtype).view(tok.shape))

    # ------------------------------------------------------------------ results
    def read(self, tokens: Tensor | None = None):
        """``(done, finish_at)`` as host lists of ints — or, with a block of ``tokens`` [B, k] (a burst's,
        on the state's device), ``(tokens, done, finish_at)`` from one copy to the host."""
        cols = [self.done.long().unsqueeze(1), self.finish_at.long().unsqueeze(1)]
        if tokens is None:
            both = torch.cat(cols, dim=1).tolist()
            return [r[0] for r in both], [r[1] for r in both]
        both = torch.cat(cols + [tokens.to(self.device)], dim=1).tolist()
        return [r[2:] for r in both], [r[0] for r in both], [r[1] for r in both]


class StopRun:
    """What a generate call hands ``_token_bursts`` about its stop sequences and gets back: ``seqs``
    (``check_stop``'s result) going in, ``state`` (the decoder's ``StopState``, or a fresh one) once the
    first burst is asked for."""

    def __init__(self, seqs: list[list[int]]):
        self.seqs = seqs
        self.state: StopState | None = None


def finish_info(done: int, produced: int, finish_at: int) -> tuple[int, dict]:
    """One row's (tokens kept, {"finish_reason", "stop_sequence"}) from its ``done`` / ``finish_at`` and
    the tokens the call produced."""
    if done:
        return finish_at, {"finish_reason": "stop", "stop_sequence": done - 1}
    return produced, {"finish_reason": "length", "stop_sequence": None}
