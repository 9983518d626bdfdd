"""Graph-captured incremental decoding: one HIP graph replays a whole decode step.

The reference decodes one token per Python iteration through every layer module
(``neural_net_model.py:360-406, 457-514``) and grows its KV cache with ``torch.cat``. At
batch 64 on MI355X that per-token path is launch-bound: ~150 kernel launches plus Python
dispatch per token cost ~2.9 ms while the actual work (weights + cache read once) is ~0.2 ms.

Here the decode step — the model's forward, KV append, sampling, and the feedback of the sampled
token into the next step's input — is captured ONCE per (rows, block size, sampling settings) into
a ``torch.cuda.CUDAGraph`` (a hipGraph on ROCm) and replayed. For bf16 GPT-2-pattern and Gemma-family
models the forward is an explicit kernel sequence (``GPTDecodeProgram``, ``GemmaDecodeProgram``:
one loop over the blocks, the kernel of each linear chosen by the row count); any other model
replays its own module forward, whose numerics are the eager path's. Everything that changes
between steps lives on the device:

* ``StaticKVCache.pos_t`` / ``len_t``: the slot this step writes and the cache length after it;
  the decode-attention kernel reads q in place and ``len_t`` at run time, and appends this step's
  K/V (read in place from the fused QKV rows, int8-quantised for TurboQuant) at slot
  ``len_t - 1 = pos_t`` itself (``csrc/kernels/decode_attn.hip``: ``k_new``, ``seq_len_dev``);
* ``PositionEmbedding.position_offset_tensor``: the learned position gathered at ``pos_t``;
* the sampler hashes its uniforms on the device from (seed of the generate call, absolute token
  index, row) and writes the token straight into the next step's input and the burst output
  buffer; one tiny kernel then advances the position / length / step counters. Streaming and
  non-streaming calls therefore draw identical tokens under the same ``torch.manual_seed``;
* the step's ``nn.Linear`` GEMMs (M = rows ≤ 64) run on the decode-shaped MFMA kernel
  (``csrc/kernels/skinny_gemm.hip``): called explicitly by the decode programs, or — for the
  module-forward fallback — through ``ops/gemm.py: decode_gemms(model)``, which re-routes only
  that model's own ``nn.Linear`` instances for the capture.
* with ``weight_quant="int8"`` the decode programs' batch 1-4 step reads int8 copies of every
  linear's weight (``ops/weight_quant.py``, ``csrc/kernels/decode_gemv_q8.hip``), built per weight
  version before the warm-up step; ``GraphDecoder.weight_quant`` records whether that is in effect.
* repetition / presence / frequency penalties (``ops/penalties.py``, ``csrc/kernels/logit_penalty.hip``)
  act on the logits between the lm_head and the sampler, from count tables the decoder owns; their
  values are read from the device. The step with that kernel and the step without it are two graphs
  of one decoder (``GraphDecoder.configure``, ``StepMode``): same KV cache, same program.
* per-token log-probabilities (``ops/logprobs.py``, ``csrc/kernels/token_logprobs.hip``) are computed
  behind the sampler from the logits it read and the token it wrote, into burst buffers the decoder
  owns; ``n`` is read from the device. With them the step is another graph of the same decoder: by
  (penalised, log-probabilities on).
* stop sequences (``ops/stopping.py``, ``csrc/kernels/stop_check.hip``) are checked by the step's last
  kernel against the token just chosen: per-row finish state on the device, finished rows frozen on
  their finishing token in the next step's input and the burst buffer. The stop set is read from the
  device; the step with the check is a further graph of the decoder: up to eight, by (penalised,
  log-probabilities on, stop check on).
* logit bias, banned and allowed tokens and ``min_tokens`` (``ops/logit_bias.py``,
  ``csrc/kernels/logit_bias.hip``) rewrite the logits behind the penalties, in front of the sampler and
  the log-probabilities, in one launch that reads its entries, its mask and ``t`` from the device. The
  graph mode gains a fourth element: off, entries, or entries + mask —
  the last two differ in their grid, so they are separate graphs.

* ragged batches (``ops/ragged.py``): a ``GraphDecoder`` with ``ragged=True`` keeps ``pos_t`` / ``len_t`` as
  ``[rows]`` — every row's own slot and cache length. The decode-attention kernel's workgroups read their
  batch row's entry (key range, split count, in-launch merge and append slot per row), the embedding
  gathers each row's own position, the RoPE table is ``[rows, D/2]`` (Gemma then runs the plain QKV linear
  and the separate RoPE pass over the rows viewed as ``[1, rows, W]``: the QKV epilogues take one
  position's table), and the sampler's fused advance adds 1 to every row's two entries: the same number
  of launches as the uniform step for GPT, one more per block for Gemma where the uniform step rotates in
  the QKV epilogue. The host tracks the longest row for the capacity check; the prompt lengths come from
  ``set_lengths`` once per call. Graph modes and their lazily captured graphs are as above.

* speculative decoding (``ops/speculative.py``, ``csrc/kernels/spec_decode.hip``): a ``GraphDecoder`` with
  ``speculate=k`` runs ``k + 1`` rows — consecutive positions of ONE greedy sequence — against a batch-1 cache:
  ``pos_t`` is ``[k + 1]``, ``len_t`` ``[1]``. The program runs as for a ragged step (per-row positions in the
  embedding and the RoPE table); ``_attend_graph`` appends the rows' K/V into the one cache (``kv_append``'s
  shared-cache form) and attends with ``Tq = k + 1``, row i over its own ``n + i`` keys; the greedy sampler
  chooses per row and ``spec_advance`` accepts the confirmed drafts, keeps the history and drafts the next
  step's rows, all on the device. ``run_speculative`` replays bursts of steps without a host synchronisation
  per step and reads the history's new part once per burst.

The host only tracks the cache length (one per replay) to switch to the reference's
sliding-window re-prefill when the window is full, and copies each burst of tokens back once
(stop-token checks per burst). Prefill and re-prefill run eagerly. RoPE models (Gemma) rotate
with a cos/sin table computed on the device from ``pos_t`` once per step
(``_GraphMode.rope_table``); their head_dim 256 runs on the same decode-attention kernel.
"""
from __future__ import annotations

import gc
import logging
import os
import weakref
from typing import NamedTuple

import torch
from torch import Tensor

from penroz.models import kv_cache as kvc
from penroz.ops import _ext
from penroz.ops import activations as act_ops
from penroz.ops import attention as attn_ops
from penroz.ops import fused as fused_ops
from penroz.ops import gemm as gemm_ops
from penroz.ops import logit_bias as bias_ops
from penroz.ops import logprobs as lp_ops
from penroz.ops import norms as norm_ops
from penroz.ops import penalties as pen_ops
from penroz.ops import rope as rope_ops
from penroz.ops import sampling as samp_ops
from penroz.ops import stopping as stop_ops
from penroz.ops import weight_quant as wq_ops

log = logging.getLogger(__name__)

GRAPH_DECODE = os.environ.get("PENROZ_GRAPH_DECODE", "1") != "0"
# GPT-2-pattern bf16 models: the captured step is the explicit program below instead of the
# module forward ("0": module forward, numerically identical to the eager decode path)
DECODE_PROGRAM = os.environ.get("PENROZ_DECODE_PROGRAM", "1") != "0"
# the decode-attention kernel appends the step's K/V itself (one kernel less per layer); "0":
# separate kv_append kernel
FUSED_APPEND = os.environ.get("PENROZ_FUSED_APPEND", "1") != "0"
# decode rows up to which the linears use the decode-shaped MFMA kernel instead of hipBLASLt
# (measured: a win at batch 1, none at batch 64 — profiles/bench_r1_decode_graph.log)
SKINNY_MAX_ROWS = int(os.environ.get("PENROZ_SKINNY_MAX_ROWS", "16"))
# Gemma program: RoPE and the gated activation in the skinny GEMM epilogues ("1", default) or the
# separate RoPE / packed-activation kernels after plain skinny GEMMs ("0": same-box A/B switch)
DECODE_EPILOGUES = os.environ.get("PENROZ_DECODE_EPILOGUES", "1") != "0"
# GPT decode program: residual add + LayerNorm fused in front of the QKV and fc GEMMs (and GELU
# behind fc) in one decode-shaped kernel (csrc/kernels/skinny_gemm.hip decode_ln_linear); "0":
# separate add+LN, GEMM and GELU kernels
FUSED_LN_LINEAR = os.environ.get("PENROZ_DECODE_FUSED", "1") != "0"
# ... up to this many decode rows: every workgroup normalises all rows itself, which pays off
# while the rows are few (batch 1 / 4 / 8: -8 / -10 / -3 %) and loses from 16 rows on (+14 % at 16,
# +69 % at 64): profiles/decode_fused_rows_r2.log
FUSED_MAX_ROWS = int(os.environ.get("PENROZ_DECODE_FUSED_MAX_ROWS", "8"))
# ... above that: the batched block (csrc/kernels/decode_linear.hip) — 5 kernels per block, the
# fp32 residual updated in place by the proj / fc2 epilogues, LayerNorm recomputed per 16-row
# block inside the QKV / fc GEMMs; "0": add+LN, GEMM, GELU kernels (8 per block)
BATCHED_BLOCK = os.environ.get("PENROZ_DECODE_BATCHED", "1") != "0"
# ... and up to this many rows (batch 1-4) every linear of the GPT block — the LN-fused QKV and
# fc(+GELU), proj, fc2 and the lm_head — runs as the one-wave-per-workgroup decode GEMV
# (csrc/kernels/decode_linear.hip decode_gemv: one memory round trip, no LDS, no barrier, no
# split-K hand-off); "0": decode_ln_linear + skinny GEMMs
GEMV_MAX_ROWS = int(os.environ.get("PENROZ_DECODE_GEMV_MAX_ROWS", "4"))
# the sampler's last row advances the step counters itself (sample_step with adv_a / adv_b / done:
# one launch less per token); "0": the separate decode_advance kernel
FUSED_ADVANCE = os.environ.get("PENROZ_DECODE_FUSED_ADVANCE", "1") != "0"


def _gemv_limits():
    """(rows, K, LN-mode K, paired-row K) the decode GEMV launchers accept at most: their own
    limits (csrc/kernels/host_plan.h), read here instead of repeated; wider linears take the
    skinny GEMM. Needs the built extension (callers ask ``_ext.available()`` first)."""
    return _ext.kernels().decode_gemv_limits()


def _gemv_q8_limits():
    """(rows, K, LN-mode K, paired-row K, K multiple) of the int8-weight decode GEMV launchers
    (decode_gemv_q8 / decode_gemv_q8_pair), their own constants as well."""
    return _ext.kernels().decode_gemv_q8_limits()


class _GraphMode:
    """Mixin: ``attend`` switches to device-positioned append + attention while capturing."""

    graph_mode = False

    shared = False

    def init_graph_state(self, device, rows: int | None = None, shared: bool = False):
        """``rows``: a ragged decoder's row count — one slot and one length per row instead of one.
        ``shared`` (a speculative decoder): the rows are positions of one sequence in a batch-1 cache — a slot
        per row, one length; the program takes its per-row positions as from a ragged cache."""
        self.ragged = rows is not None
        self.shared = bool(shared)
        assert self.ragged or not self.shared
        n = rows if self.ragged else 1
        self.pos_t = torch.zeros(n, dtype=torch.long, device=device)  # slot written by the step
        self.len_t = torch.ones(1 if self.shared else n, dtype=torch.long, device=device)   # cache length after it
        self._rope_tables: dict = {}

    def begin_step(self):
        self._rope_tables.clear()

    def rope_table(self, key, inv_freq: Tensor, T: int):
        """cos / sin for positions pos_t..pos_t+T-1, computed on the device once per step and
        ``key`` = (theta, head_dim): layers with the same rotary setup share it. Ragged (T == 1):
        [rows, D/2], every row at its own position."""
        key = (*key, T)
        tab = self._rope_tables.get(key)
        if tab is None:
            tab = self._rope_tables[key] = rope_ops.rope_table(inv_freq, 0, T, inv_freq.device, offset_dev=self.pos_t)
        return tab

    def attend(self, layer_idx: int, q: Tensor, k: Tensor, v: Tensor) -> Tensor:
        if not self.graph_mode:
            return super().attend(layer_idx, q, k, v)
        return self._attend_graph(layer_idx, q, k, v)


class StaticKVCache(_GraphMode, kvc.KVCache):
    def _attend_graph(self, l: int, q: Tensor, k: Tensor, v: Tensor) -> Tensor:
        # k, v, q are views into this layer's fused QKV rows: one kernel appends K/V at pos_t,
        # the decode kernel reads q in place and the cache length from len_t
        kc, vc = self._k[l], self._v[l]
        if self.shared:  # the rows' K/V into the one cache at pos_t [R], then Tq = R queries over len_t [1] keys
            _ext.kernels().kv_append(k, v, kc, vc, None, None, self.pos_t, 0)
            return attn_ops.decode_attention(_as_one_sequence(q), kc, vc, kc.shape[2], seq_len_dev=self.len_t)
        if FUSED_APPEND:
            return attn_ops.decode_attention(q, kc, vc, kc.shape[2], seq_len_dev=self.len_t, k_new=k, v_new=v)
        _ext.kernels().kv_append(k, v, kc, vc, None, None, self.pos_t, 0)
        return attn_ops.decode_attention(q, kc, vc, kc.shape[2], seq_len_dev=self.len_t)

    def rope_attend_ok(self, B: int, H: int, Hkv: int, D: int) -> bool:
        """``attend_rope`` applies: opted in (PENROZ_DECODE_ROPE_IN_ATTN=1), graph mode with the
        fused append, the small decode kernel. Off by default: Gemma-3 1B batch 32 / 64 measured
        2.108 / 2.100 and 2.442 / 2.445 ms/step with it vs 2.074 / 2.077 and 2.425 / 2.433 ms with
        the separate RoPE pass (profiles/negative_r6_rope_in_decode_attn.log)."""
        kc = self._k[0]
        return (os.environ.get("PENROZ_DECODE_ROPE_IN_ATTN", "0") == "1" and self.graph_mode and FUSED_APPEND
                and not self.ragged and _ext.available()  # (the in-kernel rotation takes one position)
                and attn_ops.decode_rope_fusable(B, H, Hkv, D, kc.shape[2], kc.dtype))

    def attend_rope(self, l: int, q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor) -> Tensor:
        """``attend`` with q / k unrotated: the decode kernel applies RoPE (cos / sin [1, D/2]) to
        q and to the key it appends, in place of a separate RoPE pass over the QKV rows."""
        kc, vc = self._k[l], self._v[l]
        return attn_ops.decode_attention(q, kc, vc, kc.shape[2], seq_len_dev=self.len_t, k_new=k, v_new=v,
                                         rope=(cos.view(-1), sin.view(-1)))


class StaticTurboKVCache(_GraphMode, kvc.TurboQuantKVCache):
    def _attend_graph(self, l: int, q: Tensor, k: Tensor, v: Tensor) -> Tensor:
        # same per-token int8 quantiser as the eager append (kv_quantize)
        self._dtype[l] = k.dtype
        if self.shared:
            _ext.kernels().kv_append(k, v, self._k[l], self._v[l], self._sk[l], self._sv[l], self.pos_t, 0)
            return attn_ops.decode_attention(_as_one_sequence(q), self._k[l], self._v[l], self._k[l].shape[2],
                                             self._sk[l], self._sv[l], seq_len_dev=self.len_t)
        if FUSED_APPEND:
            return attn_ops.decode_attention(q, self._k[l], self._v[l], self._k[l].shape[2], self._sk[l],
                                             self._sv[l], seq_len_dev=self.len_t, k_new=k, v_new=v)
        _ext.kernels().kv_append(k, v, self._k[l], self._v[l], self._sk[l], self._sv[l], self.pos_t, 0)
        return attn_ops.decode_attention(q, self._k[l], self._v[l], self._k[l].shape[2], self._sk[l], self._sv[l],
                                         seq_len_dev=self.len_t)


def _qkv_views(qkv: Tensor, H: int, Hkv: int, D: int):
    """q [rows, 1, H, D], k and v [rows, 1, Hkv, D] as views into the fused QKV rows."""
    rows = qkv.shape[0]
    q, k, v = qkv.view(rows, 1, -1).split([H * D, Hkv * D, Hkv * D], dim=2)
    return q.reshape(rows, 1, H, D), k.view(rows, 1, Hkv, D), v.view(rows, 1, Hkv, D)


def _as_one_sequence(q: Tensor) -> Tensor:
    """q [rows, 1, H, D] (a view into the fused QKV rows) as [1, rows, H, D]: the rows as consecutive queries
    of one sequence, still read in place."""
    return q.squeeze(1).unsqueeze(0)


class _PlainSteps:
    """The GPT block's steps on separate kernels: [add-residual + bias + LN] → GEMM+bias (→ GELU),
    8 per block (9 with the separate KV append). Owns the fp32 residual stream, as every regime
    does: ``x`` is the sum up to the last norm; proj and fc2 leave their output and fp32 bias
    pending in ``delta`` / ``dbias``, and the next norm's kernel adds them, writing the new sum to
    the other buffer ``x2`` (the stream ping-pongs, no aliasing)."""

    def __init__(self, prog, x: Tensor, x2: Tensor | None = None, emb=None):
        self.prog, self.x, self.x2, self.emb = prog, x, x2, emb
        self.delta = self.dbias = None
        self._live = (None, None)
        self.act = 2 if prog.spec.gelu_approx == "tanh" else 1

    def _take(self):
        """(resid_in, delta, dbias, resid_out) for the next norm's kernel; the sum it writes is the
        residual from here on."""
        if self.delta is None:
            return self.x, None, None, None
        args = (self.x, self.delta, self.dbias, self.x2)
        self.x, self.x2, self.delta, self.dbias = self.x2, self.x, None, None
        return args

    def norm_linear(self, ln, lin, gelu: bool = False) -> Tensor:
        x, delta, dbias, out = self._take()
        if delta is None:
            y, _, _ = norm_ops.ln_fwd(x, *ln)
        else:
            y, _, _ = norm_ops.add_ln_fwd(x, delta, out, *ln, delta_bias=dbias)
        h = self.prog._linear(y, lin)
        return act_ops.gelu_fwd(h, self.prog.spec.gelu_approx, out=h) if gelu else h

    def _defer(self, delta: Tensor, fbias: Tensor) -> None:
        """proj's or fc2's output and the fp32 copy of its bias (GPTDecodeProgram.out_bias), left
        for the next norm's kernel to add. The output before it stays referenced too: each lives
        until its successor of the next block exists, so a capture's allocator alternates two
        buffers for proj and two for fc2 and never hands fc2 the block proj just used (buffer
        placement shows in the replayed step's time: batch 64 ran 0.7 % slower with fc's output
        freed one step earlier)."""
        self.delta, self.dbias = delta, fbias
        self._live = (self._live[1], delta)

    def project(self, h: Tensor, lin, fbias: Tensor) -> None:
        self._defer(self.prog._linear(h, lin, bias=False), fbias)

    def head(self, ln, lin) -> Tensor:
        return _PlainSteps.norm_linear(self, ln, lin)


class _FusedSteps(_PlainSteps):
    """Up to FUSED_MAX_ROWS rows, per block: [add + LN1 + QKV GEMM + bias] → decode attention (K/V
    append fused) → proj GEMM → [add + proj bias + LN2 + fc GEMM + bias + GELU] → fc2 GEMM: 5 kernels
    instead of 8. The final add + LN and the lm_head stay separate kernels."""

    def norm_linear(self, ln, lin, gelu: bool = False) -> Tensor:
        x, delta, dbias, out = self._take()
        return gemm_ops.decode_ln_linear(x, ln, lin.weight, lin.bias, self.act if gelu else 0, delta=delta,
                                         dbias=dbias, resid_out=out)


class _GemvSteps(_PlainSteps):
    """Batch 1-4, per block: [add + LN1 + QKV GEMV + bias] → decode attention (K/V append fused)
    → proj GEMV → [add + proj bias + LN2 + fc GEMV + bias + GELU] → fc2 GEMV; then the final
    add + LN and the lm_head GEMV — every linear one decode_gemv launch. ``emb`` = (token ids,
    device position): the first GEMV builds the residual rows wte[tok] + wpe[pos] itself and
    writes them to ``x`` (one kernel less per token)."""

    def norm_linear(self, ln, lin, gelu: bool = False) -> Tensor:
        act = self.act if gelu else 0
        if self.emb is not None:
            (idx, pos), self.emb, sp = self.emb, None, self.prog.spec
            return gemm_ops.decode_gemv_emb(idx, pos, sp.wte.weight, sp.wpe.weight, self.x, ln, lin.weight,
                                            lin.bias, act)
        x, delta, dbias, out = self._take()
        return gemm_ops.decode_gemv_ln(x, ln, lin.weight, lin.bias, act, delta=delta, dbias=dbias, resid_out=out)

    def project(self, h: Tensor, lin, fbias: Tensor) -> None:
        self._defer(gemm_ops.decode_gemv(h, lin.weight), fbias)

    head = norm_linear


class _GemvQ8Steps(_PlainSteps):
    """``_GemvSteps`` on the int8 weight copies (``GPTDecodeProgram.q8``): the same five launches per
    block, each reading half the weight bytes. The embedding stays its own kernel (the int8 GEMV has
    no gather prologue)."""

    def norm_linear(self, ln, lin, gelu: bool = False) -> Tensor:
        x, delta, dbias, out = self._take()
        return gemm_ops.decode_gemv_q8_ln(x, ln, self.prog.q8[id(lin)], lin.bias, self.act if gelu else 0,
                                          delta=delta, dbias=dbias, resid_out=out)

    def project(self, h: Tensor, lin, fbias: Tensor) -> None:
        self._defer(gemm_ops.decode_gemv_q8(h, self.prog.q8[id(lin)]), fbias)

    head = norm_linear


class _BatchedSteps(_PlainSteps):
    """Above FUSED_MAX_ROWS rows, per block: [LN1 + QKV GEMM + bias] → decode attention (K/V append
    fused) → [proj GEMM + bias, added into the fp32 residual in place] → [LN2 + fc GEMM + bias +
    GELU] → [fc2 GEMM + bias, added into the residual]: 5 kernels instead of 8. Nothing is ever
    pending, so there is no second residual buffer and the last norm is a plain LN."""

    def norm_linear(self, ln, lin, gelu: bool = False) -> Tensor:
        return gemm_ops.decode_ln_gemm(self.x, ln, lin.weight, lin.bias, self.act if gelu else 0)

    def project(self, h: Tensor, lin, fbias: Tensor) -> None:
        _ext.kernels().decode_gemm_acc(h, lin.weight, lin.bias, self.x)


class GPTDecodeProgram:
    """One decode step of a GPT-2-pattern bf16 model as an explicit kernel sequence.

    The module forward costs ~12 kernels per block at decode shapes (residual adds and dtype
    glue included) and every kernel has a fixed ~4-5 µs cost in a replayed graph at batch 64 —
    more than most of them compute. ``forward`` is one loop over the blocks: norm + QKV linear →
    decode attention (K/V append fused) → proj into the residual → norm + fc linear + GELU → fc2
    into the residual, then the final norm + lm_head. Which kernels run those steps depends on the
    row count (``_GemvSteps`` / ``_FusedSteps`` / ``_BatchedSteps``: 5 per block, ``_PlainSteps``:
    8). The residual stream is kept in fp32 (the training executor's numerics; the module path
    rounds it to bf16 after every add). The embedding reads the position from the device.
    """

    def __init__(self, model, spec):
        self.spec = spec
        dev = spec.wte.weight.device
        # LayerNorm kernels take fp32 affine parameters
        self.ln = [((b.ln1.weight.float(), b.ln1.bias.float(), b.ln1.eps),
                    (b.ln2.weight.float(), b.ln2.bias.float(), b.ln2.eps)) for b in spec.blocks]
        self.lnf = (spec.lnf.weight.float(), spec.lnf.bias.float(), spec.lnf.eps)
        # proj / fc2 biases are added by the following add+LN kernel (fp32), so those two GEMMs
        # run without a bias epilogue (hipBLASLt's pick for fc2 at M = 64 has none: torch then
        # launches an extra bias-broadcast copy per call)
        self.out_bias = [(b.proj.bias.float(), b.fc2.bias.float()) for b in spec.blocks]
        self.device = dev
        self.q8: dict | None = None  # id(linear) -> (q, scale) once enable_q8 admitted the step

    @staticmethod
    def build(model):
        if not DECODE_PROGRAM:
            return None
        from penroz.models.executor import GPTExecutor
        spec = GPTExecutor.match(model)
        if spec is None or any(p.dtype != torch.bfloat16 for p in model.parameters()):
            return None
        return GPTDecodeProgram(model, spec)

    def _linear(self, x: Tensor, lin, bias: bool = True) -> Tensor:
        b = lin.bias if bias else None
        if x.shape[0] <= SKINNY_MAX_ROWS and gemm_ops.skinny_ok(x, lin.weight):
            return gemm_ops.skinny_linear(x, lin.weight, b)
        if b is not None:
            return torch.addmm(b, x, lin.weight.t())
        return torch.mm(x, lin.weight.t())

    def _gemv_ok(self, rows: int) -> bool:
        if not _ext.available():
            return False
        sp = self.spec
        max_rows, _, max_ln_k, _ = _gemv_limits()  # the QKV / fc GEMVs run in LN mode
        return (1 <= rows <= min(max_rows, GEMV_MAX_ROWS) and sp.C % 8 == 0 and sp.C <= max_ln_k
                and sp.blocks[0].fc.out_features % 8 == 0 and sp.gelu_approx in ("none", "tanh"))

    def _linears(self):
        sp = self.spec
        return [lin for b in sp.blocks for lin in (b.qkv, b.proj, b.fc, b.fc2)] + [sp.head]

    def enable_q8(self, rows: int) -> bool:
        """Int8 weights for this row count: admitted when the step runs the decode GEMVs and every
        linear's K fits the int8 kernel (a multiple of its chunk, within its limits) — all of the
        step or none of it. Builds (or finds) the quantised copies now, outside any capture."""
        if not self._gemv_ok(rows):
            return False
        max_rows, max_k, max_ln_k, _, k_mult = _gemv_q8_limits()
        sp = self.spec
        for b in sp.blocks:  # qkv / fc (and the head) in LN mode on K = C; proj / fc2 plain
            if (b.qkv.in_features != sp.C or b.fc.in_features != sp.C or b.proj.in_features > max_k
                    or b.fc2.in_features > max_k or b.proj.in_features % k_mult or b.fc2.in_features % k_mult):
                return False
        if rows > max_rows or sp.C % k_mult or sp.C > max_ln_k or sp.head.in_features != sp.C:
            return False
        self.q8 = {id(lin): wq_ops.linear_q8(lin) for lin in self._linears()}
        return True

    def _fused_ok(self, rows: int) -> bool:
        sp = self.spec
        return (FUSED_LN_LINEAR and 1 <= rows <= min(64, FUSED_MAX_ROWS) and sp.C % 32 == 0 and sp.C <= 1024
                and sp.gelu_approx in ("none", "tanh") and _ext.available())

    def _batched_ok(self, rows: int) -> bool:
        sp = self.spec
        return (BATCHED_BLOCK and rows > FUSED_MAX_ROWS and sp.C % 32 == 0 and sp.C <= 1024
                and sp.blocks[0].fc.out_features % 32 == 0 and sp.gelu_approx in ("none", "tanh")
                and _ext.available())

    def forward(self, idx: Tensor, cache) -> Tensor:
        """idx [rows, 1] -> logits [rows, V] (bf16); appends this step's K/V at cache.pos_t."""
        sp = self.spec
        rows, C, H, D = idx.shape[0], sp.C, sp.H, sp.D
        if self.q8 is not None:
            x = fused_ops.embedding_fwd(idx, sp.wte.weight, sp.wpe.weight, 0, pos_dev=cache.pos_t)  # fp32 [rows, C]
            s = _GemvQ8Steps(self, x, torch.empty_like(x))
        elif (rows == 1 and self._gemv_ok(rows) and sp.wte.weight.dtype == torch.bfloat16
                and sp.wpe.weight.dtype == torch.bfloat16):
            # the first block's LN + QKV GEMV reads the embedding row itself (no embedding kernel):
            # B = 1 0.3548 / 0.3564 -> 0.3520 / 0.3544 ms; at 4 rows every workgroup's four-row
            # gather cost more than the launch it saves (0.535 -> 0.551), profiles/decode_r5.md
            x = torch.empty(rows, C, dtype=torch.float32, device=idx.device)
            s = _GemvSteps(self, x, torch.empty_like(x), emb=(idx.reshape(-1).contiguous(), cache.pos_t))
        else:
            x = fused_ops.embedding_fwd(idx, sp.wte.weight, sp.wpe.weight, 0, pos_dev=cache.pos_t)  # fp32 [rows, C]
            if self._batched_ok(rows):
                s = _BatchedSteps(self, x)
            elif self._gemv_ok(rows):
                s = _GemvSteps(self, x, torch.empty_like(x))
            elif self._fused_ok(rows):
                s = _FusedSteps(self, x, torch.empty_like(x))
            else:
                s = _PlainSteps(self, x, torch.empty_like(x))
        for l, blk in enumerate(sp.blocks):
            ln1, ln2 = self.ln[l]
            pb, fb = self.out_bias[l]
            q, k, v = _qkv_views(s.norm_linear(ln1, blk.qkv), H, H, D)
            o = cache._attend_graph(l, q, k, v)
            s.project(o.view(rows, C), blk.proj, pb)
            h = s.norm_linear(ln2, blk.fc, gelu=True)  # a local: allocated until the next block's (_defer)
            s.project(h, blk.fc2, fb)
        return s.head(self.lnf, sp.head)


def _packed_gate_up(mlp):
    """The [gate; up] weight of one gated MLP as one contiguous tensor, built once per weight
    version and cached on the module, so every decoder of the model shares one copy (no autograd
    graph: built under no_grad)."""
    g, u = mlp.gate_proj.weight, mlp.up_proj.weight
    key = (g.data_ptr(), g._version, u.data_ptr(), u._version)
    hit = mlp.__dict__.get("_packed_gu")
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        gu = torch.cat([g, u]).contiguous()
    mlp.__dict__["_packed_gu"] = (key, gu)
    return gu


class GemmaDecodeProgram:
    """One decode step of a Gemma-family bf16 model (``models/hf.py`` layer list) as an explicit
    kernel sequence.

    The module forward runs ~16 kernels per block at decode shapes (four RMSNorms, two residual
    adds, separate gate and up GEMMs). Per block this runs 6 (+1 split-K combine): QKV GEMM with
    RoPE (device-offset table) in its epilogue → decode attention with fused K/V append → O GEMM →
    [residual add + post-attention norm + pre-MLP norm] → gate|up GEMM (one concatenated weight)
    with the gated activation in its epilogue → down GEMM → [residual add + post-MLP norm + the
    next block's input norm]. ``forward`` is one loop over those steps; ``_qkv``, ``_gate_up`` and
    ``_lin`` pick each linear's kernel by the row count: the decode GEMVs for 1-4 rows, the skinny
    MFMA kernels (``skinny_qkv_rope``, ``skinny_gated``) up to SKINNY_MAX_ROWS, decode_gemm /
    hipBLASLt above. Rounding follows the module path (bf16 residual stream, torch's rounding
    points), so only the GEMM accumulation order of the fused gate|up projection can differ.
    Reference block semantics: ``neural_net_layers.py:188-225``.
    """

    def __init__(self, emb, blocks, norm_f, head):
        self.emb, self.norm_f, self.head = emb, norm_f, head
        self.blocks = []
        for b in blocks:
            in_norm, qkv, attn, o = list(b.attn_block)
            pre_mlp, mlp = list(b.mlp_block)
            if b.post_attn_norm is None:
                mode = 2
            else:
                mode = 0 if b.post_norm_on_residual else 1
            self.blocks.append(dict(
                in_norm=in_norm, qkv=qkv.weight, attn=attn, o=o.weight, pre_mlp=pre_mlp, mode=mode,
                post_attn=b.post_attn_norm, post_mlp=b.post_mlp_norm,
                gu=_packed_gate_up(mlp), down=mlp.down_proj.weight,
                kind=act_ops._GATED[mlp.act_kind], mods=(qkv, o, mlp)))
        self.q8 = False  # enable_q8: the blocks then carry int8 copies (qkv_q8, o_q8, gu_q8, down_q8)
        self.head_q8 = None

    @staticmethod
    def build(model):
        if not DECODE_PROGRAM:
            return None
        from torch import nn
        from penroz.models import layers as L
        mods = list(model.layers)
        if mods and isinstance(mods[-1], L.SoftmaxOnLast):
            mods = mods[:-1]
        if (len(mods) < 4 or not isinstance(mods[0], L.ScaledEmbedding) or not isinstance(mods[-2], L.RMSNorm)
                or not isinstance(mods[-1], nn.Linear) or mods[-1].bias is not None):
            return None
        if any(p.dtype != torch.bfloat16 for p in model.parameters()):
            return None
        C = mods[0].embedding_dim
        if C % 8 or C > 6144:
            return None
        for b in mods[1:-2]:
            if not isinstance(b, L.TransformerBlock) or (b.post_attn_norm is None) != (b.post_mlp_norm is None):
                return None
            ab, mb = list(b.attn_block), list(b.mlp_block)
            if not (len(ab) == 4 and isinstance(ab[0], L.RMSNorm) and isinstance(ab[1], nn.Linear)
                    and isinstance(ab[2], L.CausalSelfAttention) and isinstance(ab[3], nn.Linear)
                    and len(mb) == 2 and isinstance(mb[0], L.RMSNorm) and isinstance(mb[1], L.GatedMLP)):
                return None
            a, mlp = ab[2], mb[1]
            if (ab[1].bias is not None or ab[3].bias is not None or mlp.gate_proj.bias is not None
                    or mlp.down_proj.bias is not None or a.head_dim not in attn_ops.DECODE_HEAD_DIMS
                    or mlp.gate_proj.out_features % 8):
                return None
            norms = [ab[0], mb[0]] + ([b.post_attn_norm, b.post_mlp_norm] if b.post_attn_norm is not None else [])
            if any(not isinstance(n, L.RMSNorm) for n in norms):
                return None
        return GemmaDecodeProgram(mods[0], mods[1:-2], mods[-2], mods[-1])

    def _gemv_ok(self, rows: int, C: int) -> bool:
        """Batch 1-4: every projection as one decode GEMV (decode_gemv / decode_gemv_pair:
        one wave per workgroup, one memory round trip; RoPE and the gated activation in the
        paired-row epilogues). The residual adds + RMSNorms stay the rms_residual kernel: as the
        GEMVs' prologue — every workgroup normalising the rows itself — it measured neutral
        (Gemma-3 1B B=1 1.576 / 1.579 vs 1.571 / 1.571 ms, profiles/decode_r5.md)."""
        if not _ext.available():
            return False
        # the QKV and gate|up projections (K = C) are paired-row GEMVs; the O and down projections
        # are plain ones and read K = H·D and the intermediate size (12288 on Gemma-4 e2b's
        # KV-shared double-wide MLPs: above decode_gemv's K limit)
        max_rows, max_k, _, max_pair_k = _gemv_limits()
        return (1 <= rows <= min(max_rows, GEMV_MAX_ROWS) and C % 8 == 0 and C <= max_pair_k
                and all(b["o"].shape[1] <= max_k and b["down"].shape[1] <= max_k for b in self.blocks))

    def enable_q8(self, rows: int) -> bool:
        """Int8 weights for this row count: admitted when the step runs the decode GEMVs with their
        RoPE / gated epilogues and every linear's K fits the int8 kernel — all of the step or none
        of it. Builds (or finds) the quantised copies now, outside any capture; the gate|up pair is
        quantised after packing (one [2I, K] operand, one [2I] scale)."""
        C = self.emb.embedding_dim
        if not (DECODE_EPILOGUES and self._gemv_ok(rows, C)):
            return False
        max_rows, max_k, _, max_pair_k, k_mult = _gemv_q8_limits()
        if rows > max_rows or C % k_mult or C > max_pair_k or self.head.weight.shape[1] != C:
            return False
        for b in self.blocks:
            a = b["attn"]
            if (b["qkv"].shape[1] != C or b["gu"].shape[1] != C or b["gu"].shape[0] % 2
                    or any(b[k].shape[1] % k_mult or b[k].shape[1] > max_k for k in ("o", "down"))
                    or (a.rope_theta is not None and (a.head_dim % 2 or b["qkv"].shape[0] % a.head_dim))):
                return False
        for b in self.blocks:
            qkv, o, mlp = b["mods"]
            b["qkv_q8"], b["o_q8"] = wq_ops.linear_q8(qkv), wq_ops.linear_q8(o)
            b["down_q8"] = wq_ops.linear_q8(mlp.down_proj)
            b["gu_q8"] = wq_ops.cached_q8(mlp, "_packed_gu_q8", (mlp.gate_proj.weight, mlp.up_proj.weight),
                                          lambda mlp=mlp: _packed_gate_up(mlp))
        self.head_q8 = wq_ops.linear_q8(self.head)
        self.q8 = True
        return True

    def _lin(self, x: Tensor, w: Tensor, gemv: bool, q8=None) -> Tensor:
        if q8 is not None:
            return gemm_ops.decode_gemv_q8(x.contiguous(), q8)
        if gemv and w.shape[1] % 8 == 0 and w.shape[1] <= _gemv_limits()[1]:
            return gemm_ops.decode_gemv(x.contiguous(), w)
        return _linear(x, w)

    def _qkv(self, b, y: Tensor, cache, gemv: bool):
        """This block's fused QKV rows, and the (cos, sin) the attention still has to apply to q and
        the new key (None: already rotated, or a block without RoPE). Per block: layer lists may mix
        head dims."""
        a, rows = b["attn"], y.shape[0]
        H, Hkv, D = a.num_heads, a.num_kv_heads, a.head_dim
        if a.rope_theta is None:
            return self._lin(y, b["qkv"], gemv, b["qkv_q8"] if self.q8 else None), None
        inv = a._inv_freq(D, y.device)
        cos, sin = cache.rope_table((a.rope_theta, D), inv, 1)
        if getattr(cache, "ragged", False):
            # a ragged step: cos / sin are [rows, D/2] and the RoPE epilogues take one position's table, so
            # the plain QKV linear, then the RoPE pass over the rows viewed as [1, rows, W]
            qkv = self._lin(y, b["qkv"], gemv, b["qkv_q8"] if self.q8 else None)
            return rope_ops.apply_rope_qkv(qkv.view(1, rows, -1), H, Hkv, D, inv, 0, table=(cos, sin)).view(rows, -1), None
        if self.q8:
            return gemm_ops.decode_gemv_q8_rope(y.contiguous(), b["qkv_q8"], cos, sin, D, H + Hkv), None
        if gemv and DECODE_EPILOGUES and D % 2 == 0:
            return gemm_ops.decode_gemv_rope(y.contiguous(), b["qkv"], cos, sin, D, H + Hkv), None
        if DECODE_EPILOGUES and rows <= SKINNY_MAX_ROWS and gemm_ops.skinny_qkv_rope_ok(y, b["qkv"], D):
            return gemm_ops.skinny_qkv_rope(y, b["qkv"], cos, sin, D, H + Hkv), None
        if getattr(cache, "rope_attend_ok", None) is not None and cache.rope_attend_ok(rows, H, Hkv, D):
            # 17-64 rows: q and the new key rotated inside the decode attention kernel
            return _linear(y, b["qkv"]), (cos, sin)
        return rope_ops.apply_rope_qkv(_linear(y, b["qkv"]).view(rows, 1, -1), H, Hkv, D, inv, 0,
                                       table=(cos, sin)), None

    def _gate_up(self, b, y: Tensor, gemv: bool) -> Tensor:
        if self.q8:
            return gemm_ops.decode_gemv_q8_gated(y.contiguous(), b["gu_q8"], b["kind"])
        if gemv and DECODE_EPILOGUES:
            return gemm_ops.decode_gemv_gated(y.contiguous(), b["gu"], b["kind"])
        return _gated(y, b["gu"], b["kind"])

    def forward(self, idx: Tensor, cache) -> Tensor:
        """idx [rows, 1] -> logits [rows, V] (bf16); appends this step's K/V at cache.pos_t."""
        K = _ext.kernels()
        rows = idx.shape[0]
        gemv = self._gemv_ok(rows, self.emb.embedding_dim)
        x = torch.nn.functional.embedding(idx.view(rows), self.emb.weight) * self.emb.scale
        first = self.blocks[0]["in_norm"]
        y = K.rmsnorm_fwd(x, first.weight, first.eps)[0]
        for l, b in enumerate(self.blocks):
            a = b["attn"]
            H, Hkv, D = a.num_heads, a.num_kv_heads, a.head_dim
            qkv, rope = self._qkv(b, y, cache, gemv)
            q, k, v = _qkv_views(qkv, H, Hkv, D)
            att = cache.attend(l, q, k, v) if rope is None else cache.attend_rope(l, q, k, v, *rope)
            o = self._lin(att.view(rows, H * D), b["o"], gemv, b["o_q8"] if self.q8 else None)
            pa, pm, pre = b["post_attn"], b["post_mlp"], b["pre_mlp"]
            h, y = K.rms_residual(x, o, pa.weight if pa is not None else None, pre.weight, b["mode"],
                                  pa.eps if pa is not None else 0.0, pre.eps)
            g = self._gate_up(b, y, gemv)
            d = self._lin(g, b["down"], gemv, b["down_q8"] if self.q8 else None)
            nxt = self.blocks[l + 1]["in_norm"] if l + 1 < len(self.blocks) else self.norm_f
            x, y = K.rms_residual(h, d, pm.weight if pm is not None else None, nxt.weight, b["mode"],
                                  pm.eps if pm is not None else 0.0, nxt.eps)
        return self._lin(y, self.head.weight, gemv, self.head_q8 if self.q8 else None)


# 17-32 rows: decode_linear.hip decode_gemm (16 rows × 16 columns per workgroup, K split over its
# waves) instead of hipBLASLt, whose picks for these skinny shapes ran 36-216 workgroups
# (profiles/notes_r6.md §13); up to this many output columns (the lm_head keeps hipBLASLt).
# PENROZ_DECODE_GEMM=0: hipBLASLt (A/B)
DECODE_GEMM = os.environ.get("PENROZ_DECODE_GEMM", "1") != "0"
DECODE_GEMM_MAX_ROWS, DECODE_GEMM_MAX_N = 32, 32768


def _decode_gemm_ok(x: Tensor, w: Tensor, gated: bool = False) -> bool:
    """decode_gemm takes 17-32 rows (Gemma-3 1B B = 17 / 32: 2.20 -> 1.92 / 2.22 -> 2.07
    ms/step). At 64 rows every mix measured slower than hipBLASLt's step (2.42 ms: 2.60-2.88;
    the narrow O / down projections ran 19 vs 8-12 µs), so those keep hipBLASLt
    (profiles/notes_r6.md §13)."""
    n = w.shape[0] // 2 if gated else w.shape[0]
    return (DECODE_GEMM and SKINNY_MAX_ROWS < x.shape[0] <= DECODE_GEMM_MAX_ROWS and x.is_cuda
            and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0 and w.is_contiguous() and w.data_ptr() % 16 == 0
            and w.shape[1] == x.shape[1] and x.shape[1] % 32 == 0 and n % 16 == 0 and n <= DECODE_GEMM_MAX_N
            and _ext.available())


def _gated(x: Tensor, gu: Tensor, kind: int) -> Tensor:
    """act(x·Wgᵀ) ⊙ (x·Wuᵀ) from the packed gate|up weight: one fused launch with the activation
    in the GEMM epilogue (the skinny kernel up to SKINNY_MAX_ROWS rows, decode_gemm up to 64), else
    GEMM + packed activation."""
    if DECODE_EPILOGUES and x.shape[0] <= SKINNY_MAX_ROWS and gemm_ops.skinny_ok(x, gu):
        return gemm_ops.skinny_gated(x, gu, kind)
    if DECODE_EPILOGUES and _decode_gemm_ok(x, gu, gated=True):
        out = torch.empty(x.shape[0], gu.shape[0] // 2, device=x.device, dtype=torch.bfloat16)
        _ext.kernels().decode_gemm(x, gu, out, kind)
        return out
    return _ext.kernels().gated_act_packed(_linear(x, gu), kind)


def _linear(x: Tensor, w: Tensor) -> Tensor:
    """x [M, K] · wᵀ without bias: the decode-shaped MFMA kernels up to 64 rows."""
    if x.shape[0] <= SKINNY_MAX_ROWS and gemm_ops.skinny_ok(x, w):
        return gemm_ops.skinny_linear(x, w, None)
    if _decode_gemm_ok(x, w):
        out = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.bfloat16)
        _ext.kernels().decode_gemm(x, w, out, -1)
        return out
    return torch.mm(x, w.t())


def applicable(model) -> bool:
    if not GRAPH_DECODE or not torch.cuda.is_available():
        return False
    p = next(model.parameters(), None)
    if p is None or not p.is_cuda:
        return False
    attn = model._find_attention_layers()
    if not attn:
        return False
    # the captured step appends K/V and attends inside the decode kernel, so every layer's head_dim
    # must have one (HF Gemma builders set head_dim; GPT-pattern models derive it from C / H)
    gpt_d = None
    if any(a.head_dim is None for a in attn):
        from penroz.models.executor import GPTExecutor
        spec = GPTExecutor.match(model)
        gpt_d = spec.D if spec is not None else None
    for a in attn:
        d = a.head_dim if a.head_dim is not None else gpt_d
        if d is not None and d not in attn_ops.DECODE_HEAD_DIMS:
            return False
        if d is None and a.rope_theta is not None:
            return False
    return True


class StepMode(NamedTuple):
    """Which optional kernels a decoder's step runs; one captured graph per mode, captured on first use."""
    penalised: bool = False
    logprobs: bool = False
    stop: bool = False
    bias_form: str = "off"  # the logit-bias rewrite: "off", "entries" or "mask" (entries and the allowed mask)


class GraphDecoder:
    """Static decode state + the captured step graph for ``rows`` sequences."""

    def __init__(self, model, rows: int, capacity: int, temperature: float, top_k: int | None,
                 top_p: float | None = None, min_p: float | None = None, weight_quant: str | None = None,
                 ragged: bool = False, speculate: int | None = None):
        # weak: the model caches its decoders (model.__dict__), so a strong reference would make a
        # cycle that only the cyclic GC frees — and a collection that runs while ANOTHER graph is
        # being captured destroys this one's graph mid-capture (a hard abort)
        self._model = weakref.ref(model)
        self.device = next(model.parameters()).device
        self.attn = model._find_attention_layers()
        self.pos_layers = model._find_position_embeddings()
        cls = StaticTurboKVCache if kvc.TURBO_QUANT_ENABLED else StaticKVCache
        self.cache = cls(len(self.attn), capacity)
        # ragged (ops/ragged.py): every row at its own position and cache length — pos_t / len_t are [rows]
        self.ragged = bool(ragged)
        # speculative (ops/speculative.py): ``rows`` = k + 1 positions of one sequence in a batch-1 cache
        self.speculate = int(speculate or 0)
        assert not self.speculate or (rows == self.speculate + 1 and not self.ragged and not temperature), \
            (rows, speculate, ragged, temperature)
        self.cache.init_graph_state(self.device, rows if self.ragged or self.speculate else None,
                                    shared=bool(self.speculate))
        self._lens_t: Tensor | None = None  # the call's prompt lengths [rows] (device) and the longest
        self._lmax = 0
        self.rows, self.capacity = rows, capacity
        self.temperature, self.top_k = float(temperature), top_k
        self.top_p, self.min_p = _normalise_filters(temperature, top_p, min_p)
        self.idx = torch.zeros(rows, 1, dtype=torch.long, device=self.device)
        self.out = torch.zeros(rows, capacity, dtype=torch.long, device=self.device)
        self.step_t = torch.zeros(1, dtype=torch.long, device=self.device)
        self.seed_t = torch.zeros(1, dtype=torch.long, device=self.device)  # per-run sampling salt
        self.run_seed = 0  # set by begin()
        self.graph: torch.cuda.CUDAGraph | None = None
        gemm_ops.skinny_workspace(self.device)  # zeroed counters exist before any capture
        attn_ops.decode_counters(self.device)  # (the decode attention's split-merge counters too)
        gemm_ops.load_tuned_gemms()  # measured hipBLASLt solutions for the decode-shaped GEMMs too
        self.program = GPTDecodeProgram.build(model) or GemmaDecodeProgram.build(model)
        if self.ragged and self.program is None:
            raise ValueError("a ragged decoder needs a decode program (bf16 GPT-2-pattern or Gemma-family model)")
        if self.speculate:
            if self.program is None or not _ext.available():
                raise ValueError("a speculative decoder needs a decode program (bf16 GPT-2-pattern or Gemma-family "
                                 "model) and the built kernels")
            # the history and its int32 counters in one buffer, so a burst's result is one read:
            # [n, emitted, limit, steps, accepted, -, -, -] then hist [capacity]
            self._spec_buf = torch.zeros(8 + capacity, dtype=torch.int32, device=self.device)
            self.hist = self._spec_buf[8:]
            self.n_t, self.emitted_t, self.limit_t, self.steps_t, self.accepted_t = (self._spec_buf[i:i + 1] for i in range(5))
            self._greedy_u = torch.zeros(rows, dtype=torch.float32, device=self.device)  # (the greedy sampler reads none)
            self._spec_host: tuple[list[int], int] | None = None  # what _set_state loads: (tokens, limit)
        # the weight format in effect: "int8" when asked for AND this decoder's step qualifies (a
        # decode program at 1-4 rows whose linears all fit the int8 GEMV); the quantised copies exist
        # from here on, before the warm-up step and the capture
        self.weight_quant = None
        if wq_ops.resolve(weight_quant or "") == "int8":
            if self.program is not None and self.program.enable_q8(rows):
                self.weight_quant = "int8"
            else:
                _log_q8_unused(rows, self.program)
        self._done_t = torch.zeros(1, dtype=torch.int32, device=self.device)  # sample_step's arrival counter
        # the options' states, each made by the first ``configure`` that asks for it (their buffers are
        # static): logit penalties, per-token log-probabilities, stop sequences, logit bias / banned /
        # allowed tokens / min_tokens
        self.penalties: pen_ops.PenaltyState | None = None
        self.logprobs: lp_ops.LogprobState | None = None
        self.stop: stop_ops.StopState | None = None
        self.bias: bias_ops.BiasState | None = None
        self._count_new = True  # (False during a capture's warm-up step: its token is not a real one)
        # what the last run() left: (lp [rows, n_steps], top_id, top_lp [rows, n_steps, 20]) or None
        self.last_logprobs: tuple[Tensor, Tensor, Tensor] | None = None
        # which of them the step runs — ``graph`` is this mode's — and the other modes' captured graphs
        self.mode = StepMode()
        self._graphs: dict[StepMode, torch.cuda.CUDAGraph | None] = {}

    _penalised = property(lambda self: self.mode.penalised)
    _lp_on = property(lambda self: self.mode.logprobs)
    _stop_on = property(lambda self: self.mode.stop)
    _bias_form = property(lambda self: self.mode.bias_form)

    # ------------------------------------------------------------------ cache attachment
    def attach(self):
        for i, a in enumerate(self.attn):
            a.set_kv_cache(self.cache, i)

    def detach(self):
        for a in self.attn:
            a.set_kv_cache(None, 0)
        for p in self.pos_layers:
            p.position_offset = 0
            p.position_offset_tensor = None

    # ------------------------------------------------------------------ the step
    def _step(self):
        if self.speculate:
            return self._spec_step()
        for p in self.pos_layers:
            p.position_offset_tensor = self.cache.pos_t
        self.cache.graph_mode = True
        self.cache.begin_step()
        try:
            if self.program is not None:
                last = self.program.forward(self.idx, self.cache)
            else:
                model = self._model()
                with gemm_ops.decode_gemms(model, max_rows=SKINNY_MAX_ROWS):
                    acts, _ = model(self.idx, skip_softmax=True)
                logits = acts[-1]
                last = logits[:, -1, :] if logits.ndim == 3 else logits
            if self._penalised:
                # counts idx, the token the previous step sampled, then rewrites the seen tokens'
                # logits in the tensor the sampler reads
                last = self.penalties.apply(last.contiguous(), self.idx if self._count_new else None)
            if self._bias_form != "off":
                # behind the penalties: t = base_t (the burst's start) + step_t, read on the device
                last = self.bias.step(last.contiguous(), self.step_t)
            last = last.contiguous()  # the one tensor the sampler and the log-probabilities read
            if _ext.available() and last.is_cuda:
                # one sampler kernel writes the token into the next step's input and the burst
                # buffer (uniforms hashed on the device), one kernel advances the counters
                V = last.shape[-1]
                k = 0 if self.top_k is None or self.top_k >= V else int(self.top_k)
                # the nucleus / min-p cut is made by the sampler inside the captured graph
                nuc = () if self.top_p is None and self.min_p is None else (self.top_p or 1.0, self.min_p or 0.0)
                if FUSED_ADVANCE:  # the sampler's last row advances the counters itself
                    _ext.kernels().sample_step(last, self.temperature, k, self.seed_t, self.step_t,
                                               self.idx, self.out, self.cache.pos_t, self.cache.len_t, self._done_t,
                                               *nuc)
                else:
                    _ext.kernels().sample_step(last, self.temperature, k, self.seed_t, self.step_t,
                                               self.idx, self.out, None, None, None, *nuc)
                    _ext.kernels().decode_advance(self.cache.pos_t, self.cache.len_t, self.step_t)
            else:
                nxt = samp_ops.sample(last, self.temperature, self.top_k, device_rng=True, top_p=self.top_p,
                                      min_p=self.min_p)
                torch.add(nxt, 0, out=self.idx)  # a kernel, not a memcpy node
                self.out.index_copy_(1, self.step_t, nxt)
                self.cache.pos_t.add_(1)
                self.cache.len_t.add_(1)
                self.step_t.add_(1)
            if self._lp_on:
                # behind the sampler and the counter advance: idx holds the token just chosen, and
                # column step_t - 1 of the burst buffers is this step's
                lp_ops.step_logprobs(self.logprobs, last, self.idx, self.step_t)
            if self._stop_on and self._count_new:
                # last in the step: checks the token just chosen, and freezes the rows that finished
                # before on theirs (idx and this step's column of the burst buffer)
                self.stop.step(self.idx, self.out, self.step_t)
        finally:
            self.cache.graph_mode = False
            for p in self.pos_layers:
                p.position_offset_tensor = None

    def _spec_step(self):
        """One speculative step: the program on the k + 1 rows of ``idx`` at ``pos_t``, the greedy sampler on
        every row, then ``spec_advance``: accept, emit into ``hist``, draft, and the next step's idx / pos_t /
        len_t. No ``sample_step`` and no fused advance: nothing here counts steps by one."""
        K = _ext.kernels()
        self.cache.graph_mode = True
        self.cache.begin_step()
        try:
            last = self.program.forward(self.idx, self.cache).contiguous()
            cand = K.sample_tokens(last, self._greedy_u, 0.0, 0)
            K.spec_advance(self.hist, self.n_t, cand, self.idx, self.cache.pos_t, self.cache.len_t, self.emitted_t,
                           self.limit_t, self.steps_t, self.accepted_t, self.speculate, False)
        finally:
            self.cache.graph_mode = False

    def _spec_load(self, tokens: list[int], limit: int):
        """The state of a call whose sequence so far is ``tokens`` and which wants ``limit`` more: history,
        counters at zero, and — the draft half of ``spec_advance``, run eagerly — the first step's rows."""
        n = len(tokens)
        assert 1 <= n and limit >= 0 and n + limit + self.speculate <= self.capacity, (n, limit, self.capacity)
        head = torch.tensor([n, 0, limit, 0, 0, 0, 0, 0] + list(tokens), dtype=torch.int32)
        self._spec_buf[:head.numel()].copy_(head)
        _ext.kernels().spec_advance(self.hist, self.n_t, self.idx, self.idx, self.cache.pos_t, self.cache.len_t,
                                    self.emitted_t, self.limit_t, self.steps_t, self.accepted_t, self.speculate, True)

    @torch.inference_mode()
    def run_speculative(self, tokens: list[int], limit: int, stop_token: int | None = None):
        """Emit ``limit`` tokens behind ``tokens`` (the sequence so far; the cache holds its positions — the
        last one's slot is rewritten by the first step, whose row 0 feeds that token, so a cache that holds
        all but the last will do as well) -> (the new tokens, cut behind the first
        ``stop_token``; {"steps", "drafted", "accepted"}). Bursts of ``ceil(remaining / (k + 1))`` replays with
        no host synchronisation inside; after each, one read of the counters and the history. Every step emits
        at least one token and a step at the limit is frozen, so a burst neither stalls nor overshoots."""
        k, n0 = self.speculate, len(tokens)
        assert self.cache.seq_len() in (n0 - 1, n0), (self.cache.seq_len(), n0)
        self._spec_host = (list(tokens), int(limit))
        if self.graph is None:
            self._capture(None, None, 0)
        else:
            self._set_state(None, None, 0)
        n, emitted, steps, accepted, new = n0, 0, 0, 0, []
        while emitted < limit:
            burst = -(-(limit - emitted) // (k + 1))
            for _ in range(burst):
                self.graph.replay()
            got = self._spec_buf[:8 + min(n + burst * (k + 1), self.capacity)].tolist()
            n1, emitted, steps, accepted = got[0], got[1], got[3], got[4]
            assert n1 > n and n1 - n0 == emitted, (n, n1, n0, emitted)  # every step emits
            new += got[8 + n:8 + n1]
            n = n1
            if stop_token is not None and stop_token in new:
                new = new[:new.index(stop_token) + 1]
                break
        self.cache._len = [n0 + len(new) - 1] * self.cache.num_layers
        return new, {"steps": steps, "drafted": steps * k, "accepted": accepted}

    # The sampler kernel hashes each uniform from (seed_t, step_t, row) as
    #   seed + G·(step + 1) + R·(row + 1)  (mod 2^64, csrc/kernels/sampling.hip),
    # with step_t counting from 0 inside a burst. Loading seed_t = run_seed + G·start for a burst
    # that starts at absolute token index ``start`` makes every draw a function of
    # (run seed, absolute index, row) alone: how the tokens are cut into bursts (streaming = bursts
    # of 1, non-streaming = one long burst), and whether the graph was captured in this call or
    # reused, no longer changes them.
    _HASH_STEP = 0x9E3779B97F4A7C15

    def begin(self, run_seed: int):
        """Once per generate call: the seed every burst of this call derives from."""
        self.run_seed = int(run_seed) & (2 ** 64 - 1)

    def configure(self, opts):
        """Once per generate call, with its checked options (``ops.decode_options.DecodeOptions``): makes
        the states the call needs and this decoder does not have yet, loads the call's values into them,
        and makes ``graph`` the captured step of the call's ``StepMode`` (None: captured on first use).
        An option that is off costs the step no kernel. The step reads every value from the device, so
        other penalty values, another n, another stop set, other bias entries, another allowed set and
        another ``min_tokens`` replay the same graph; with and without an allowed set are two modes (their
        grids differ). The caller begins ``penalties`` / ``stop`` once per call and reads ``stop.read()``
        after a burst."""
        if opts.penalties is not None:
            if self.penalties is None:
                self.penalties = pen_ops.PenaltyState()
            self.penalties.set_params(*opts.penalties)
        if opts.logprobs is not None:
            if self.logprobs is None:
                self.logprobs = lp_ops.LogprobState(self.rows, self.capacity, self.device)
            self.logprobs.set_n(opts.logprobs)
        if opts.stop is not None:
            if self.stop is None:
                self.stop = stop_ops.StopState(self.rows, self.device)
            self.stop.set_stop(opts.stop)
        if opts.bias is not None:
            if self.bias is None:
                self.bias = bias_ops.BiasState(self.device)
            self.bias.set(opts.bias)
        mode = StepMode(opts.penalties is not None, opts.logprobs is not None, opts.stop is not None,
                        "off" if opts.bias is None else self.bias.form)
        if mode != self.mode:
            self._graphs[self.mode] = self.graph
            self.graph = self._graphs.pop(mode, None)
            self.mode = mode

    def _burst_seed(self, start: int) -> int:
        v = (self.run_seed + self._HASH_STEP * int(start)) & (2 ** 64 - 1)
        return v - 2 ** 64 if v >= 2 ** 63 else v

    def set_lengths(self, lens: list[int]):
        """Once per ragged generate call, before its first ``run()``: the rows' prompt lengths. The
        eager prefill pads to the longest, so the host-side cache length counts from there; row ``b``'s
        own is that minus ``max(lens) - lens[b]``."""
        assert self.ragged and len(lens) == self.rows and min(lens) >= 1, (self.ragged, len(lens), self.rows)
        self._lens_t = torch.tensor(lens, dtype=torch.long, device=self.device)
        self._lmax = max(lens)

    def _row_lengths(self, cache_len: int):
        """What ``_set_state`` takes for a host-side cache length (the longest row's): the number itself,
        or, ragged, every row's own length [rows] on the device."""
        if not self.ragged:
            return cache_len
        assert self._lens_t is not None, "ragged decoder: set_lengths() comes before run()"
        return self._lens_t + (cache_len - self._lmax)

    def _set_state(self, last_tok: Tensor, cache_len, start: int = 0):
        """``cache_len``: the cache length every row is at — or, ragged, int64 [rows]: each row's own. A
        speculative decoder's state is its call's (``run_speculative``), whatever the arguments."""
        if self.speculate:
            return self._spec_load(*self._spec_host)
        self.seed_t.fill_(self._burst_seed(start))
        self.idx.copy_(last_tok)
        if self.ragged:
            self.cache.pos_t.copy_(cache_len)
            torch.add(cache_len, 1, out=self.cache.len_t)
        else:
            self.cache.pos_t.fill_(cache_len)
            self.cache.len_t.fill_(cache_len + 1)
        self.step_t.zero_()
        if self._bias_form != "off":
            self.bias.base_t.fill_(int(start))  # the step's t = start + step_t

    def _capture(self, last_tok: Tensor, cache_len, start: int = 0):
        # warm-up run on a side stream (lazy allocations, kernel loading), then capture. The
        # warm-up really executes a step, so it must start from the true state: it then writes
        # exactly the cache slot the first real step rewrites.
        self._set_state(last_tok, cache_len, start)
        # the penalty tables exist and hold this call's prompt (the eager prefill step applied them):
        # nothing is allocated inside the capture, and the warm-up step counts no token
        assert not self._penalised or self.penalties.ready, "penalties: begin() and a first apply come before a capture"
        from penroz.models.executor import shared_stream
        side = shared_stream(self.device, "side")  # (no new pool stream per capture)
        side.wait_stream(torch.cuda.current_stream(self.device))
        self._count_new = False
        try:
            with torch.cuda.stream(side):
                self._step()
        finally:
            self._count_new = True
        torch.cuda.current_stream(self.device).wait_stream(side)
        self._set_state(last_tok, cache_len, start)
        g = torch.cuda.CUDAGraph()
        # no cyclic GC inside the capture: a collection there can free objects that own HIP
        # resources (another decoder's graph, events), which is illegal while capturing
        gc_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                self._step()
        finally:
            if gc_on:
                gc.enable()
        self.graph = g
        self._set_state(last_tok, cache_len, start)  # capture does not execute; state is as before
        spec = f" speculate={self.speculate}" if self.speculate else ""
        log.info(f"captured decode graph: rows={self.rows}{' ragged' if self.ragged else ''}{spec} block={self.capacity} "
                 f"temperature={self.temperature} top_k={self.top_k} top_p={self.top_p} min_p={self.min_p} "
                 f"penalties={'on' if self._penalised else 'off'} logprobs={'on' if self._lp_on else 'off'} "
                 f"stop={'on' if self._stop_on else 'off'} logit_bias={self._bias_form}")

    @torch.inference_mode()
    def run(self, last_tok: Tensor, n_steps: int, start: int = 0) -> Tensor:
        """Decode ``n_steps`` tokens after ``last_tok`` [rows, 1] from the current cache; returns
        the [rows, n_steps] new tokens (device). ``start``: absolute index (within this generate
        call) of the first of them. The cache must have room for n_steps more. With log-probabilities
        on, ``last_logprobs`` then holds this burst's (views of the burst buffers, like the tokens).
        Ragged: the host-side cache length is the longest row's (the capacity check is against it);
        the rows' own come from ``set_lengths``."""
        cache_len = self.cache.seq_len()
        assert 0 < cache_len and cache_len + n_steps <= self.capacity, (cache_len, n_steps, self.capacity)
        assert not self.ragged or cache_len >= self._lmax, (cache_len, self._lmax)
        lens = self._row_lengths(cache_len)
        if self.graph is None:
            self._capture(last_tok, lens, start)
        else:
            self._set_state(last_tok, lens, start)
        for _ in range(n_steps):
            self.graph.replay()
        self.cache._len = [cache_len + n_steps] * self.cache.num_layers
        self.last_logprobs = self.logprobs.burst(n_steps) if self._lp_on else None
        return self.out[:, :n_steps]


_q8_unused_logged = False


def _log_q8_unused(rows: int, program) -> None:
    """Once per process: int8 decode weights were asked for and this step keeps bf16 weights."""
    global _q8_unused_logged
    if _q8_unused_logged:
        return
    _q8_unused_logged = True
    why = ("the model has no decode program (bf16 GPT-2-pattern or Gemma-family)" if program is None
           else f"{rows} rows or a linear's K is outside the int8 decode GEMV's limits")
    log.info(f"int8 decode weights requested, but the step keeps bf16 weights: {why}")


def ragged_program_ok(model) -> bool:
    """A ragged step is an explicit decode program's (the module forward has one position for all rows),
    which the built kernels run."""
    if not _ext.available():
        return False
    p = next(model.parameters())
    key = (p.data_ptr(), p.dtype, DECODE_PROGRAM)
    hit = model.__dict__.get("_ragged_program_ok")
    if hit is None or hit[0] != key:  # (asked once per generate call: remembered per weights)
        hit = (key, (GPTDecodeProgram.build(model) or GemmaDecodeProgram.build(model)) is not None)
        model.__dict__["_ragged_program_ok"] = hit
    return hit[1]


def _normalise_filters(temperature: float, top_p: float | None, min_p: float | None):
    """(top_p, min_p) with the values that mean "no filter" — and both at temperature 0, which
    ignores them — folded to None, so equal behaviour shares one captured graph."""
    tp, mp = samp_ops._check_filters(top_p, min_p)
    if not temperature:
        return None, None
    return (tp if tp < 1.0 else None), (mp if mp > 0.0 else None)


def get_decoder(model, rows: int, block_size: int, temperature: float, top_k: int | None,
                top_p: float | None = None, min_p: float | None = None,
                weight_quant: str | None = None, ragged: bool = False,
                speculate: int | None = None) -> GraphDecoder | None:
    """Cached per model and (rows, block size, sampling settings, weights identity, ragged or not, weight
    format in effect for ``weight_quant`` — as ``ops.weight_quant.resolve`` returned it); None when the
    model does not qualify (CPU, no attention, RoPE head_dim without a decode kernel) or ``PENROZ_GRAPH_DECODE=0``
    — and, for a ragged decoder, when the model has no decode program or the kernels are not built."""
    # (these two are the only ways to None; ``NeuralNetworkModel._ragged_fallback`` names them to a ragged call
    # before its options are checked, so a third belongs there too: tests/test_ragged.py ties the two together)
    if not applicable(model):
        return None
    if (ragged or speculate) and not ragged_program_ok(model):
        return None
    p = next(model.parameters())
    # weights identity AND version: in-place updates (training) re-capture, so nothing captured
    # (e.g. LayerNorm's cached fp32 weight copies for bf16 models) can go stale
    version = sum(q._version for q in model.parameters())
    base = (rows, block_size, float(temperature), top_k if temperature else None,
            *_normalise_filters(temperature, top_p, min_p), kvc.TURBO_QUANT_ENABLED, p.data_ptr(), p.dtype, version,
            bool(ragged))
    if speculate:  # (a plain decoder's key is what it always was)
        base += (("speculate", int(speculate)),)
    cache = model.__dict__.setdefault("_graph_decoders", {})
    # the key holds the weight format IN EFFECT: a request for int8 that this step cannot honour
    # (more than 4 rows, no decode program, a K that does not fit) shares the bf16 decoder instead of
    # building a second identical one; which (rows, ...) settings those are is remembered per model
    unused = model.__dict__.setdefault("_q8_no_effect", set())
    if weight_quant is not None and base in unused:
        weight_quant = None
    dec = cache.get(base + (weight_quant,))
    if dec is None:
        spec = {"speculate": int(speculate)} if speculate else {}
        dec = GraphDecoder(model, rows, block_size, temperature, top_k, top_p, min_p, weight_quant, ragged=ragged, **spec)
        if dec.weight_quant != weight_quant:  # asked for int8, runs bf16
            if len(unused) >= 64:
                unused.clear()
            unused.add(base)
            twin = cache.get(base + (dec.weight_quant,))
            if twin is not None:
                return twin
        while len(cache) >= 2:  # bounded: each holds a KV cache and a graph memory pool
            cache.pop(next(iter(cache)))
        cache[base + (dec.weight_quant,)] = dec
    return dec


def decoder_for(model, rows: int, block_size: int, opts, ragged: bool = False) -> GraphDecoder | None:
    """``get_decoder`` for a generate call's checked options (``ops.decode_options.DecodeOptions``)."""
    ragged = {"ragged": True} if ragged else {}  # (a rectangular call's lookup is what it always was)
    if opts.speculate:  # k + 1 rows for the call's one sequence
        return get_decoder(model, opts.speculate + 1, block_size, 0.0, None, weight_quant=opts.weight_quant,
                           speculate=opts.speculate)
    return get_decoder(model, rows, block_size, opts.temperature, opts.top_k, opts.top_p, opts.min_p,
                       opts.weight_quant, **ragged)
