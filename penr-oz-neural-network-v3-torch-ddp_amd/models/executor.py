"""Fused GPT-2 training/eval executor for MI355X.

A layer list that matches the GPT-2 pattern of the reference's example/HF-import layout
(``main.py:57-83``, ``mappers.py:122-176``) is *lowered* to this executor while the
``nn.Module`` tree (and therefore every state_dict key) stays exactly as compiled.  Instead of
per-module autograd it runs an explicit forward and backward:

forward, per layer (N = B·T tokens, fp32 residual stream — the reference's autocast numerics)
  LN1 (HIP, → bf16) → QKV GEMM+bias (hipBLASLt) → flash attention (HIP, reads the fused QKV
  tensor, writes head-merged O + LSE) → proj GEMM+bias → residual-add+LN2 (one HIP pass)
  → fc GEMM+bias (hipBLASLt) → GELU (HIP elementwise kernel writing the activation; the
  pre-activation is kept for the backward) → fc2 GEMM+bias → (residual-add fused into the next LN)
head: final LN → lm_head GEMM → cross-entropy (HIP: one LDS-resident pass per row, writes
  the logits gradient in place, no fp32 logits). The head can run in token chunks
  (``_head_chunk_rows``: automatic above 8 GiB of logits, or ``PENROZ_HEAD_CHUNK`` rows):
  lm_head GEMM → CE → dgrad → wgrad per chunk over two rotating chunk buffers, so the [N, V]
  logits tensor is never materialised (the reference's ``F.cross_entropy`` over full logits,
  ``neural_net_model.py:263-267``).
backward mirrors it: dgrad/wgrad GEMMs (wgrad accumulated in fp32), GELU backward fused with
  the fc bias-gradient column sum, LayerNorm backward fused with dγ/dβ, the residual-gradient
  accumulation, its bf16 copy for the next GEMM, and the bias gradient of the preceding
  linear; flash-attention backward with the qkv bias gradient summed in its epilogues; embedding
  backward (dwte scatter, dwpe reduction).

Dropout (the HF GPT-2 import: embd/resid/attn_pdrop = 0.1, ``mappers.py:140-142`` in the
reference): attention dropout runs inside the flash kernels; embedding dropout inside the
embedding kernels; each residual branch's dropout inside the add+LayerNorm kernel that adds it
to the stream, and the LayerNorm backward applies the regenerated mask to the branch gradient.
Masks are hashed from (step seed, site, element) and never stored.

bf16-parameter models (``/import/`` loads HF weights in bf16, ``neural_net_model.py:222``) train
here too: the executor keeps fp32 master copies and makes the module parameters views of the
bf16 shadow the fused AdamW rewrites every step, so ``state_dict()`` stays bf16 (the checkpoint
dtype of the reference) while the update itself is fp32.

Parameters, gradients and AdamW moments live in flat fp32 buffers laid out in backward
completion order (lm_head … wte) so gradient buckets are contiguous slices: the reducer
launches each bucket's RCCL all-reduce as soon as the layers in it finish, overlapped with
the remaining backward.  A flat bf16 shadow of every parameter feeds the GEMMs and is
refreshed by the fused AdamW kernel in the same pass that updates the fp32 masters.

This module holds what is GPT-2 about that: the pattern match, the parameter order, the
activation buffers, the forward and the block loop of the backward. The flat buffers, the lm_head,
the side stream, ``zero_grad``, the reducer / optimizer plumbing and the stream helpers re-exported
here live in :class:`penroz.models.flat_executor.FlatExecutor`, shared with the Gemma executor.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import partial

import torch
import torch.nn as nn
from torch import Tensor

from penroz.models import layers as L
from penroz.models.flat_executor import (FlatExecutor, _head_chunk_rows, _high_priority_stream,  # noqa: F401
                                         _minus, _site_seed, cu_mask_words, shared_stream)
from penroz.ops import attention as attn_ops
from penroz.ops import fused as fused_ops
from penroz.ops import norms as norm_ops
from penroz.ops import gemm as gemm_ops
from penroz.utils.profiling import trace_range


@dataclass
class _Block:
    ln1: nn.LayerNorm
    qkv: nn.Linear
    attn: L.CausalSelfAttention
    proj: nn.Linear
    ln2: nn.LayerNorm
    fc: nn.Linear
    act: nn.GELU
    fc2: nn.Linear
    p_attn_res: float = 0.0  # dropout on the attention branch (after proj)
    p_mlp_res: float = 0.0   # dropout on the MLP branch (after fc2)


@dataclass
class GPTSpec:
    V: int
    C: int
    H: int
    D: int
    F: int
    P: int
    wte: nn.Embedding
    wpe: L.PositionEmbedding
    blocks: list = field(default_factory=list)
    lnf: nn.LayerNorm = None
    head: nn.Linear = None
    gelu_approx: str = "none"
    p_embd: float = 0.0
    param_dtype: torch.dtype = torch.float32


def _is(m, cls):
    return isinstance(m, cls)


def _dropout_ok(m) -> bool:
    return _is(m, nn.Dropout) and 0.0 <= m.p < 1.0


class GPTExecutor(FlatExecutor):
    PATTERN = "GPT-2"

    # ------------------------------------------------------------------ pattern match
    @staticmethod
    def match(model, require_fp32: bool = False) -> GPTSpec | None:
        """The GPT-2 block structure, with fp32 or bf16 parameters (one dtype for all; the
        executor keeps fp32 masters either way). ``require_fp32``: fp32 parameters only."""
        ls = list(model.layers)
        if len(ls) < 5:
            return None
        emb = ls[0]
        if not (_is(emb, L.Summation) and len(emb) == 2 and type(emb[0]) is nn.Embedding
                and _is(emb[1], L.PositionEmbedding)):
            return None
        if not _dropout_ok(ls[1]):
            return None
        tail = ls[-3:] if _is(ls[-1], L.SoftmaxOnLast) else ls[-2:]
        if len(tail) < 2 or not _is(tail[0], nn.LayerNorm) or not _is(tail[1], nn.Linear) or tail[1].bias is not None:
            return None
        body = ls[2:len(ls) - len(tail)]
        if not body:
            return None
        C = emb[0].embedding_dim
        spec = GPTSpec(V=emb[0].num_embeddings, C=C, H=0, D=0, F=0, P=emb[1].num_embeddings,
                       wte=emb[0], wpe=emb[1], lnf=tail[0], head=tail[1])
        approx = None
        for blk in body:
            if not (_is(blk, L.ResidualConnection) and len(blk) == 2):
                return None
            a, m = blk[0], blk[1]
            if not (_is(a, nn.Sequential) and len(a) == 5 and _is(m, nn.Sequential) and len(m) == 5):
                return None
            ln1, qkv, att, proj, d1 = a
            ln2, fc, act, fc2, d2 = m
            ok = (_is(ln1, nn.LayerNorm) and _is(qkv, nn.Linear) and _is(att, L.CausalSelfAttention)
                  and _is(proj, nn.Linear) and _dropout_ok(d1) and _is(ln2, nn.LayerNorm)
                  and _is(fc, nn.Linear) and _is(act, nn.GELU) and _is(fc2, nn.Linear) and _dropout_ok(d2))
            if not ok:
                return None
            if att.rope_theta is not None or att.num_kv_heads != att.num_heads or not 0.0 <= att.dropout < 1.0:
                return None
            H = att.num_heads
            D = C // H
            if (qkv.in_features, qkv.out_features) != (C, 3 * C) or (proj.in_features, proj.out_features) != (C, C):
                return None
            if fc.in_features != C or fc2.out_features != C or fc2.in_features != fc.out_features:
                return None
            if any(x.bias is None for x in (qkv, proj, fc, fc2)) or any(
                    x.weight is None or x.bias is None or tuple(x.normalized_shape) != (C,) for x in (ln1, ln2)):
                return None
            if approx is None:
                approx = act.approximate
            if act.approximate != approx:
                return None
            spec.H, spec.D, spec.F = H, D, fc.out_features
            spec.blocks.append(_Block(ln1, qkv, att, proj, ln2, fc, act, fc2, float(d1.p), float(d2.p)))
        if spec.D not in attn_ops.SUPPORTED_HEAD_DIMS or C % 64 != 0 or spec.F % 64 != 0:
            return None
        if tuple(spec.lnf.normalized_shape) != (C,) or spec.head.in_features != C:
            return None
        dtypes = {p.dtype for p in model.parameters()}
        if len(dtypes) != 1 or not dtypes <= ({torch.float32} if require_fp32 else {torch.float32, torch.bfloat16}):
            return None
        spec.param_dtype = dtypes.pop()
        spec.p_embd = float(ls[1].p)
        spec.gelu_approx = approx
        return spec

    def _param_order(self):
        s = self.spec
        segs = [[s.head.weight, s.lnf.weight, s.lnf.bias]]
        for b in reversed(s.blocks):
            segs.append([b.fc2.weight, b.fc2.bias, b.fc.weight, b.fc.bias, b.ln2.weight, b.ln2.bias,
                         b.proj.weight, b.proj.bias, b.qkv.weight, b.qkv.bias, b.ln1.weight, b.ln1.bias])
        segs.append([s.wpe.weight, s.wte.weight])
        return segs

    def _dgrad_sources(self):
        s = self.spec
        lins = [l for b in s.blocks for l in (b.qkv, b.proj, b.fc, b.fc2)]
        # the head's source (and so its transposed copy) covers its pad rows
        return [(s.head.weight, self.head_w)] + [(l.weight, partial(self.bf16, l.weight)) for l in lins]

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int, T: int):
        if self._acts_shape == (B, T):
            return
        s, dev = self.spec, self.device
        N, C, F, V = B * T, s.C, s.F, s.V
        bf, f32 = torch.bfloat16, torch.float32
        self.resid = [torch.empty(N, C, dtype=f32, device=dev) for _ in range(self.L + 1)]
        self.resid_mid = [torch.empty(N, C, dtype=f32, device=dev) for _ in range(self.L)]
        self.ln1 = [torch.empty(N, C, dtype=bf, device=dev) for _ in range(self.L)]
        self.ln2 = [torch.empty(N, C, dtype=bf, device=dev) for _ in range(self.L)]
        self.stats = [tuple(torch.empty(N, dtype=f32, device=dev) for _ in range(4)) for _ in range(self.L)]
        self.statsf = (torch.empty(N, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev))
        self.qkv = [torch.empty(N, 3 * C, dtype=bf, device=dev) for _ in range(self.L)]
        self.att = [torch.empty(N, C, dtype=bf, device=dev) for _ in range(self.L)]
        self.lse = [torch.empty(B, s.H, T, dtype=f32, device=dev) for _ in range(self.L)]
        self.fcpre = [torch.empty(N, F, dtype=bf, device=dev) for _ in range(self.L)]
        self.fcact = [torch.empty(N, F, dtype=bf, device=dev) for _ in range(self.L)]
        self.lnf_out = torch.empty(N, C, dtype=bf, device=dev)
        self._alloc_head(N)
        self.tmp_c = torch.empty(N, C, dtype=bf, device=dev)
        self.dresid = torch.empty(N, C, dtype=f32, device=dev)
        # gradient buffers read by the side-stream weight-gradient GEMMs rotate between two
        # copies, so the main stream can produce the next one while the side stream still reads
        self.dresid_bf2 = [torch.empty(N, C, dtype=bf, device=dev) for _ in range(2)]
        self.d_f2 = [torch.empty(N, F, dtype=bf, device=dev) for _ in range(2)]
        self.dqkv2 = [torch.empty(N, 3 * C, dtype=bf, device=dev) for _ in range(2)]
        self.d_c = torch.empty(N, C, dtype=bf, device=dev)
        self._acts_shape = (B, T)

    def free_buffers(self):
        for name in ("resid", "resid_mid", "ln1", "ln2", "qkv", "fcpre", "fcact", "lnf_out", "_head_bufs", "tmp_c",
                     "dresid", "dresid_bf2", "d_f2", "d_c", "dqkv2", "att", "lse", "stats", "statsf"):
            if hasattr(self, name):
                delattr(self, name)
        self._acts_shape = None

    # ------------------------------------------------------------------ forward
    def _linear(self, x: Tensor, lin: nn.Linear, out: Tensor | None = None) -> Tensor:
        w = self.bf16(lin.weight)
        if lin.bias is not None:
            return torch.addmm(self.bf16(lin.bias), x, w.t(), out=out) if out is not None else \
                torch.addmm(self.bf16(lin.bias), x, w.t())
        return torch.mm(x, w.t(), out=out) if out is not None else torch.mm(x, w.t())

    def _drop(self, training: bool, seed: int, l: int, branch: int) -> tuple[float, int]:
        """(p, mask seed) of residual-dropout site (layer l, branch 0 = attention / 1 = MLP)."""
        b = self.spec.blocks[l]
        p = (b.p_attn_res if branch == 0 else b.p_mlp_res) if training else 0.0
        return p, _site_seed(seed, 2 * l + branch)

    def _forward(self, idx: Tensor, training: bool, dropout_seed: int = 0):
        """Embedding … final LayerNorm (``self.lnf_out``); the lm_head runs in ``_head_*``."""
        s = self.spec
        B, T = idx.shape
        if T > s.P:
            raise ValueError(f"sequence length {T} exceeds the position table {s.P}")
        self._alloc(B, T)
        H, D, C = s.H, s.D, s.C
        f = self.f32
        fused_ops.embedding_fwd(idx, f(s.wte.weight), f(s.wpe.weight), s.wpe.position_offset, out=self.resid[0],
                                dropout_p=s.p_embd if training else 0.0,
                                dropout_seed=_site_seed(dropout_seed, -1))
        for l, b in enumerate(s.blocks):
            mean1, rstd1, mean2, rstd2 = self.stats[l]
            if l == 0:
                norm_ops.ln_fwd(self.resid[0], f(b.ln1.weight), f(b.ln1.bias), b.ln1.eps, y=self.ln1[0],
                                mean=mean1, rstd=rstd1)
            else:  # resid[l] = resid_mid[l-1] + drop(fc2(l-1)), LN1(l) in the same pass
                dp, ds = self._drop(training, dropout_seed, l - 1, 1)
                norm_ops.add_ln_fwd(self.resid_mid[l - 1], self.tmp_c, self.resid[l], f(b.ln1.weight),
                                    f(b.ln1.bias), b.ln1.eps, y=self.ln1[l], mean=mean1, rstd=rstd1,
                                    dropout_p=dp, dropout_seed=ds)
            self._linear(self.ln1[l], b.qkv, out=self.qkv[l])
            p = b.attn.dropout if training else 0.0
            attn_ops.flash_fwd(self.qkv[l].view(B, T, 3 * C), H, H, D, p, dropout_seed + l,
                               out=self.att[l].view(B, T, C), lse=self.lse[l])
            self._linear(self.att[l], b.proj, out=self.tmp_c)
            dp, ds = self._drop(training, dropout_seed, l, 0)
            norm_ops.add_ln_fwd(self.resid[l], self.tmp_c, self.resid_mid[l], f(b.ln2.weight), f(b.ln2.bias),
                                b.ln2.eps, y=self.ln2[l], mean=mean2, rstd=rstd2, dropout_p=dp, dropout_seed=ds)
            # fc: library GEMM + bias into the pre-activation, then the HIP GELU kernel writes the
            # activation (ops/gemm.py linear_gelu); the backward's dgrad_gelu is a library GEMM
            # followed by one GELU-backward + fc-bias column-sum kernel
            gemm_ops.linear_gelu(self.ln2[l], self.bf16(b.fc.weight), self.bf16(b.fc.bias), self.fcpre[l],
                                 self.fcact[l], s.gelu_approx)
            self._linear(self.fcact[l], b.fc2, out=self.tmp_c)
        Lc = self.L
        meanf, rstdf = self.statsf
        dp, ds = self._drop(training, dropout_seed, Lc - 1, 1)
        norm_ops.add_ln_fwd(self.resid_mid[Lc - 1], self.tmp_c, self.resid[Lc], f(s.lnf.weight), f(s.lnf.bias),
                            s.lnf.eps, y=self.lnf_out, mean=meanf, rstd=rstdf, dropout_p=dp, dropout_seed=ds)

    def _train_micro_step(self, idx: Tensor, targets: Tensor, scale: float, sync: bool, capture: bool) -> Tensor:
        s = self.spec
        B, T = idx.shape
        N, C = B * T, s.C
        seed = self._step_seed
        self._step_seed += 1000
        self._refresh_transposed()
        with trace_range("forward"):
            self._forward(idx, training=True, dropout_seed=seed)
        cap = capture and self._captured is None
        # ---- head, per token chunk: lm_head GEMM, CE (in place -> dlogits), dgrad, wgrad
        head_range = trace_range("backward.head")
        head_range.__enter__()
        self._defer_reductions(True)
        tg = targets.reshape(-1)
        V, full = s.V, None
        if cap:  # diagnostics want the whole logits / dlogits tensors: one transient chunk
            full = self._full_logits(padded=True)
            acts = [self.resid[0].view(B, T, C).clone()] * 2 + [r.view(B, T, C).clone() for r in self.resid[1:]] + \
                   [self.lnf_out.view(B, T, C).float().clone(), full[:, :V].reshape(B, T, V).clone()]
        loss = self._head_backward(tg, scale, N, full)
        mean, rstd = self.statsf
        last = s.blocks[-1]
        rb = 0  # rotating dresid_bf buffer index
        dp, ds = self._drop(True, seed, self.L - 1, 1)
        norm_ops.ln_bwd(self.d_c, self.resid[self.L], mean, rstd, self.f32(s.lnf.weight), self.dresid, False,
                        self._reuse(self.dresid_bf2[rb]), self.grad(s.lnf.weight), self.grad(s.lnf.bias),
                        self.grad(last.fc2.bias), dropout_p=dp, dropout_seed=ds)
        grads_cap = []
        if cap:
            grads_cap = [full[:, :V].reshape(B, T, V).clone(), self.d_c.view(B, T, C).float().clone(),
                         self.dresid.view(B, T, C).clone()]
        self._segment_done(0, sync)
        head_range.__exit__(None, None, None)
        for l in range(self.L - 1, -1, -1):
            layer_range = trace_range(f"backward.block{l}")
            layer_range.__enter__()
            b = s.blocks[l]
            d_f, dqkv = self._reuse(self.d_f2[l & 1]), self._reuse(self.dqkv2[l & 1])
            dres_bf = self.dresid_bf2[rb]
            # ---- MLP branch
            # fc2 data gradient, GELU backward and the fc bias gradient in one kernel (ops/gemm.py)
            gemm_ops.dgrad_gelu(dres_bf, self._dgrad_w(b.fc2.weight).t(), self.fcpre[l], d_f, self.grad(b.fc.bias),
                                s.gelu_approx)
            self._wgrad(dres_bf, self.fcact[l], b.fc2.weight)
            torch.mm(d_f, self._dgrad_w(b.fc.weight), out=self.d_c)
            self._wgrad(d_f, self.ln2[l], b.fc.weight)
            _, _, mean, rstd = self.stats[l]
            rb ^= 1
            dres_bf = self._reuse(self.dresid_bf2[rb])
            dp, ds = self._drop(True, seed, l, 0)
            norm_ops.ln_bwd(self.d_c, self.resid_mid[l], mean, rstd, self.f32(b.ln2.weight), self.dresid, True,
                            dres_bf, self.grad(b.ln2.weight), self.grad(b.ln2.bias), self.grad(b.proj.bias),
                            dropout_p=dp, dropout_seed=ds)
            # ---- attention branch
            torch.mm(dres_bf, self._dgrad_w(b.proj.weight), out=self.d_c)
            self._wgrad(dres_bf, self.att[l], b.proj.weight)
            # the qkv bias gradient comes out of the attention-backward epilogues (partials finished
            # on the side stream by the deferred reduction)
            attn_ops.flash_bwd(self.d_c.view(B, T, C), self.qkv[l].view(B, T, 3 * C), self.att[l].view(B, T, C),
                               self.lse[l], s.H, s.H, s.D, b.attn.dropout, seed + l, dqkv=dqkv.view(B, T, 3 * C),
                               dbias=self.grad(b.qkv.bias))
            torch.mm(dqkv, self._dgrad_w(b.qkv.weight), out=self.d_c)
            self._wgrad(dqkv, self.ln1[l], b.qkv.weight)
            mean, rstd, _, _ = self.stats[l]
            prev_bias = self.grad(s.blocks[l - 1].fc2.bias) if l > 0 else None
            rb ^= 1
            dp, ds = self._drop(True, seed, l - 1, 1) if l > 0 else (0.0, 0)
            norm_ops.ln_bwd(self.d_c, self.resid[l], mean, rstd, self.f32(b.ln1.weight), self.dresid, True,
                            self._reuse(self.dresid_bf2[rb]) if l > 0 else None, self.grad(b.ln1.weight),
                            self.grad(b.ln1.bias), prev_bias, dropout_p=dp, dropout_seed=ds)
            if cap:
                grads_cap.append(self.dresid.view(B, T, C).clone())
            self._segment_done(self.L - l, sync)
            layer_range.__exit__(None, None, None)
        fused_ops.embedding_bwd(self.dresid, idx, self.grad(s.wte.weight), self.grad(s.wpe.weight),
                                s.wpe.position_offset, dropout_p=s.p_embd, dropout_seed=_site_seed(seed, -1))
        self._segment_done(self.L + 1, sync)
        self._finish_backward(sync, cap)
        if cap:
            # grads_cap: [dlogits, d_lnf, d_resid[L], d_resid[L-1], ..., d_resid[0]]
            dlog, dlnf, dres = grads_cap[0], grads_cap[1], grads_cap[2:]
            dres = list(reversed(dres))  # d_resid[0] ... d_resid[L]
            act_grads = [dres[0], dres[0]] + dres[1:] + [dlnf, dlog]
            self._set_captured(acts, act_grads)
        return loss
