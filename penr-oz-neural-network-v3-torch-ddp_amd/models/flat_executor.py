"""The model-independent half of the fused training executors for MI355X.

:class:`FlatExecutor` is the base of :class:`penroz.models.executor.GPTExecutor` and
:class:`penroz.models.gemma_executor.GemmaExecutor`. It owns everything that does not depend on the
block structure of the model:

* the flat fp32 / gradient / bf16-shadow buffers, laid out in backward completion order, and the
  lm_head's zero pad rows;
* the transposed bf16 weight copies the data-gradient GEMMs read;
* the lm_head: logits, evaluation loss, and the chunked lm_head → cross-entropy → dgrad → wgrad loop
  of the backward;
* the weight-gradient side stream and its buffer-reuse events, the gradient ranges ``zero_grad``
  may leave alone, the per-segment / per-bucket optimizer inside the backward, the gradient
  reducer's tail, ``optimizer_step`` and gradient clipping by global norm (``set_grad_clip``).

A subclass supplies the model: ``PATTERN`` and ``match`` (layer list → spec, or None; the spec has
``V``, ``C``, ``head``, ``blocks`` and ``param_dtype``), ``_param_order`` (the parameters per
segment, in backward completion order, the lm_head weight first), ``_dgrad_sources``, ``_alloc``
/ ``free_buffers``, ``_forward`` (leaves the final norm's bf16 output in ``self.lnf_out``) and
``_train_micro_step`` (calls ``_head_backward``, which leaves the gradient of ``lnf_out`` in
``self.d_c``, then walks its blocks calling ``_segment_done`` after each segment, and ends with
``_finish_backward``). Every piece of instance state is created in ``__init__`` or in one of the
``_init_*`` methods it calls.
"""
from __future__ import annotations

import logging
import os

import torch
from torch import Tensor

from penroz.ops import fused as fused_ops
from penroz.ops import gemm as gemm_ops
from penroz.ops import grad_clip as grad_clip_ops
from penroz.utils.profiling import trace_range
from penroz.ops import _ext

log = logging.getLogger(__name__)


def _head_chunk_rows(N: int, V: int) -> int:
    """Token rows per lm_head/CE chunk.

    ``PENROZ_HEAD_CHUNK`` = rows (0 = one chunk of all N rows). Unset: one chunk while the bf16
    [N, V] logits fit in ``PENROZ_HEAD_CHUNK_AUTO_GB`` (default 8 GiB), else chunks of ≈ 2 GiB.
    Chunking trades time for memory on MI355X (GPT-2 124M headline, N = 65 536:
    ``profiles/head_chunk_r2_sweep.log``): 67.7 ms/step unchunked, 68.7 at 16 384 rows, 69.1 at
    8 192, 76.3 at 4 096 (per-chunk wgrad accumulation and untuned GEMM shapes), while the 6.6 GB
    logits are < 3 % of the 288 GB HBM, so the full tensor stays the default at that size.
    """
    env = os.environ.get("PENROZ_HEAD_CHUNK")
    if env is not None:
        c = int(env)
    else:
        row_bytes = ((V + 7) // 8 * 8) * 2
        limit = float(os.environ.get("PENROZ_HEAD_CHUNK_AUTO_GB", "8")) * 2**30
        c = 0 if N * row_bytes <= limit else max(1024, int(2 * 2**30 // row_bytes) // 1024 * 1024)
    return N if c <= 0 or c >= N else c


# residual-dropout mask streams: one per (step seed, site); attention dropout uses seed + layer
def _site_seed(seed: int, site: int) -> int:
    return (seed * 1_000_003 + 7_919 * (site + 1) + 0x5BD1E995) & 0x7FFFFFFFFFFFFFFF


def _minus(ranges, cut):
    """[(a, b)] ranges with the range ``cut`` (or None) removed."""
    if cut is None:
        return list(ranges)
    c0, c1 = cut
    out = []
    for a, b in ranges:
        if a < c0:
            out.append((a, min(b, c0)))
        if b > c1:
            out.append((max(a, c1), b))
    return [(a, b) for a, b in out if b > a]


def cu_mask_words(spec: str, n_cu: int) -> list[int]:
    """CU mask words for PENROZ_SIDE_CUS: ``stride:k[:o]`` = CUs i with i % k == o, ``first:n`` =
    CUs 0..n-1 (bit i of word i // 32 = CU i)."""
    kind, _, rest = spec.partition(":")
    if kind == "stride":
        k, _, o = rest.partition(":")
        sel = [i for i in range(n_cu) if i % int(k) == int(o or 0)]
    elif kind == "first":
        sel = list(range(min(int(rest), n_cu)))
    else:
        raise ValueError(f"PENROZ_SIDE_CUS: want stride:k[:o] or first:n, got {spec!r}")
    if not sel:
        raise ValueError(f"PENROZ_SIDE_CUS={spec!r} selects no CU")
    words = [0] * ((n_cu + 31) // 32)
    for i in sel:
        words[i // 32] |= 1 << (i % 32)
    return words


def _cu_masked_stream(device: torch.device, spec: str):
    """The side stream confined to a CU subset (A/B of critical-path GEMM interference)."""
    k = _ext.kernels()
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ptr = k.cu_masked_stream(idx, cu_mask_words(spec, k.cu_count(idx)))
    return torch.cuda.ExternalStream(ptr, device=device)


_HP_STREAMS: dict = {}
_SHARED_STREAMS: dict = {}


def shared_stream(device: torch.device, role: str):
    """ONE stream per (device, role) for the whole process — the executors' weight-gradient side
    stream ("side"), the per-bucket optimizer stream ("opt") and the input-copy stream ("copy").
    Every extra stream drawn from torch's pool is mapped onto one of the device's few hardware
    queues (GPU_MAX_HW_QUEUES = 4), and which streams end up sharing a queue depends on how many
    were drawn before: a copy stream created before a second model's executor cut that model's
    step from 0.98 to 0.88 of the first's (bench.py --via-runtime, profiles/notes_r6.md). Shared
    streams keep a later executor on the first one's queues; sharing only adds ordering."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _SHARED_STREAMS.get((idx, role))
    if st is None:
        st = _SHARED_STREAMS[(idx, role)] = torch.cuda.Stream(device=torch.device("cuda", idx))
    return st


def _high_priority_stream(device: torch.device):
    """ONE high-priority stream per device for every executor of the process. A second executor
    drawing a second stream from torch's high-priority pool (a later model in the same process —
    the server's worker, bench.py --via-runtime) ran the headline step at 65.4-65.5 ms instead of
    61.2-61.3: the second stream does not get the first one's queue priority, and the side stream's
    weight-gradient GEMMs then delay the dgrad chain (11 main-queue stalls of 0.3-0.56 ms before
    LayerNorm backward per step); with PENROZ_MAIN_PRIORITY=0 the second run matched the first
    (bench/runtime_ab.py, profiles/notes_r6.md). Sharing the stream only adds ordering between
    executors, never removes it."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    hp = _HP_STREAMS.get(idx)
    if hp is None:
        lo, hi = torch.cuda.Stream.priority_range()
        hp = _HP_STREAMS[idx] = torch.cuda.Stream(device=torch.device("cuda", idx), priority=min(lo, hi))
    return hp


class FlatExecutor:
    PATTERN = ""  # the subclass's layer pattern, as named in the "does not match" error

    # ------------------------------------------------------------------ setup
    def __init__(self, model, device):
        spec = self.match(model)
        if spec is None:
            raise ValueError(f"model does not match the {self.PATTERN} pattern")
        _ext.kernels()  # hard requirement on GPU
        if device.type == "cuda":
            gemm_ops.load_tuned_gemms()
        self.model = model
        self.spec = spec
        self.device = device
        self.L = len(spec.blocks)
        self._flatten()
        self._acts_shape = None
        self._captured = None
        self._step_seed = 0
        self._init_wgrad_state()
        self._init_optimizer_state()
        self._side_init()
        self._init_model_state()

    def _init_wgrad_state(self):
        """What ``zero_grad`` and the weight-gradient writes know about the flat gradient buffer."""
        self._wgrad_ranges = {}             # key -> flat range its wgrad GEMM writes (first backward)
        self._ranges_learned = False
        self._wgrad_ranges_invalid = False  # the writes are no partition / changed after learning
        self._zero_gaps = None              # the ranges zero_grad clears once the rest is overwritten
        self._zero_views, self._zero_views_key = None, None
        self._zero_skip = None              # a range the last backward left all-zero itself
        self._stale = {}                    # key -> parts zero_grad skipped, not yet written this step
        self._micro_since_zero = 0

    def _init_optimizer_state(self):
        """The gradient reducer and how the optimizer step overlaps the backward."""
        self.reducer = None
        self._ready_at = {}                 # segment index -> buckets complete after it
        self._reduce_pending = False
        self._overlap_opt = os.environ.get("PENROZ_OVERLAP_OPT", "1") != "0"
        self._opt_apply, self._opt_done = None, False
        self._opt_bucketed, self._opt_buckets_done = False, set()
        self._opt_mode = None
        # drawn at first use: which hardware queue a stream gets depends on how many came before
        self._opt_stream = None
        self._hp_stream = None
        # gradient clipping by global norm (set_grad_clip): the bound, and (norm, coef) on the device
        self._clip = None
        self._clip_out = None

    def _init_model_state(self):
        """The subclass's own state (Gemma: rope tables, the row-split embedding step)."""

    def _flatten(self):
        """Re-point every parameter at a view of flat fp32 / grad / bf16-shadow buffers."""
        segs = self._param_order()
        params = [p for seg in segs for p in seg]
        if len({id(p) for p in params}) != len(params) or len(params) != len(list(self.model.parameters())):
            raise ValueError("executor needs every parameter exactly once (no tying)")
        # zero rows after the lm_head weight (V rounded up to HEAD_PAD): the head GEMMs run at the
        # padded width (the logit rows are padded anyway), the pad rows stay zero (zero gradient,
        # zero update) and the state_dict sees only the first V rows. Decided once, here: every
        # later slice of the flat buffers (Vp, head_w, head_grad, the logit stride) uses this value
        self._head_pad = self._head_pad_policy()
        pad = {id(self.spec.head.weight): self._head_pad * self.spec.C} if self._head_pad else {}
        total = sum(p.numel() + pad.get(id(p), 0) for p in params)
        dev = self.device
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.shadow = torch.empty(total, dtype=torch.bfloat16, device=dev)
        self.offsets = {}
        self.segments = []
        bf16_params = self.spec.param_dtype == torch.bfloat16
        off = 0
        for seg in segs:
            start = off
            for p in seg:
                n = p.numel()
                self.flat[off:off + n].copy_(p.data.reshape(-1))
                if bf16_params:
                    # the module sees the bf16 shadow (rewritten by every optimizer step); the
                    # fp32 masters and gradients stay internal (grad(p) / f32(p))
                    p.data = self.shadow[off:off + n].view_as(p)
                else:
                    p.data = self.flat[off:off + n].view_as(p)
                    p.grad = self.flat_grad[off:off + n].view_as(p)
                self.offsets[id(p)] = off
                off += n
                if pad.get(id(p)):
                    self.flat[off:off + pad[id(p)]].zero_()
                    off += pad[id(p)]
            self.segments.append((start, off))
        self.params_in_order = params
        self._init_transposed()
        self.refresh_shadow()
        opt = self.model.optimizer
        if hasattr(opt, "attach_flat") and len(opt.param_groups) == 1:
            opt.attach_flat(params, self.flat, self.flat_grad, self.shadow, [self.offsets[id(p)] for p in params])
            self._opt_flat = True
        else:
            self._opt_flat = False

    # the lm_head weight's rows are padded to a multiple of this (HF GPT-2 V = 50257 -> 50304, the
    # headline's width: hipBLASLt ran the 50257-wide lm_head forward 1.7 ms slower per step, and the
    # transposed dgrad copy needs widths % 64; profiles/notes_r6.md). PENROZ_HEAD_PAD=0: off
    HEAD_PAD = 128

    def _head_pad_policy(self) -> int:
        """Pad rows for a new flat layout (read by ``_flatten`` alone)."""
        m = int(os.environ.get("PENROZ_HEAD_PAD", self.HEAD_PAD))
        return (-self.spec.V) % m if m > 0 and self.device.type == "cuda" else 0

    def head_pad_rows(self) -> int:
        return self._head_pad

    @property
    def Vp(self) -> int:
        """Rows of the padded lm_head weight (= logit columns the head GEMMs produce)."""
        return self.spec.V + self._head_pad

    def head_w(self) -> Tensor:
        """The bf16 lm_head weight with its zero pad rows, [Vp, C]."""
        off = self.offsets[id(self.spec.head.weight)]
        return self.shadow[off:off + self.Vp * self.spec.C].view(self.Vp, self.spec.C)

    def head_grad(self) -> Tensor:
        off = self.offsets[id(self.spec.head.weight)]
        return self.flat_grad[off:off + self.Vp * self.spec.C].view(self.Vp, self.spec.C)

    def refresh_shadow(self):
        self.shadow.copy_(self.flat)
        # a shadow rebuilt outside the fused optimizer (a new session, weights loaded) makes every
        # transposed dgrad copy stale, including those rebuilt after the last segment AdamW pass
        self._t_fresh.clear()

    def bf16(self, p: Tensor) -> Tensor:
        off = self.offsets[id(p)]
        return self.shadow[off:off + p.numel()].view(p.shape)

    def grad(self, p: Tensor) -> Tensor:
        off = self.offsets[id(p)]
        return self.flat_grad[off:off + p.numel()].view(p.shape)

    def f32(self, p: Tensor) -> Tensor:
        """The fp32 master of ``p`` (``p`` itself for fp32 models)."""
        off = self.offsets[id(p)]
        return self.flat[off:off + p.numel()].view(p.shape)

    # ---- transposed bf16 weight copies for the data-gradient GEMMs ----------------------------
    # dx = dy·W with W [out, in] as stored reaches 0.94-1.32 PF on hipBLASLt at GPT-2 shapes; with
    # W transposed ([in, out], so both operands are reduction-contiguous as in the forward) it
    # reaches 1.11-1.53 PF (profiles/dgrad_layout_r1.log). With the optimizer fused into the
    # backward, a segment's copies are rebuilt right after its optimizer pass on the side stream
    # (overlapping the rest of the backward; _t_fresh); otherwise — and for anything not yet
    # rebuilt — at the start of the micro-step on the side stream, and the backward's first dgrad
    # waits for them (Gemma-3 1B: the 1.1 ms of transposes sat between the step's last AdamW pass
    # and the next forward, profiles/notes_r5.md). PENROZ_DGRAD_T=0: off.
    def _init_transposed(self):
        """``_dgrad_src``: id(key parameter) -> function returning the bf16 [out, in] weight, for
        every ``_dgrad_sources`` entry; ``_tw``: the same key -> (that function, its transposed
        copy [in, out] in ``shadow_t``) for the weights whose two widths are multiples of 64."""
        self._dgrad_src = {id(p): f for p, f in self._dgrad_sources()}
        self._tw, self._t_ready, self._t_fresh = {}, None, set()
        if self.device.type != "cuda" or os.environ.get("PENROZ_DGRAD_T", "1") == "0" or not _ext.available():
            return
        srcs = [(k, f) for k, f in self._dgrad_src.items() if f().shape[0] % 64 == 0 and f().shape[1] % 64 == 0]
        self.shadow_t = torch.empty(sum(f().numel() for _, f in srcs), dtype=torch.bfloat16, device=self.device)
        off = 0
        for key, f in srcs:
            r, c = f().shape
            self._tw[key] = (f, self.shadow_t[off:off + r * c].view(c, r))
            off += r * c

    def _refresh_transposed(self):
        if not self._tw:
            return
        k = _ext.kernels()
        todo = [e for key, e in self._tw.items() if key not in self._t_fresh]
        self._t_fresh.clear()
        if self._side is None:
            for f, t in todo:
                k.transpose_bf16(f(), t)
            return
        if not todo:  # all rebuilt after their segments' optimizer passes (the main stream joined)
            return
        # the copies must see this step's weights: the side stream waits for everything the main
        # stream has queued (the optimizer's shadow refresh). The main stream is captured BEFORE
        # entering the side-stream context — inside it, current_stream() IS the side stream, and
        # waiting on it orders nothing (that was a race: transposes of a half-refreshed shadow)
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._side):
            self._side.wait_stream(main)
            for f, t in todo:
                k.transpose_bf16(f(), t)
            self._t_ready = torch.cuda.Event()
            self._t_ready.record(self._side)

    # rebuild a segment's transposed copies right after its optimizer pass: Gemma-3 1B B=8 −0.2 to
    # −0.3 ms, Gemma-4 e2b −0.4 ms; GPT-2 +0.16 / +0.19 ms (its start-of-step transposes already
    # overlap the forward), so the copies are rebuilt at the step start
    SEGMENT_TRANSPOSE = False

    def _transpose_segment(self, s: int, e: int):
        """Rebuild the transposed dgrad copies of the parameters in flat range [s, e) on the current
        stream, right after that range's optimizer pass (their shadow is final for the next step)."""
        env = os.environ.get("PENROZ_SEGMENT_TRANSPOSE")  # (A/B: 1 / 0 overrides the class default)
        if not self._tw or not (self.SEGMENT_TRANSPOSE if env is None else env == "1"):
            return
        k = _ext.kernels()
        for key, (f, t) in self._tw.items():
            off = self.offsets.get(key)
            if off is not None and s <= off and off + t.numel() <= e:  # the whole weight is final
                k.transpose_bf16(f(), t)
                self._t_fresh.add(key)

    def _dgrad_w(self, key_param: Tensor) -> Tensor:
        """The weight operand of dx = dy·W for the ``_dgrad_sources`` entry of ``key_param``: the
        transposed copy (viewed back as [out, in]) or, without one, the source itself."""
        tw = self._tw.get(id(key_param))
        if tw is None:
            return self._dgrad_src[id(key_param)]()
        if self._t_ready is not None:
            torch.cuda.current_stream(self.device).wait_event(self._t_ready)
            self._t_ready = None
        return tw[1].t()

    # ------------------------------------------------------------------ lm_head
    def _alloc_head(self, N: int):
        """The logits buffers, rows padded to a multiple of 8 elements (``_logit_ld``). Training:
        two rotating [chunk, ld] buffers (lm_head → CE → dgrad/wgrad per token chunk); the full
        [N, ld] logits only exist transiently for logits_for / diagnostics captures."""
        self.head_chunk = _head_chunk_rows(N, self.spec.V)
        self._head_bufs = [torch.empty(self.head_chunk, self._logit_ld(), dtype=torch.bfloat16, device=self.device)
                           for _ in range(2 if self.head_chunk < N else 1)]

    def _logit_ld(self) -> int:
        """Row stride of the logits buffers: the padded head width, and a multiple of 8 elements
        (16 B: the GEMMs take the stride, the CE kernel's 16-B chunks stay inside the row; HF GPT-2
        unpadded: V = 50257 -> stride 50264)."""
        return (self.Vp + 7) // 8 * 8

    def _head_logits(self, r0: int, r1: int, buf: Tensor) -> Tensor:
        """lm_head GEMM of token rows [r0, r1) into ``buf`` ([rows, ld]); returns the [rows, Vp]
        view (columns V..Vp-1 are the pad rows' exact zeros; slice [:, :V] for the logits)."""
        lg = buf[: r1 - r0, : self.Vp]
        torch.mm(self.lnf_out[r0:r1], self.head_w().t(), out=lg)
        return lg

    def _full_logits(self, padded: bool = False) -> Tensor:
        N = self.lnf_out.shape[0]
        buf = torch.empty(N, self._logit_ld(), dtype=torch.bfloat16, device=self.device)
        lg = self._head_logits(0, N, buf)
        return lg if padded else lg[:, : self.spec.V]

    def _head_backward(self, tg: Tensor, scale: float, N: int, full: Tensor | None = None) -> Tensor:
        """The head of the backward, per token chunk: lm_head GEMM, CE (in place -> dlogits), dgrad
        into ``self.d_c``, wgrad. ``full`` (diagnostics captures, which want the whole logits /
        dlogits tensors): the padded [N, Vp] logits as one transient chunk. Returns the scaled loss."""
        V, head = self.spec.V, self.spec.head.weight
        if full is not None:
            chunks = [(0, N, full)]
        else:
            chunks = [(r0, min(N, r0 + self.head_chunk), None) for r0 in range(0, N, self.head_chunk)]
        loss = torch.zeros((), dtype=torch.float32, device=self.device)
        w_dgrad = self._dgrad_w(head)
        for i, (r0, r1, lg) in enumerate(chunks):
            if lg is None:  # the side stream may still be reading this buffer (wgrad two chunks back)
                lg = self._head_logits(r0, r1, self._reuse(self._head_bufs[i % len(self._head_bufs)]))
            # CE rewrites the V real columns with dlogits; the pad columns stay the exact zeros of
            # the pad rows, so the padded dgrad / wgrad equal the unpadded ones (pad rows get 0)
            loss += fused_ops.cross_entropy_fwd_bwd(lg[:, :V], tg[r0:r1], scale / N).sum()
            torch.mm(lg[:, : w_dgrad.shape[0]], w_dgrad, out=self.d_c[r0:r1])
            self._wgrad_into(id(head), lg, self.lnf_out[r0:r1], self.head_grad())
        loss *= scale / N
        return loss

    # ------------------------------------------------------------------ public API
    @torch.no_grad()
    def eval_loss(self, idx: Tensor, targets: Tensor) -> Tensor:
        self._forward(idx, training=False)
        N, tg = self.lnf_out.shape[0], targets.reshape(-1)
        total = torch.zeros((), dtype=torch.float32, device=self.device)
        for r0 in range(0, N, self.head_chunk):
            r1 = min(N, r0 + self.head_chunk)
            total += fused_ops.cross_entropy_fwd_bwd(self._head_logits(r0, r1, self._head_bufs[0])[:, : self.spec.V],
                                                     tg[r0:r1], 0.0).sum()
        return total / N

    @torch.no_grad()
    def logits_for(self, idx: Tensor) -> Tensor:
        self._forward(idx, training=False)
        return self._full_logits().view(idx.shape[0], idx.shape[1], -1)

    # the last bucket (wpe + wte: 157 MB fp32 at GPT-2 124M, produced by the backward's final
    # kernel) is cut into this many pieces so its all-reduce pipelines with the optimizer passes of
    # the pieces already landed (PENROZ_TAIL_PIECES)
    TAIL_PIECES = 4

    def setup_training(self, distributed: bool):
        from penroz.parallel.reducer import GradReducer, plan_buckets, default_bucket_mb, ready_map, split_last_bucket
        import torch.distributed as dist
        self.refresh_shadow()
        self.reducer = None
        if distributed and dist.is_initialized() and dist.get_world_size() > 1:
            buckets = plan_buckets(self.segments, default_bucket_mb(dist.get_backend()) * 2**20)
            buckets = split_last_bucket(buckets, int(os.environ.get("PENROZ_TAIL_PIECES", self.TAIL_PIECES)))
            self.reducer = GradReducer(self.flat_grad, buckets)
            self.reducer.broadcast_params(self.flat)
            self.refresh_shadow()
            self._ready_at = ready_map(buckets, self.segments)

    def _per_bucket_opt_ok(self) -> bool:
        """World > 1: apply the fused AdamW to each gradient bucket inside the backward, on its own
        stream, as soon as that bucket's all-reduce has landed (PENROZ_OPT_PER_BUCKET=1 forces it on
        a host-blocking transport such as gloo, 0 disables it)."""
        env = os.environ.get("PENROZ_OPT_PER_BUCKET")
        if env == "0" or self.device.type != "cuda" or not self._buckets_tile_flat():
            return False
        return env == "1" or self.reducer.stream_waits()

    def opt_overlap_mode(self) -> str:
        """How the optimizer step overlaps the backward (reported by bench.py in ``comm``)."""
        if self._clip is not None:
            return "after-backward-clipped"
        return self._opt_mode or "none"

    def set_grad_clip(self, max_norm: float | None):
        """Clip the gradients by their global L2 norm in every following step (``ops/grad_clip.py``
        has the definition; None: off, the schedule and the results of the unclipped executor).

        The norm exists only once every gradient is final and all-reduced, so with a bound the
        optimizer does not run inside the backward: ``train_micro_step(fuse_optimizer=True)`` starts
        no per-segment, per-bucket or row-split step, and ``optimizer_step`` waits for the
        outstanding buckets, computes (norm, coef) over the whole flat gradient buffer on the
        device, and applies the flat fused step with the coefficient read from the device; the
        transposed dgrad copies are rebuilt at the next step's start. Without a flat fused optimizer
        the gradient buffer is multiplied by the coefficient in place before ``opt.step()``.

        Unlike torch's, the flat fused step does not write the gradient: ``flat_grad`` (and the
        dashboard's gradient statistics) keep the unclipped values. ``last_grad_norm`` /
        ``last_clip_coef`` are device views of the last step's result; nothing here reads them on
        the host."""
        self._clip = grad_clip_ops.check_max_grad_norm(max_norm)
        if self._clip is None:
            self._clip_out = None
        elif self._clip_out is None:
            self._clip_out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.device)

    @property
    def last_grad_norm(self) -> Tensor | None:
        """The last clipped step's pre-clip gradient norm, fp32 [] on the device (None: off)."""
        return None if self._clip_out is None else self._clip_out[0]

    @property
    def last_clip_coef(self) -> Tensor | None:
        """The last clipped step's coefficient min(1, max_norm / (norm + 1e-6)), fp32 [] on the device."""
        return None if self._clip_out is None else self._clip_out[1]

    def end_training(self):
        if self.reducer is not None:
            self.wait_gradients()
        self.reducer = None

    def zero_grad(self):
        """Zero the gradients. Once a backward has shown which flat ranges only the weight-gradient
        GEMMs write (the linear weights: most of the buffer), those are left alone and the first
        GEMM into each writes instead of accumulating (``gemm_ops.wgrad(accumulate=False)``), so
        the step neither clears them nor reads them back (PENROZ_GRAD_OVERWRITE=0: clear all)."""
        self.wait_gradients()
        # a flat range the last backward left all-zero itself (the Gemma row-split embedding step)
        skip, self._zero_skip = self._zero_skip, None
        self._micro_since_zero = 0
        if self._zero_gaps is not None:
            key = (self.flat_grad.data_ptr(), skip)
            if self._zero_views_key != key:  # views of THIS buffer
                self._zero_views = [self.flat_grad[a:b] for a, b in _minus(self._zero_gaps, skip)]
                self._zero_views_key = key
            torch._foreach_zero_(self._zero_views)
            self._stale = {k: [r] for k, r in self._wgrad_ranges.items()}
        else:
            for a, b in _minus([(0, self.flat_grad.numel())], skip):
                self.flat_grad[a:b].zero_()
            self._stale = {}
        self._captured = None

    def _learn_wgrad_ranges(self):
        """After the first backward: the flat ranges outside the weight-gradient GEMMs' outputs,
        as views for one multi-tensor zero (neighbouring ranges merged)."""
        self._zero_gaps = None
        if (os.environ.get("PENROZ_GRAD_OVERWRITE", "1") == "0" or self.device.type != "cuda"
                or not self._wgrad_ranges or self._wgrad_ranges_invalid):
            return
        covered = sorted(self._wgrad_ranges.values())
        gaps, pos = [], 0
        for s, e in covered:
            if s < pos:  # overlapping outputs: not a partition, keep clearing everything
                return
            if s > pos:
                gaps.append((pos, s))
            pos = e
        if pos < self.flat_grad.numel():
            gaps.append((pos, self.flat_grad.numel()))
        self._zero_gaps = gaps

    def _segment_done(self, seg_index: int, sync: bool):
        if self._opt_apply is not None and sync and self.reducer is None:
            # optimizer inside the backward: this segment's gradients are final once the side
            # stream (its weight gradients, deferred dγ / bias reductions) has caught up with the
            # main stream (its other gradients); nothing later in this backward reads its weights
            s, e = self.segments[seg_index]
            if self._side is None:
                self._opt_apply(s, e)
                self._transpose_segment(s, e)
                return
            main = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self._side):
                self._side.wait_stream(main)
                self._opt_apply(s, e)
                self._transpose_segment(s, e)
            return
        if self.reducer is None or not sync:
            return
        ready = self._ready_at.get(seg_index, ())
        if not ready:
            return
        if self._side is None:
            for i in ready:
                self.reducer.bucket_ready(i)
        else:
            # the bucket's weight gradients come from the side stream, its bias / LayerNorm
            # gradients from the main stream: launch the collective from the side stream after
            # it has caught up with the main stream
            main = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self._side):
                self._side.wait_stream(main)
                for i in ready:
                    self.reducer.bucket_ready(i)
        if self._opt_bucketed:
            self._opt_buckets(ready)

    def _opt_buckets(self, ids):
        """Per-bucket optimizer (world > 1): on the optimizer stream, wait for each bucket's
        all-reduce (a stream wait, not a host wait) and apply the fused AdamW to its range, then
        rebuild the transposed dgrad copies of the weights wholly inside it (Gemma). Nothing later
        in the backward reads the parameters of a finished segment; the main stream joins this
        stream before the step returns (the next forward reads the new weights)."""
        if self._opt_stream is None:
            self._opt_stream = shared_stream(self.device, "opt")
        with torch.cuda.stream(self._opt_stream):
            for i in ids:
                if i in self._opt_buckets_done:
                    continue
                s, e = self.reducer.wait_bucket(i)
                self._opt_apply(s, e)
                self._transpose_segment(s, e)
                self._opt_buckets_done.add(i)

    # ---- weight gradients on a side HIP stream -------------------------------------------------
    # The weight-gradient GEMMs and the finishing kernels of every dγ / dβ / bias column reduction
    # (the qkv bias partials come from the attention-backward epilogues) are off the backward's
    # critical path (nothing in the backward reads parameter gradients), so they run on a second
    # stream and overlap the main stream's dgrad GEMMs, LayerNorm / GELU backward, flash-attention
    # backward. Ordering: the side stream waits on an event recorded after each operand's producer;
    # before the main stream overwrites a rotating operand buffer it waits on the event recorded
    # after that buffer's last side-stream reader; gradient buckets are handed to the reducer from
    # the side stream (after it has also waited for the main stream's bias / LayerNorm gradients),
    # and the main stream joins the side stream before the step returns. PENROZ_WGRAD_STREAM=0 runs
    # everything on one stream (A/B).
    def _side_init(self):
        self._side = None
        if self.device.type == "cuda" and os.environ.get("PENROZ_WGRAD_STREAM", "1") != "0":
            cus = os.environ.get("PENROZ_SIDE_CUS", "")
            self._side = _cu_masked_stream(self.device, cus) if cus else shared_stream(self.device, "side")
        self._buf_free = {}

    def _side_call(self, operand: Tensor, fn):
        """Run ``fn`` (gradient-only work reading ``operand``) on the side stream, or inline."""
        if self._side is None:
            fn()
            return
        main = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            fn()
            done = torch.cuda.Event()
            done.record(self._side)
        self._buf_free[operand.data_ptr()] = done

    def _wgrad(self, dy: Tensor, x: Tensor, p: Tensor):
        self._wgrad_into(id(p), dy, x, self.grad(p))

    def _wgrad_into(self, key: int, dy: Tensor, x: Tensor, g: Tensor):
        """g (+)= dyᵀ·x on the side stream: the first write of a range that zero_grad left alone
        overwrites it; the ranges are recorded during the first backward (see zero_grad).

        ``_stale[key]`` holds the parts of the key's learned range that zero_grad skipped and no
        write of this step has touched yet. A write covering exactly the whole stale learned range
        overwrites it; any other write (e.g. a chunked wgrad writing sub-ranges under one key)
        first clears the stale parts it overlaps and accumulates; parts still stale at the end of
        the backward are cleared by :meth:`_finish_wgrad_bookkeeping`. A range pattern that differs
        from the learned one also makes zero_grad clear everything from the next step on."""
        rec = self._wgrad_ranges
        off = g.data_ptr() - self.flat_grad.data_ptr()
        rng = (off // 4, off // 4 + g.numel())
        if not self._ranges_learned:
            if rec.get(key, rng) != rng:  # one key, several sub-ranges: not a plain overwrite
                self._wgrad_ranges_invalid = True
            rec[key] = rng
        elif rec.get(key) != rng:
            self._wgrad_ranges_invalid = True
            self._zero_gaps = None
        stale = self._stale
        parts = stale.get(key)
        if parts and parts == [rng]:  # the whole learned range, untouched this step: overwrite
            del stale[key]
            self._side_call(dy, lambda: gemm_ops.wgrad(dy, x, g, False))
            return
        if parts:
            keep = []
            for s_, e_ in parts:
                a, b = max(s_, rng[0]), min(e_, rng[1])
                if a >= b:
                    keep.append((s_, e_))
                    continue
                view = self.flat_grad[a:b]
                self._side_call(dy, lambda v=view: v.zero_())
                if s_ < a:
                    keep.append((s_, a))
                if b < e_:
                    keep.append((b, e_))
            if keep:
                stale[key] = keep
            else:
                del stale[key]
        self._side_call(dy, lambda: gemm_ops.wgrad(dy, x, g, True))

    def _finish_wgrad_bookkeeping(self):
        """End of a backward: learn the ranges once; clear any part of a range zero_grad skipped
        that no GEMM wrote (not expected: every backward writes every linear weight's gradient)."""
        if not self._ranges_learned:
            self._ranges_learned = True
            self._learn_wgrad_ranges()
        stale = self._stale
        if stale:
            log.warning(f"weight-gradient ranges not written by this backward: {len(stale)}; clearing them")
            self._join_side()
            for parts in stale.values():
                for s_, e_ in parts:
                    self.flat_grad[s_:e_].zero_()
            stale.clear()

    def _defer_reductions(self, on: bool):
        """LayerNorm / bias column-reduction finishing kernels go to the side stream (on) or not."""
        if self._side is not None:
            _ext.kernels().set_deferred_reduce_stream(self._side.cuda_stream if on else 0, self.device.index or 0)

    def _reuse(self, buf: Tensor) -> Tensor:
        """Main stream: wait until the side stream no longer reads ``buf`` (before overwriting)."""
        ev = self._buf_free.pop(buf.data_ptr(), None) if self._side is not None else None
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return buf

    def _join_side(self):
        if self._side is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._side)
            self._buf_free.clear()

    @torch.no_grad()
    def train_micro_step(self, idx: Tensor, targets: Tensor, scale: float, sync: bool = True,
                         capture: bool = False, fuse_optimizer: bool = False) -> Tensor:
        """Forward + backward of one micro-batch; gradients accumulate into the flat buffer.
        Returns the (scaled) mean loss as a device scalar.

        ``fuse_optimizer`` (the last micro-step of a step whose ``optimizer_step`` follows, single
        process): the fused AdamW updates each parameter segment inside the backward, on the side
        stream, as soon as that segment's gradients are final — the optimizer pass overlaps the
        rest of the backward instead of running after it (``optimizer_step`` then has nothing left
        to do). ``PENROZ_OPT_IN_BWD=0`` keeps the separate step, and so does gradient clipping
        (``set_grad_clip``): the global norm needs every gradient first."""
        self._opt_apply = None
        self._opt_bucketed = False
        if (fuse_optimizer and sync and not capture and self._opt_flat and self._clip is None
                and os.environ.get("PENROZ_OPT_IN_BWD", "1") != "0"):
            if self.reducer is None:
                self._opt_apply = self.model.optimizer.begin_flat_ranges()
                self._opt_mode = "per-segment-in-backward" if self._opt_apply is not None else None
            elif self._per_bucket_opt_ok():
                self._opt_apply = self.model.optimizer.begin_flat_ranges()
                self._opt_bucketed = self._opt_apply is not None
                self._opt_buckets_done = set()
                self._opt_mode = "per-bucket-in-backward" if self._opt_bucketed else None
        hp = self._main_stream() if not capture else None
        try:
            if hp is None:
                loss = self._train_micro_step(idx, targets, scale, sync, capture)
            else:  # the step's critical path on a high-priority stream (PENROZ_MAIN_PRIORITY=1)
                cur = torch.cuda.current_stream(self.device)
                hp.wait_stream(cur)
                with torch.cuda.stream(hp):
                    loss = self._train_micro_step(idx, targets, scale, sync, capture)
                cur.wait_stream(hp)
        finally:
            self._opt_done = self._opt_apply is not None
            self._opt_apply = None
        return loss

    # the critical path on a high-priority stream. Round 5: GPT-2 headline 61.63 / 61.63 -> 61.19 /
    # 61.19 ms/step. Round 6, with one stream per role per process and the batch copy on its own
    # stream, the headline is faster WITHOUT it: 61.83 / 61.76 / 61.79 (high) vs 61.55 / 61.60 /
    # 61.63 (normal) and 60.45 / 60.54 vs 60.40 / 60.29 on a second box; the Gemma executors keep
    # it (faster there, profiles/notes_r6.md §15, §17)
    MAIN_PRIORITY_DEFAULT = False

    def _main_stream(self):
        """A high-priority stream for the forward / backward critical path, so the side stream's
        weight-gradient GEMMs yield the CUs to the dgrad / attention chain when both have work
        (PENROZ_MAIN_PRIORITY=1 / 0 overrides the executor's default)."""
        env = os.environ.get("PENROZ_MAIN_PRIORITY")
        on = self.MAIN_PRIORITY_DEFAULT if env is None else env == "1"
        if self.device.type != "cuda" or not on or self._side is None:
            return None
        if self._hp_stream is None:
            self._hp_stream = _high_priority_stream(self.device)
        return self._hp_stream

    def _finish_backward(self, sync: bool, cap: bool):
        """The tail of every backward: join the side stream, then the reducer / optimizer tail."""
        self._defer_reductions(False)
        self._finish_wgrad_bookkeeping()
        self._join_side()
        if sync and self.reducer is not None:
            # Overlap the tail: the last bucket (token embedding, produced by the final kernel of
            # the backward) is still reducing when the backward ends. If the optimizer step comes
            # next, it updates each bucket's slice as soon as that bucket's all-reduce has landed
            # (optimizer_step), instead of waiting for all of them here.
            self.reducer.launch_remaining()
            if self._opt_bucketed:  # every bucket's AdamW is queued on the optimizer stream
                self._opt_buckets(range(len(self.reducer.buckets)))
                torch.cuda.current_stream(self.device).wait_stream(self._opt_stream)
                self.reducer.reset()
            elif self._overlap_opt and not cap and self.reducer.per_bucket_waits():
                self._reduce_pending = True
            else:
                with trace_range("grad_allreduce.wait"):
                    self.reducer.finish()

    def wait_gradients(self):
        """Make the current stream wait for every outstanding gradient all-reduce."""
        if self._reduce_pending:
            self._reduce_pending = False
            self.reducer.finish()

    def optimizer_step(self):
        opt = self.model.optimizer
        if self._opt_done:  # applied segment by segment inside the backward
            self._opt_done = False
            return
        if self._clip is not None:
            with trace_range("optimizer"):
                self.wait_gradients()  # every outstanding bucket: the norm is over the averaged gradient
                out = grad_clip_ops.grad_clip_coef(self.flat_grad, self._clip, out=self._clip_out)
                if self._opt_flat:
                    opt.step(scale_dev=out[1:2])
                else:
                    self.flat_grad.mul_(out[1])
                    opt.step()
                    self.refresh_shadow()
            return
        with trace_range("optimizer"):
            if self._reduce_pending:
                self._reduce_pending = False
                red = self.reducer
                ranges = [(lambda i=i: red.wait_bucket(i)) for i in range(len(red.buckets))]
                if self._buckets_tile_flat() and self._opt_flat and opt.flat_step_ranges(ranges):
                    red.reset()
                    self._opt_mode = "per-bucket-after-backward"
                    return
                red.finish()
            opt.step()
            if not self._opt_flat:
                self.refresh_shadow()

    def _buckets_tile_flat(self) -> bool:
        """The ranged optimizer step needs the buckets to cover the flat buffer exactly once."""
        pos = 0
        for s, e in sorted(self.reducer.buckets):
            if s != pos:
                return False
            pos = e
        return pos == self.flat.numel()

    def _layer_names(self) -> list:
        return [l.__class__.__name__.lower() for l in self.model.layers]

    def _set_captured(self, acts: list, act_grads: list):
        """Diagnostics capture: (layer names, one (activation, gradient) pair per layer)."""
        algos = self._layer_names()
        self._captured = (algos, list(zip(acts, act_grads))[:len(algos)])

    def captured(self):
        if self._captured is None:
            return self._layer_names(), []
        return self._captured
