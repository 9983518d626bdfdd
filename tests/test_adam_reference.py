"""CPU checks behind tests/test_optimizer_kernels_gpu.py:

* the fp64 reference, the inputs and the bound (tests/adam_reference.py) can tell a wrong Adam
  step from a right one: each deliberate mistake in the reference exceeds the bound 10x or more;
* the fp32 yardstick that sets K still measures what the header of adam_reference.py records;
* every range boundary the executors hand to the flat Adam kernel (segments, gradient buckets, the
  pieces of the last bucket) is a multiple of 4 elements, so the kernel's float4 / packed-bf16
  accesses are aligned and ``flat_step`` may refuse anything else.
"""
import types
from types import SimpleNamespace

import pytest
import torch

import adam_reference as A
import bench
from penroz.models.executor import GPTExecutor
from penroz.models.gemma_executor import GemmaExecutor
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.parallel.reducer import plan_buckets, split_last_bucket


def test_fp32_yardstick_matches_the_recorded_ratios():
    for si, h in enumerate(A.HYPER_SETS):
        for dec in (True, False):
            worst = 0.0
            for n in A.CALIBRATION_SIZES:
                worst = max(worst, A.fp32_ratios(*A.make_inputs(n, h["step"], 0), h, dec)[0])
            print(f"set {si} {'decoupled' if dec else 'L2'}: fp32 p ratio {worst:.2f}, K_p {A.k_for(h, dec)[0]:.1f}")
            # recorded: 2.95 … 13.01 (the issue measured 3.4 … 10.3 with its own draw of the inputs)
            assert 2.0 <= worst <= 20.0, (si, dec, worst)
            assert A.k_for(h, dec)[0] == pytest.approx(4 * worst)


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_each_mutation_of_the_reference_exceeds_the_bound(mutation):
    """A kernel with this mistake would miss the p bound by >= 10x on at least one set."""
    best = 0.0
    for h in A.HYPER_SETS:
        for dec in (True, False):
            p, g, m, v = A.make_inputs(1023, h["step"], 0)
            ref, sc = A.scales(p, g, m, v, h, dec)
            got = A.adam_ref_mutated(mutation, p, g, m, v, decoupled=dec, **h)[:3]
            over = A.worst_ratios(got, ref, sc)[0] / A.k_for(h, dec)[0]
            best = max(best, over)
    print(f"{mutation}: worst p err / bound = {best:.3g}")
    assert best >= 10.0, (mutation, best)


def test_unmutated_reference_is_within_its_own_bound():
    for h in A.HYPER_SETS:
        for dec in (True, False):
            p, g, m, v = A.make_inputs(1023, h["step"], 0)
            ref, sc = A.scales(p, g, m, v, h, dec)
            A.assert_within(A.adam_fp32(p, g, m, v, decoupled=dec, **h), ref, sc, A.k_for(h, dec), "fp32 torch")


# ---------------------------------------------------------------- flat range boundaries
def _gpt(V):
    return NeuralNetworkModel("t", Mapper(bench.gpt2_layers(V=V, C=256, L=2, H=4, P=256), {"adamw": {"lr": 1e-3}}))


def _gemma(model_type, V, L=2, F=512, **extra):
    cfg = SimpleNamespace(model_type=model_type, vocab_size=V, hidden_size=256, intermediate_size=F,
                          num_hidden_layers=L, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                          rms_norm_eps=1e-6, rope_theta=10000.0, rope_local_base_freq=10000.0, attention_dropout=0.0,
                          hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=64, sliding_window=512, **extra)
    return NeuralNetworkModel("g", Mapper(Mapper.from_hf_config(cfg), {"adamw": {"lr": 1e-3}}))


GEMMA4 = dict(layer_types=["sliding_attention", "full_attention", "sliding_attention", "full_attention"],
              global_head_dim=512, num_global_key_value_heads=1, num_kv_shared_layers=2, use_double_wide_mlp=True)

LAYOUTS = [
    (GPTExecutor, lambda: _gpt(512)),
    (GPTExecutor, lambda: _gpt(509)),
    (GemmaExecutor, lambda: _gemma("gemma3_text", 512)),
    (GemmaExecutor, lambda: _gemma("gemma3_text", 1000)),
    (GemmaExecutor, lambda: _gemma("gemma2", 1000)),
    (GemmaExecutor, lambda: _gemma("gemma", 1000)),
    (GemmaExecutor, lambda: _gemma("gemma4", 512, L=4, F=256, **GEMMA4)),
]


def _flattened(cls, model, monkeypatch, padded):
    """The executor's flat layout on the CPU; ``padded`` lays the lm_head out with its pad rows
    (up to a multiple of 128) as on the GPU, where alone the padding is on."""
    if padded:
        monkeypatch.setattr(cls, "_head_pad_policy", lambda self: (-self.spec.V) % self.HEAD_PAD)
    ex = object.__new__(cls)
    ex.model, ex.spec, ex.device = model, cls.match(model), torch.device("cpu")
    assert ex.spec is not None
    ex.L = len(ex.spec.blocks)
    ex._flatten()
    return ex


def test_head_pad_is_fixed_when_the_flat_buffers_are_laid_out(monkeypatch):
    """PENROZ_HEAD_PAD is read once, by ``_flatten``: changing it afterwards must not move the
    slices an existing executor takes out of its flat buffers."""
    monkeypatch.delenv("PENROZ_HEAD_PAD", raising=False)
    with monkeypatch.context() as construction:  # the padded policy holds for the layout only
        ex = _flattened(GPTExecutor, _gpt(509), construction, True)
    C = ex.spec.C
    assert ex.Vp == 512 and ex.head_pad_rows() == 3
    monkeypatch.setenv("PENROZ_HEAD_PAD", "0")
    assert ex.Vp == 512 and ex.head_pad_rows() == 3
    assert ex.head_w().shape == (512, C) and ex.head_grad().shape == (512, C)
    off = ex.offsets[id(ex.spec.head.weight)]
    pad = slice(off + 509 * C, off + 512 * C)  # the flat pad range: right after the V real rows
    for rows, flat in ((ex.head_w()[509:], ex.shadow), (ex.head_grad()[509:], ex.flat_grad)):
        assert rows.shape == (3, C) and rows.is_contiguous()
        assert rows.data_ptr() == flat[pad].data_ptr() and rows.numel() == flat[pad].numel()
    assert torch.all(ex.flat[pad] == 0) and torch.all(ex.head_w()[509:] == 0)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_every_flat_range_boundary_is_a_multiple_of_4(monkeypatch, layout, padded):
    cls, make = LAYOUTS[layout]
    ex = _flattened(cls, make(), monkeypatch, padded)
    total = ex.flat.numel()
    assert ex.segments[0][0] == 0 and ex.segments[-1][1] == total
    if padded:
        assert ex.Vp % 128 == 0 and total == sum(p.numel() for p in ex.params_in_order) + ex.head_pad_rows() * ex.spec.C
    bounds = {b for seg in ex.segments for b in seg}
    for bucket_bytes in (1, 2**18, 2**20, 2**40):  # one bucket per segment … one bucket in all
        buckets = plan_buckets(ex.segments, bucket_bytes)
        for pieces in (1, 3, 4, 7):
            cut = split_last_bucket(buckets, pieces)
            assert cut[0][0] == 0 and cut[-1][1] == total and all(a[1] == b[0] for a, b in zip(cut, cut[1:]))
            bounds |= {b for r in cut for b in r}
    # the row-split embedding step takes the last segment as a table: C % 4 and its start
    assert ex.spec.C % 4 == 0
    off = [b for b in sorted(bounds) if b % 4]
    assert not off, f"flat range boundaries off a multiple of 4 elements: {off[:8]}"
    # the flat buffers themselves come 16-B aligned from the allocator
    for t in (ex.flat, ex.flat_grad):
        assert t.data_ptr() % 16 == 0
    assert ex.shadow.data_ptr() % 8 == 0
