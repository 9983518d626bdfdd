"""Int8 weight-only decode on MI355X: the int8 decode GEMV (csrc/kernels/decode_gemv_q8.hip) against
``linear_q8_reference`` on the same quantised operand, in every form the decode programs use, and
the GPT / Gemma decode programs, the decoder cache and ``generate_*`` with ``weight_quant="int8"``.

Kernel tolerances are those of the matching bf16 GEMV tests (tests/test_kernels_gpu.py): the
reference sees the same int8 operand, so the quantisation adds no error. Row scales differ by powers
of two over a 2^6 range, so a scale read from the wrong row (the partner half's row of a pair, a
clamped tail row) fails; every row holds both -127 and +127. Program tests first make every linear
weight lossless under the quantiser (tests/test_weight_quant.py pins the construction), so the int8
step computes the same function as the bf16 step."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode as gd
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext, gemm as G
from penroz.ops import weight_quant as WQ

DEV = "cuda"
SENTINEL = 5.0


def _close(a, b, atol, rtol=0.0, msg=""):
    err = (a.float() - b.float()).abs().max().item()
    lim = atol + rtol * b.float().abs().max().item()
    print(f"{msg}: max err {err:.5g}, limit {lim:.5g}")
    assert err <= lim, f"{msg} max err {err} > {lim}"


def _operand(N, K, seed):
    """int8 rows with -127 and +127 in each, scale[n] = 2^(n mod 7 - 3) × the natural scale of a
    1/sqrt(K) weight (absmax ≈ 3 sigma)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
    q[:, 0], q[:, K - 1] = 127, -127
    s = torch.exp2((torch.arange(N) % 7 - 3).float()) * (3.0 / (127.0 * math.sqrt(K)))
    return q.to(DEV), s.to(DEV)


def _out(M, N):
    """The output as a view into a wider buffer of sentinels: nothing past N may be written."""
    full = torch.full((M, N + 3), SENTINEL, device=DEV, dtype=torch.bfloat16)
    return full, full[:, :N]


def _untouched(full, N):
    assert torch.all(full[:, N:] == SENTINEL), "wrote past N"


# ------------------------------------------------------------------ kernel parity
@pytest.mark.parametrize("M,K,N", [(1, 16, 2), (3, 48, 33), (4, 1024, 75), (1, 8192, 16), (2, 768, 50304)])
def test_q8_gemv_plain(M, K, N):
    """bf16 x (a strided view), with and without bias, rows per wave by shape (the wave-per-row form
    below 16k rows) and forced to 2 / 8 (the half-wave form)."""
    torch.manual_seed(1)
    x = torch.randn(M, K + 16, device=DEV).to(torch.bfloat16)[:, :K]
    q, s = _operand(N, K, 1)
    b = torch.randn(N, device=DEV).to(torch.bfloat16)
    ref = WQ.linear_q8_reference(x, q, s)
    for bias in (None, b):
        want = ref if bias is None else ref + b.float()
        for rpw in (0, 2, 8):
            full, out = _out(M, N)
            _ext.kernels().decode_gemv_q8(x, None, None, None, None, None, None, 0.0, q, s, bias, out, 0, rpw)
            _close(out, want, 2e-2, 2e-2, f"plain rpw {rpw} bias {bias is not None}")
            _untouched(full, N)


@pytest.mark.parametrize("M,K,N", [(1, 768, 2304), (4, 1024, 75), (3, 96, 50)])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_delta", [True, False])
def test_q8_gemv_ln(M, K, N, act, with_delta):
    """LN mode: act(LN(resid + delta + dbias) · Wᵀ + b), the residual sum written by workgroup 0."""
    torch.manual_seed(0)
    rin = torch.randn(M, K, device=DEV) * 2 + 0.5
    delta = torch.randn(M, K, device=DEV).to(torch.bfloat16) if with_delta else None
    dbias = torch.randn(K, device=DEV) if with_delta else None
    gamma, beta = torch.randn(K, device=DEV), torch.randn(K, device=DEV)
    q, s = _operand(N, K, 2)
    b = torch.randn(N, device=DEV).to(torch.bfloat16)
    sm = rin + (delta.float() + dbias) if with_delta else rin
    y = F.layer_norm(sm, (K,), gamma, beta, 1e-5).to(torch.bfloat16)
    want = WQ.linear_q8_reference(y, q, s, b, act)
    for rpw in (0, 8):
        rout = torch.full((M, K), 7.0, device=DEV) if with_delta else None
        full, out = _out(M, N)
        _ext.kernels().decode_gemv_q8(None, rin, delta, dbias, rout, gamma, beta, 1e-5, q, s, b, out, act, rpw)
        _close(out, want, 2e-2, 2e-2, f"ln rpw {rpw}")
        _untouched(full, N)
        if with_delta:
            _close(rout, sm, 1e-6, 1e-6, "resid_out")


@pytest.mark.parametrize("M,K,I", [(3, 64, 128), (2, 1792, 32), (1, 1152, 6912)])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_q8_gemv_gated(M, K, I, kind):
    """Paired rows on the packed [gate; up] operand: gate row n and up row I + n have different scales."""
    torch.manual_seed(2)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    q, s = _operand(2 * I, K, 3)
    assert I % 7, "rows n and I + n of a pair must get different scales"
    want = WQ.gated_q8_reference(x, q, s, kind)
    for ppw in (0, 4):
        full, out = _out(M, I)
        _ext.kernels().decode_gemv_q8_pair(x, q, s, out, 1, kind, pairs_per_wave=ppw)
        _close(out, want, 3e-2, 2e-2, f"gated ppw {ppw}")
        _untouched(full, I)


@pytest.mark.parametrize("M,K,H,Hkv,D", [(3, 64, 2, 2, 64), (2, 96, 3, 1, 32), (1, 1152, 4, 1, 256)])
def test_q8_gemv_rope(M, K, H, Hkv, D):
    """Paired rows j, j + D/2 of each head, rotated for the first H + Hkv heads, V passed through."""
    torch.manual_seed(3)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    N = (H + 2 * Hkv) * D
    q, s = _operand(N, K, 4)
    ang = torch.rand(D // 2, device=DEV) * 6.0
    cos, sin = torch.cos(ang).view(1, -1).contiguous(), torch.sin(ang).view(1, -1).contiguous()
    want = WQ.rope_q8_reference(x, q, s, cos, sin, D, H + Hkv)
    for ppw in (0, 2):
        full, out = _out(M, N)
        _ext.kernels().decode_gemv_q8_pair(x, q, s, out, 2, 0, D, H + Hkv, cos, sin, ppw)
        _close(out, want, 3e-2, 2e-2, f"rope ppw {ppw}")
        _untouched(full, N)


def test_q8_launcher_refuses_shapes_outside_its_limits():
    K_ = _ext.kernels()

    def plain(M, K, N=8):
        q, s = torch.zeros(N, K, dtype=torch.int8, device=DEV), torch.ones(N, device=DEV)
        x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
        out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
        K_.decode_gemv_q8(x, None, None, None, None, None, None, 0.0, q, s, None, out, 0, 0)

    with pytest.raises(RuntimeError, match="K % 16 == 0"):
        plain(1, 24)
    with pytest.raises(RuntimeError, match="K <= 8192"):
        plain(1, 8192 + 16)
    with pytest.raises(RuntimeError, match="1..4 rows"):
        plain(5, 64)
    q, s = torch.zeros(8, 1792 + 16, dtype=torch.int8, device=DEV), torch.ones(8, device=DEV)
    x = torch.zeros(1, 1792 + 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="K <= 1792"):
        K_.decode_gemv_q8_pair(x, q, s, torch.zeros(1, 4, device=DEV, dtype=torch.bfloat16), 1, 0)
    q, s = torch.zeros(8, 1040, dtype=torch.int8, device=DEV), torch.ones(8, device=DEV)
    with pytest.raises(RuntimeError, match="LN mode needs K <= 1024"):
        K_.decode_gemv_q8(None, torch.zeros(1, 1040, device=DEV), None, None, None, torch.ones(1040, device=DEV),
                          torch.zeros(1040, device=DEV), 1e-5, q, s, None,
                          torch.zeros(1, 8, device=DEV, dtype=torch.bfloat16), 0, 0)
    with pytest.raises(RuntimeError, match="row scales"):
        K_.decode_gemv_q8(torch.zeros(1, 64, device=DEV, dtype=torch.bfloat16), None, None, None, None, None, None, 0.0,
                          torch.zeros(8, 64, dtype=torch.int8, device=DEV), torch.ones(7, device=DEV), None,
                          torch.zeros(1, 8, device=DEV, dtype=torch.bfloat16), 0, 0)


# ------------------------------------------------------------------ decode programs
def _make_lossless(model):
    """Every nn.Linear weight becomes k · 2^-e (integer |k| <= 127, ±127 in every row, e by row) at
    about its initial magnitude: quantised without loss, so int8 and bf16 steps compute one function."""
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for mod in model.modules():
            if type(mod) is not torch.nn.Linear:
                continue
            N, K = mod.weight.shape
            k = torch.randint(-127, 128, (N, K), generator=g)
            k[:, 0], k[:, K - 1] = 127, -127
            e = round(math.log2(73.0 * math.sqrt(K))) + torch.arange(N) % 3
            w = k.float() * torch.exp2(-e.float()).unsqueeze(1)
            mod.weight.copy_(w.to(mod.weight.dtype))
            assert torch.equal(mod.weight.float().cpu(), w)
    return model


def _gpt():
    torch.manual_seed(11)
    m = NeuralNetworkModel("wq", Mapper(bench.gpt2_layers(V=256, C=128, L=2, H=2, P=64),
                                        {"adamw": {"lr": 1e-3}})).to("cuda")
    return _make_lossless(m.to(dtype=torch.bfloat16))


def _gemma(head_dim):
    """Tiny Gemma-3 style model (RoPE, GQA 4:1, RMSNorm, gated MLP) from the HF config builder."""
    from types import SimpleNamespace
    tc = SimpleNamespace(vocab_size=256, hidden_size=64, num_attention_heads=4, num_key_value_heads=1,
                         head_dim=head_dim, num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6,
                         rope_theta=10000.0, attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh",
                         model_type="gemma3_text")
    torch.manual_seed(5)
    m = NeuralNetworkModel("wg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}})).to("cuda")
    return _make_lossless(m.to(dtype=torch.bfloat16))


def _int8_steps_vs_bf16_steps(m, program_cls, rows):
    """After a 6-token module prefill, 3 teacher-forced steps: the int8 program against the bf16
    program of the same model on the same cache state (each step's slot written by both in turn)."""
    dec = gd.GraphDecoder(m, rows, 32, 0.0, None, weight_quant="int8")
    assert isinstance(dec.program, program_cls) and dec.weight_quant == "int8"
    ref_prog = program_cls.build(m)  # no int8 copies enabled: the parent commit's step
    idx = torch.randint(0, 256, (rows, 9), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    with torch.inference_mode():
        dec.attach()
        try:
            m(idx[:, :6], skip_softmax=True)  # prefill through the modules
            assert dec.cache.seq_len() == 6
            dec.cache.graph_mode = True
            for t in range(3):
                tok = idx[:, 6 + t:7 + t]
                dec._set_state(tok, 6 + t)
                dec.cache.begin_step()
                ref = ref_prog.forward(tok, dec.cache).float()
                dec.cache.begin_step()
                got = dec.program.forward(tok, dec.cache).float()  # rewrites the same cache slot
                rel = ((got - ref).norm() / ref.norm()).item()
                print(f"step {t}: rel {rel:.3g}")
                assert torch.isfinite(got).all() and rel < 2e-2, (t, rel)
        finally:
            dec.cache.graph_mode = False
            dec.detach()


@pytest.mark.parametrize("rows", [1, 3])
def test_gpt_int8_program_steps_match_bf16_program(rows):
    _int8_steps_vs_bf16_steps(_gpt(), gd.GPTDecodeProgram, rows)


@pytest.mark.parametrize("head_dim", [64, 256])
@pytest.mark.parametrize("rows", [1, 4])
def test_gemma_int8_program_steps_match_bf16_program(head_dim, rows):
    _int8_steps_vs_bf16_steps(_gemma(head_dim), gd.GemmaDecodeProgram, rows)


@pytest.mark.parametrize("build", [_gpt, lambda: _gemma(64)], ids=["gpt", "gemma"])
def test_six_rows_keep_bf16_weights(build):
    m = build()
    ctx = torch.randint(0, 256, (6, 5), generator=torch.Generator().manual_seed(2)).tolist()
    plain = m.generate_batch(ctx, 16, 12, temperature=0.0)
    (bf16_dec,) = m._graph_decoders.values()
    asked = m.generate_batch(ctx, 16, 12, temperature=0.0, weight_quant="int8")
    # the request has no effect, so it shares the bf16 decoder: the cache is keyed on the format in effect
    assert list(m._graph_decoders.values()) == [bf16_dec]
    assert bf16_dec.weight_quant is None and bf16_dec.graph is not None
    assert asked == plain
    m.__dict__.pop("_graph_decoders")
    assert m.generate_batch(ctx, 16, 12, temperature=0.0, weight_quant="int8") == plain  # and asked for first
    assert [d.weight_quant for d in m._graph_decoders.values()] == [None]


class _EagerGraph:
    """Stands in for a captured graph: replay() runs the decode step eagerly."""

    def __init__(self, dec):
        self.dec = dec

    def replay(self):
        self.dec._step()


@pytest.mark.parametrize("build", [_gpt, lambda: _gemma(256)], ids=["gpt", "gemma"])
def test_int8_generation_graph_replay_matches_eager_program(monkeypatch, build):
    m = build()
    ctx = [[3, 1, 4, 1, 5]]
    graphed = m.generate_tokens(ctx, 16, 40, temperature=0.0, weight_quant="int8")  # through the sliding window
    decs = list(m._graph_decoders.values())
    assert decs and all(d.weight_quant == "int8" and isinstance(d.graph, torch.cuda.CUDAGraph) for d in decs)
    assert len(graphed) == 45
    assert m.generate_tokens(ctx, 16, 40, temperature=0.0, weight_quant="int8") == graphed
    assert list(m.generate_tokens_stream(ctx, 16, 40, temperature=0.0, weight_quant="int8")) == graphed[5:]
    m.__dict__.pop("_graph_decoders")

    def eager_capture(self, last_tok, cache_len, start=0):
        self._set_state(last_tok, cache_len, start)
        self.graph = _EagerGraph(self)

    monkeypatch.setattr(gd.GraphDecoder, "_capture", eager_capture)
    eager = m.generate_tokens(ctx, 16, 40, temperature=0.0, weight_quant="int8")
    assert all(d.weight_quant == "int8" for d in m._graph_decoders.values())
    assert graphed == eager


def test_decoder_cache_keys_on_the_format_and_requantises_updated_weights(monkeypatch):
    m = _gpt()
    ctx = [[3, 1, 4, 1, 5]]
    m.generate_tokens(ctx, 32, 4, temperature=0.0)
    m.generate_tokens(ctx, 32, 4, temperature=0.0, weight_quant="int8")
    decs = list(m._graph_decoders.values())
    assert len(decs) == 2 and decs[0] is not decs[1]
    assert [d.weight_quant for d in decs] == [None, "int8"]
    old = decs[1]
    head = old.program.spec.head
    stale = old.program.q8[id(head)]
    assert all(gd.get_decoder(m, 1, 32, 0.0, None, weight_quant=wq) is d for wq, d in zip((None, "int8"), decs))

    with torch.no_grad():  # an in-place update of one weight: the next call must not decode with the old copy
        head.weight.add_((torch.randn(head.weight.shape, device="cuda") * head.weight.float().std()).to(torch.bfloat16))
    dec = gd.get_decoder(m, 1, 32, 0.0, None, weight_quant="int8")
    assert dec is not old and dec.weight_quant == "int8"
    fresh = WQ.quantize_rows_int8(head.weight)
    assert all(torch.equal(a, b) for a, b in zip(dec.program.q8[id(head)], fresh))
    assert not torch.equal(fresh[0], stale[0])

    calls = []
    real = G.decode_gemv_q8_ln

    def spy(resid, ln, qw, bias, act=0, delta=None, dbias=None, resid_out=None):
        out = real(resid, ln, qw, bias, act, delta=delta, dbias=dbias, resid_out=resid_out)
        calls.append((resid.clone(), ln, delta, dbias, bias, out))
        return out

    monkeypatch.setattr(G, "decode_gemv_q8_ln", spy)
    idx = torch.tensor([[3, 1, 4, 1, 5, 9, 2]], device="cuda")
    with torch.inference_mode():
        dec.attach()
        try:
            m(idx[:, :6], skip_softmax=True)
            dec._set_state(idx[:, 6:], 6)
            dec.cache.graph_mode = True
            dec.cache.begin_step()
            logits = dec.program.forward(idx[:, 6:], dec.cache)
        finally:
            dec.cache.graph_mode = False
            dec.detach()
    resid, ln, delta, dbias, bias, out = calls[-1]  # the lm_head: LN_f of the last residual sum
    assert out is logits
    y = F.layer_norm(resid + delta.float() + dbias, (resid.shape[1],), ln[0], ln[1], ln[2]).to(torch.bfloat16)
    _close(logits, WQ.linear_q8_reference(y, *fresh, bias), 2e-2, 2e-2, "first-step logits, fresh copy")
    gap = (WQ.linear_q8_reference(y, *stale, bias) - logits.float()).abs().max().item()
    assert gap > 3 * (2e-2 + 2e-2 * logits.float().abs().max().item()), gap  # the old copy is far off
