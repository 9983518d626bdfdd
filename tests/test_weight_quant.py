"""Weight-only int8 quantisation on the CPU (ops/weight_quant.py): the per-row quantiser and its
bounds, the lossless construction the GPU tests rely on, the fp32 reference and its gated / RoPE
compositions, the ``weight_quant`` argument of the generate calls and of ``POST /generate/``, and the
int8 decode GEMV's launch plan (host code of the built extension)."""
from unittest.mock import patch

import pytest
import torch
import torch.nn.functional as F
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext
from penroz.ops import weight_quant as WQ
from penroz.serve import app as A

SHAPES = [(5, 16), (33, 48), (4, 1024)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_quantize_rows_int8_bounds(dtype, shape):
    torch.manual_seed(0)
    w = (torch.randn(*shape) * 0.3).to(dtype)
    w[1] = 0  # an all-zero row
    q, s = WQ.quantize_rows_int8(w)
    assert q.dtype == torch.int8 and q.shape == w.shape and q.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (shape[0],)
    assert int(q.abs().max()) <= 127
    amax = w.float().abs().amax(dim=1)
    live = amax > 0
    assert torch.equal(s[live], (amax / 127.0)[live])
    assert s[1] == 1.0 and not q[1].any()
    assert torch.isfinite(s).all() and torch.isfinite(WQ.dequantize_rows(q, s)).all()
    err = (w.double() - q.double() * s.double().unsqueeze(1)).abs()
    assert (err <= s.double().unsqueeze(1) / 2 * (1 + 2.0 ** -20)).all()
    assert (q.abs().amax(dim=1)[live] == 127).all()  # the row's largest weight maps to ±127


def lossless_weight(N, K, seed, dtype=torch.bfloat16):
    """k · 2^-e with integer |k| <= 127, both -127 and +127 in every row, e varying by row: exactly
    representable in bf16, and quantised without loss (q == k, scale == 2^-e)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-127, 128, (N, K), generator=g)
    k[:, 0], k[:, K - 1] = 127, -127
    e = torch.arange(N) % 5 + 3
    return (k.float() * torch.exp2(-e.float()).unsqueeze(1)).to(dtype), k, torch.exp2(-e.float())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_lossless_rows_come_back_exactly(dtype, shape):
    w, k, s_want = lossless_weight(*shape, seed=1, dtype=dtype)
    assert torch.equal(w.float(), k.float() * s_want.unsqueeze(1))  # the construction is exact in dtype
    q, s = WQ.quantize_rows_int8(w)
    assert torch.equal(q.long(), k) and torch.equal(s, s_want)
    assert torch.equal(WQ.dequantize_rows(q, s), w.float())


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_bias", [False, True])
def test_linear_q8_reference_is_the_dequantised_linear(act, with_bias):
    torch.manual_seed(2)
    x = torch.randn(3, 48).to(torch.bfloat16)
    q, s = WQ.quantize_rows_int8(torch.randn(33, 48))
    b = torch.randn(33).to(torch.bfloat16) if with_bias else None
    want = x.float() @ WQ.dequantize_rows(q, s).t() + (b.float() if with_bias else 0)
    if act:
        want = F.gelu(want, approximate="tanh" if act == 2 else "none")
    got = WQ.linear_q8_reference(x, q, s, b, act)
    assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gated_q8_reference(kind):
    torch.manual_seed(3)
    x = torch.randn(2, 32).to(torch.bfloat16)
    q, s = WQ.quantize_rows_int8(torch.randn(2 * 24, 32))
    y = x.float() @ WQ.dequantize_rows(q, s).t()
    g, u = y[:, :24], y[:, 24:]
    a = {0: F.gelu(g), 1: F.gelu(g, approximate="tanh"), 2: F.silu(g)}[kind]
    assert torch.allclose(WQ.gated_q8_reference(x, q, s, kind), a * u, rtol=1e-6, atol=1e-6)


def test_rope_q8_reference():
    torch.manual_seed(4)
    M, K, H, Hkv, D = 2, 32, 3, 1, 8
    x = torch.randn(M, K).to(torch.bfloat16)
    q, s = WQ.quantize_rows_int8(torch.randn((H + 2 * Hkv) * D, K))
    ang = torch.rand(D // 2) * 6.0
    cos, sin = torch.cos(ang).view(1, -1), torch.sin(ang).view(1, -1)
    y = (x.float() @ WQ.dequantize_rows(q, s).t()).view(M, H + 2 * Hkv, D)
    x1, x2 = y[..., :D // 2], y[..., D // 2:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    want = torch.cat([rot[:, :H + Hkv], y[:, H + Hkv:]], dim=1).reshape(M, -1)
    assert torch.allclose(WQ.rope_q8_reference(x, q, s, cos, sin, D, H + Hkv), want, rtol=1e-6, atol=1e-6)


def test_cached_copy_follows_the_weight_version():
    lin = torch.nn.Linear(16, 4, bias=False)
    a = WQ.linear_q8(lin)
    assert WQ.linear_q8(lin) is a  # one copy per weight version
    with torch.no_grad():
        lin.weight.add_(1.0)
    b = WQ.linear_q8(lin)
    assert b is not a and torch.equal(WQ.dequantize_rows(*b), WQ.dequantize_rows(*WQ.quantize_rows_int8(lin.weight)))


# ------------------------------------------------------------------ the public argument
def gpt():
    torch.manual_seed(0)
    return NeuralNetworkModel("gpt", Mapper(bench.gpt2_layers(V=64, C=32, L=2, H=2, P=32), {"adamw": {"lr": 3e-3}}))


def test_resolve(monkeypatch):
    monkeypatch.delenv("PENROZ_DECODE_WEIGHTS", raising=False)
    assert WQ.resolve(None) is None and WQ.resolve("") is None and WQ.resolve("int8") == "int8"
    monkeypatch.setenv("PENROZ_DECODE_WEIGHTS", "int8")
    assert WQ.resolve(None) == "int8" and WQ.resolve("") is None  # the environment is only the default
    monkeypatch.setenv("PENROZ_DECODE_WEIGHTS", "int4")
    with pytest.raises(ValueError):
        WQ.resolve(None)
    for bad in ("int4", "fp8", "INT8", "bf16"):
        with pytest.raises(ValueError):
            WQ.resolve(bad)


def test_unknown_format_raises_before_any_forward():
    m = gpt()
    with patch.object(NeuralNetworkModel, "forward", side_effect=AssertionError("forward ran")):
        with pytest.raises(ValueError):
            m.generate_tokens([[1, 2, 3]], 8, 4, temperature=0.0, weight_quant="int4")
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2, 3]], 8, 4, temperature=0.0, weight_quant="int4")
        with pytest.raises(ValueError):
            list(m.generate_tokens_stream([[1, 2, 3]], 8, 4, temperature=0.0, weight_quant="int4"))


def test_int8_on_a_cpu_model_changes_nothing(monkeypatch):
    m = gpt()
    greedy = m.generate_tokens([[1, 2, 3]], 8, 10, temperature=0.0)
    assert m.generate_tokens([[1, 2, 3]], 8, 10, temperature=0.0, weight_quant="int8") == greedy
    assert list(m.generate_tokens_stream([[1, 2, 3]], 8, 10, temperature=0.0, weight_quant="int8")) == greedy[3:]
    assert m.generate_batch([[1, 2, 3]] * 2, 8, 4, temperature=0.0, weight_quant="int8") == [greedy[:7]] * 2
    monkeypatch.setenv("PENROZ_DECODE_WEIGHTS", "int8")
    assert m.generate_tokens([[1, 2, 3]], 8, 10, temperature=0.0) == greedy


def test_environment_default_reaches_the_decoder_lookup(monkeypatch):
    """PENROZ_DECODE_WEIGHTS is the default of every generate call: what ``get_decoder`` is asked for."""
    from penroz.models import graph_decode as gd
    seen = []
    monkeypatch.setattr(gd, "get_decoder", lambda *a: seen.append(a[-1]))  # None: the eager path
    m = gpt()
    monkeypatch.setenv("PENROZ_DECODE_WEIGHTS", "int8")
    m.generate_tokens([[1, 2]], 8, 2, temperature=0.0)
    m.generate_tokens([[1, 2]], 8, 2, temperature=0.0, weight_quant="")
    monkeypatch.delenv("PENROZ_DECODE_WEIGHTS")
    m.generate_tokens([[1, 2]], 8, 2, temperature=0.0)
    m.generate_batch([[1, 2]], 8, 2, temperature=0.0, weight_quant="int8")
    assert seen == ["int8", None, None, "int8"]


client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1, 2, 3]], "block_size": 8, "max_new_tokens": 3, "temperature": 0.0}


def test_api_unknown_format_is_400_before_a_forward():
    m = gpt()
    with patch.object(A, "load_for_serving", return_value=m), \
            patch.object(NeuralNetworkModel, "forward", side_effect=AssertionError("forward ran")):
        for stream in (False, True):
            r = client.post("/generate/", json={**BODY, "weight_quant": "int4", "stream": stream})
            assert r.status_code == 400 and "weight_quant" in r.json()["detail"]


def test_api_passes_the_format_through():
    m = gpt()
    want = m.generate_tokens([[1, 2, 3]], 8, 3, temperature=0.0)
    with patch.object(A, "load_for_serving", return_value=m), \
            patch.object(m, "generate_tokens", wraps=m.generate_tokens) as plain, \
            patch.object(m, "generate_tokens_stream", wraps=m.generate_tokens_stream) as stream:
        r = client.post("/generate/", json={**BODY, "weight_quant": "int8"})
        assert r.status_code == 200 and r.json() == {"tokens": want}
        assert plain.call_args.kwargs["weight_quant"] == "int8"
        r = client.post("/generate/", json={**BODY, "weight_quant": "int8", "stream": True})
        assert r.text == "".join(f"{t}\n" for t in want[3:])
        assert stream.call_args.kwargs["weight_quant"] == "int8"
        assert client.post("/generate/", json=BODY).status_code == 200
        assert plain.call_args.kwargs["weight_quant"] is None


# ------------------------------------------------------------------ launch plan (host code)
needs_ext = pytest.mark.skipif(not _ext.available(), reason="HIP extension not built")
HALF, WAVE, LN = 0, 1, 2


@needs_ext
def test_q8_limits_are_the_launchers_own():
    from penroz.models import graph_decode as gd
    assert _ext.kernels().decode_gemv_q8_limits() == (4, 8192, 1024, 1792, 16)
    assert gd._gemv_q8_limits() == (4, 8192, 1024, 1792, 16)
    assert _ext.kernels().decode_gemv_q8_limits()[:4] == _ext.kernels().decode_gemv_limits()


@needs_ext
@pytest.mark.parametrize("M,N,K,ln,rpw,want", [
    # GPT-2 124M: qkv / fc in LN mode (2 rows per wave), proj / fc2 one row per wave, lm_head 8 rows
    (1, 2304, 768, True, 0, (LN, 1, 1, 2, 1152)),
    (4, 3072, 768, True, 0, (LN, 4, 1, 2, 1536)),
    (1, 768, 768, False, 0, (WAVE, 1, 1, 1, 768)),
    (4, 768, 3072, False, 0, (WAVE, 4, 1, 3, 768)),
    (1, 50257, 768, True, 0, (LN, 1, 4, 2, 6283)),
    # Gemma-3 1B: o (K = 1024), down (K = 6912), lm_head (N = 262144, K = 1152)
    (1, 1152, 1024, False, 0, (WAVE, 1, 1, 1, 1152)),
    (4, 1152, 6912, False, 0, (WAVE, 4, 1, 7, 1152)),
    (1, 262144, 1152, False, 0, (HALF, 1, 4, 3, 32768)),
    (4, 262144, 1152, False, 0, (HALF, 4, 4, 3, 32768)),
    # degenerate: one chunk, one row, odd N, forced rows per wave
    (1, 1, 16, False, 0, (WAVE, 1, 1, 1, 1)),
    (1, 1, 16, False, 2, (HALF, 1, 1, 1, 1)),
    (3, 33, 48, False, 8, (HALF, 3, 4, 1, 5)),
    (3, 33, 48, True, 0, (LN, 3, 1, 1, 17)),
    (1, 16, 8192, False, 8, (HALF, 1, 4, 16, 2)),
    (1, 16, 8192, False, 0, (WAVE, 1, 1, 8, 16)),
    # the K limit at 4 rows: 16 chunks per lane × (4 VGPRs per row pair + 8 per x row) is above the
    # register budget at every rows-per-wave, so the wave-per-row form (8 chunks per lane) takes it
    (4, 50304, 8192, False, 0, (WAVE, 4, 1, 8, 50304)),
    (4, 16, 8192, False, 2, (WAVE, 4, 1, 8, 16)),
    # ... and at 2 rows 8 rows per wave is halved until it fits: 16·(4·2 + 8·2) = 384 <= 416
    (2, 50304, 8192, False, 0, (HALF, 2, 2, 16, 12576)),
])
def test_q8_plan(M, N, K, ln, rpw, want):
    assert _ext.kernels().decode_gemv_q8_plan(M, N, K, ln, rpw) == want


@needs_ext
def test_q8_plan_refuses_what_has_no_kernel():
    plan = _ext.kernels().decode_gemv_q8_plan
    assert plan(1, 64, 768, False, 3)[2] == 0  # rows per wave 2, 4 or 8
    assert plan(1, 64, 8192 + 512, False, 2)[3] == 0  # chunks per lane above every bucket
    assert plan(1, 64, 1024 + 512, True, 0)[3] == 0  # LN mode: K <= 1024
    assert _ext.kernels().decode_gemv_q8_pair_plan(64, 1792 + 512, 0)[1] == 0


@needs_ext
@pytest.mark.parametrize("N,K,ppw,want", [
    (2 * 6912, 1152, 0, (2, 3, 3456)),   # Gemma-3 1B gate|up
    (1536, 1152, 0, (1, 3, 768)),        # ... and QKV
    (256, 64, 0, (1, 2, 128)),
    (64, 1792, 4, (4, 4, 8)),
    (2, 16, 0, (1, 2, 1)),
    (66, 16, 2, (2, 2, 17)),             # an odd number of pairs: the last wave has one
])
def test_q8_pair_plan(N, K, ppw, want):
    assert _ext.kernels().decode_gemv_q8_pair_plan(N, K, ppw) == want
