"""Prompt log-probabilities on the CPU (ops/prompt_logprobs.py): the option's validation, the fp32 torch path
against the fp64 reference, ``score_tokens`` / ``generate_*`` with and without the option, ``/generate/``'s JSON."""
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext
from penroz.ops.prompt_logprobs import reference_score, score_rows
from penroz.serve import app as A

V, BLOCK = 64, 8


def gpt(layers=None):
    torch.manual_seed(0)
    return NeuralNetworkModel("gpt", Mapper(layers or bench.gpt2_layers(V=V, C=32, L=2, H=2, P=32), {"adamw": {"lr": 3e-3}}))


@pytest.mark.parametrize("call, text", [
    (lambda m: m.score_tokens([[1]], BLOCK), "2 to block_size"),
    (lambda m: m.score_tokens([[1, 2], list(range(BLOCK + 1))], BLOCK), "sequence 1"),
    (lambda m: m.score_tokens([[1, V]], BLOCK), f"outside [0, {V})"),
    (lambda m: gpt(bench.gpt2_layers(V=V, C=32, L=1, H=2, P=32)[:-2]).score_tokens([[1, 2]], BLOCK), "vocabulary projection"),
    (lambda m: m.generate_tokens([[1]], BLOCK, 2, temperature=0.0, prompt_logprobs=True), "2 to block_size"),
    (lambda m: m.generate_batch([[1, 2], [3]], BLOCK, 2, temperature=0.0, prompt_logprobs=True), "sequence 1"),
    (lambda m: m.generate_tokens([[1, 2]], BLOCK, 2, temperature=0.0, prompt_logprobs=1), "a bool"),
    (lambda m: m.generate_tokens([[1, 2]], BLOCK, 2, temperature=0.0, prompt_logprobs=True, speculate=1), "speculate"),
    (lambda m: list(m.generate_tokens_stream([[1, 2]], BLOCK, 2, temperature=0.0, prompt_logprobs=True)), "stream"),
])
def test_refused_before_any_forward(monkeypatch, call, text):
    m = gpt()

    def no_forward(*a, **k):
        raise AssertionError("a layer ran before validation")

    monkeypatch.setattr(torch.nn.Embedding, "forward", no_forward)
    with pytest.raises(ValueError, match=text.replace("[", r"\[").replace(")", r"\)")):
        call(m)


@pytest.mark.parametrize("dtype, bias", [(torch.float32, True), (torch.bfloat16, False)])
def test_torch_path_matches_the_reference(monkeypatch, dtype, bias):
    g = torch.Generator().manual_seed(3)
    h, W = (torch.randn(n, 48, generator=g).to(dtype) for n in (37, 301))
    b = torch.randn(301, generator=g) if bias else None
    t = torch.randint(0, 301, (37,), generator=g)
    monkeypatch.setattr("penroz.ops.prompt_logprobs.CHUNK_ELEMS", 301 * 8)  # five chunks of rows
    lp, top, top_lp = score_rows(h, W, b, t)
    r_lp, r_top, r_top_lp = reference_score(h, W, b, t)
    assert lp.dtype == top_lp.dtype == torch.float32 and top.dtype == torch.int64 and torch.equal(top, r_top)
    # fp32 over C = 48 and V = 301 terms of |x| < ~40: a few units of 2^-24 · 64
    assert (lp.double() - r_lp).abs().max() < 1e-4 and (top_lp.double() - r_top_lp).abs().max() < 1e-4
    lp, top, top_lp = score_rows(torch.zeros(2, 48, dtype=dtype), W, None, torch.tensor([300, 0]))  # every logit equal
    assert top.tolist() == [0, 0] and torch.allclose(lp, top_lp) and abs(lp[0].item() + torch.tensor(301.0).log().item()) < 1e-6


def test_score_tokens_is_the_definition_row_by_row():
    m = gpt()
    seqs = [[5, 9, 2, 7, 7, 1], [3, 4], [8, 8, 8, 60]]
    got = m.score_tokens(seqs, BLOCK)
    for s, d in zip(seqs, got):
        assert set(d) == {"token_logprobs", "top_tokens", "top_logprobs"} and all(len(v) == len(s) and v[0] is None for v in d.values())
        acts, _ = m(torch.tensor([s]), skip_softmax=True)  # the module's own logits of this sequence alone
        ref = torch.log_softmax(acts[-1][0].double(), dim=-1)
        for i in range(1, len(s)):
            assert abs(d["token_logprobs"][i] - ref[i - 1, s[i]].item()) < 1e-4
            assert d["top_tokens"][i] == int(ref[i - 1].argmax()) and abs(d["top_logprobs"][i] - ref[i - 1].max().item()) < 1e-4
    assert all(a._kv_cache is None for a in m._find_attention_layers())


def test_generate_with_and_without_the_option():
    m = gpt()
    ctx = [[5, 9, 2], [3, 4, 4]]
    plain = m.generate_tokens(ctx, BLOCK, 3, temperature=0.0)
    assert isinstance(plain, list) and plain == m.generate_tokens(ctx, BLOCK, 3, temperature=0.0, prompt_logprobs=False)
    tokens, info = m.generate_tokens(ctx, BLOCK, 3, temperature=0.0, prompt_logprobs=True)
    assert tokens == plain and info == {"prompt_logprobs": m.score_tokens(ctx[:1], BLOCK)[0]}
    tokens, info = m.generate_tokens(ctx, BLOCK, 3, temperature=0.0, prompt_logprobs=True, logprobs=1)
    assert tokens == plain and set(info) == {"token_logprobs", "top_logprobs", "prompt_logprobs"}
    ragged = [[5, 9, 2], [3, 4]]
    batch = m.generate_batch(ragged, BLOCK, 3, temperature=0.0)
    contexts, infos = m.generate_batch(ragged, BLOCK, 3, temperature=0.0, prompt_logprobs=True)
    assert contexts == batch and [i["prompt_logprobs"] for i in infos] == m.score_tokens(ragged, BLOCK)


@pytest.mark.skipif(not _ext.available(), reason="needs the built extension")
def test_launch_plan():
    plan = _ext.kernels().lmhead_lse_plan
    for N, Vn in ((1, 50257), (4096, 50257), (1, 262144), (4096, 262144), (300, 1001), (1, 1)):
        tile, S, grid = plan(N, Vn, 768)
        tiles_m, tiles_n = -(-N // tile), -(-Vn // 128)
        assert tile in (128, 256) and 1 <= S <= tiles_n and grid % 8 == 0 and tiles_m * S <= grid < tiles_m * S + 8
        assert (S - 1) * -(-tiles_n // S) < tiles_n  # no vocabulary range is empty
        assert tiles_m * S >= min(256, tiles_m * tiles_n)  # a workgroup for every CU, where there are that many tiles
    assert plan(4, 1001, 64, 3)[1] == 3 and plan(4, 100, 64, 7)[1] == 1  # a forced S, clamped to the column tiles
    assert plan(1, 100, 40)[0] == 0 and plan(0, 100, 64)[0] == 0 and plan(1, 0, 64)[0] == 0  # refused


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1, 2]], "block_size": 8, "max_new_tokens": 2}
SCORES = {"token_logprobs": [None, -0.5], "top_tokens": [None, 7], "top_logprobs": [None, -0.25]}


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m):
        yield m


def test_api_json(served):
    served.generate_tokens.return_value = ([1, 2, 3, 4], {"prompt_logprobs": SCORES})
    r = client.post("/generate/", json={**BODY, "prompt_logprobs": True})
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3, 4], "prompt_logprobs": SCORES}
    assert served.generate_tokens.call_args.kwargs["prompt_logprobs"] is True
    lp = {"token_logprobs": [-1.0, -2.0], "top_logprobs": [[], []]}
    served.generate_tokens.return_value = ([1, 2, 3, 4], {**lp, "prompt_logprobs": SCORES})
    r = client.post("/generate/", json={**BODY, "prompt_logprobs": True, "logprobs": 0})
    assert r.json() == {"tokens": [1, 2, 3, 4], "logprobs": lp, "prompt_logprobs": SCORES}
    served.generate_batch.return_value = ([[1, 2, 3, 4]], [{"prompt_logprobs": SCORES}])
    r = client.post("/generate/", json={**BODY, "prompt_logprobs": True, "batch": True})
    assert r.json() == {"sequences": [[1, 2, 3, 4]], "prompt_logprobs": [SCORES]}
    served.generate_tokens.return_value = [1, 2, 3, 4]  # without the option: the call and the answer of before
    r = client.post("/generate/", json=BODY)
    assert r.json() == {"tokens": [1, 2, 3, 4]} and "prompt_logprobs" not in served.generate_tokens.call_args.kwargs


def test_api_refuses_stream_and_speculate(served):
    for extra, status in (({"stream": True}, 400), ({"speculate": 1, "temperature": 0.0}, 400), ({"prompt_logprobs": 1}, 422)):
        assert client.post("/generate/", json={**BODY, "prompt_logprobs": True, **extra}).status_code == status
    served.generate_tokens.assert_not_called()
    served.generate_tokens_stream.assert_not_called()
