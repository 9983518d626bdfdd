"""Ragged batches (ops/ragged.py) without a GPU: the definition's validation, generate_batch on prompts
of different lengths against the one-row calls (here the rows run one at a time: the documented
fallback), the rectangular path left as it was, and /generate's ``batch`` mode."""
import logging
from unittest.mock import patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import ragged
from penroz.serve import app as A

V, BLOCK, NEW = 256, 32, 8
PROMPTS = [[3, 1, 4], [1, 5, 9, 2, 6, 5], [3]]


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    m = NeuralNetworkModel("ragged", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 3e-3}}))
    singles = [m.generate_tokens([p], BLOCK, NEW, temperature=0.0) for p in PROMPTS]
    return m, singles


# ------------------------------------------------------------------ the definition
def test_check_prompts_accepts_the_definition():
    assert ragged.check_prompts(PROMPTS, 32, 8, V) == PROMPTS
    assert ragged.check_prompts([(1, 2), [3]], 4, 2, V) == [[1, 2], [3]]
    assert ragged.check_prompts([[0], [V - 1, 0]], 10, 8, V) == [[0], [V - 1, 0]]  # Lmax + new == block_size
    assert ragged.check_prompts([[2 ** 20]], 8, 1) == [[2 ** 20]]  # no vocabulary known


@pytest.mark.parametrize("bad", [[], [[1], []], [[1], [V]], [[1], [-1]], [[1], [1.5]], [[1], [True]], [[1], 2],
                                 "ab", [[1], "a"], None],
                         ids=["none", "empty-row", "beyondV", "negative", "float", "bool", "flat", "str", "str-row", "None"])
def test_check_prompts_refuses(bad):
    with pytest.raises(ValueError):
        ragged.check_prompts(bad, 32, 8, V)


def test_check_prompts_refuses_a_window_that_would_slide():
    with pytest.raises(ValueError, match="block_size"):
        ragged.check_prompts(PROMPTS, 13, 8, V)  # Lmax 6 + 8 > 13
    assert ragged.check_prompts(PROMPTS, 14, 8, V) == PROMPTS


def test_ragged_lengths_and_padding():
    assert ragged.ragged_lengths(PROMPTS) == [3, 6, 1]
    for rect in ([[1, 2], [3, 4]], [[1, 2]], [1, 2, 3], [[1], 2], "ab", None, []):
        assert ragged.ragged_lengths(rect) is None
    assert ragged.pad_prompts(PROMPTS) == [[3, 1, 4, 4, 4, 4], [1, 5, 9, 2, 6, 5], [3, 3, 3, 3, 3, 3]]
    assert ragged.assemble([[1], [2, 3]], [[7, 8], [9]]) == [[1, 7, 8], [2, 3, 9]]


# ------------------------------------------------------------------ through a tiny model
def test_generate_batch_takes_ragged_prompts_and_equals_the_one_row_calls(tiny):
    m, singles = tiny
    out = m.generate_batch(PROMPTS, BLOCK, NEW, temperature=0.0)
    assert len(out) == 3
    for row, p, one in zip(out, PROMPTS, singles):
        assert row[:len(p)] == p and len(row) == len(p) + NEW
        assert row == one
    assert ragged.reference_generate(m, PROMPTS, BLOCK, NEW, temperature=0.0) == out


def test_ragged_with_stop_and_logprobs(tiny):
    m, singles = tiny
    gen = [one[len(p):] for one, p in zip(singles, PROMPTS)]
    stop = [gen[1][2:4]]  # row 1's generated tokens 3-4: it finishes after 4 unless they occur earlier
    contexts, infos = m.generate_batch(PROMPTS, BLOCK, NEW, temperature=0.0, stop=stop, logprobs=2)
    assert len(contexts) == len(infos) == 3
    assert infos[1]["finish_reason"] == "stop" and infos[1]["stop_sequence"] == 0
    for p, ctx, info in zip(PROMPTS, contexts, infos):
        one_ctx, one_info = m.generate_tokens([p], BLOCK, NEW, temperature=0.0, stop=stop, logprobs=2)
        assert ctx == one_ctx  # cut where its own one-row call is
        assert info["finish_reason"] == one_info["finish_reason"] and info["stop_sequence"] == one_info["stop_sequence"]
        assert len(info["token_logprobs"]) == len(info["top_logprobs"]) == len(ctx) - len(p)
        assert all(len(top) == 2 for top in info["top_logprobs"])
        assert info["token_logprobs"] == pytest.approx(one_info["token_logprobs"])
    assert len(contexts[1]) < len(PROMPTS[1]) + NEW


def test_stop_token_cuts_every_row_at_the_column_all_rows_share(tiny):
    m, singles = tiny
    full = m.generate_batch(PROMPTS, BLOCK, NEW, temperature=0.0)
    s = full[0][len(PROMPTS[0]) + 2]
    out = m.generate_batch(PROMPTS, BLOCK, NEW, temperature=0.0, stop_token=s)
    gen = [r[len(p):] for r, p in zip(full, PROMPTS)]
    hit = next((j for j in range(NEW) if all(g[j] == s for g in gen)), None)
    keep = NEW if hit is None else hit + 1
    assert out == [r[:len(p) + keep] for r, p in zip(full, PROMPTS)]


def test_rectangular_input_is_what_it_was(tiny):
    m, _ = tiny
    rect = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]]
    with patch.object(ragged, "reference_generate", side_effect=AssertionError("not a ragged call")):
        out = m.generate_batch(rect, BLOCK, NEW, temperature=0.0)
    # (row 0 of the eager per-token loop over the same batch, as the existing suites compare it)
    assert out[0] == list(m._generate_eager(rect, BLOCK, NEW, 0.0, None, None, True))[-1]
    for b, row in enumerate(out):
        assert row == list(m._generate_eager([rect[b]], BLOCK, NEW, 0.0, None, None, True))[-1]


def test_row_zero_calls_refuse_ragged_input(tiny):
    m, _ = tiny
    with pytest.raises(ValueError, match="generate_batch"):
        m.generate_tokens(PROMPTS, BLOCK, NEW, temperature=0.0)
    with pytest.raises(ValueError, match="generate_batch"):
        list(m.generate_tokens_stream(PROMPTS, BLOCK, NEW, temperature=0.0))


def test_bad_ragged_input_fails_before_any_forward(monkeypatch, tiny):
    m, _ = tiny
    monkeypatch.setattr(NeuralNetworkModel, "forward", lambda *a, **k: pytest.fail("forward ran before validation"))
    for bad in ([[1, 2], []], [[1, 2], [V]], [[1], [2, 3.0]]):
        with pytest.raises(ValueError):
            m.generate_batch(bad, BLOCK, NEW, temperature=0.0)
    with pytest.raises(ValueError, match="block_size"):
        m.generate_batch(PROMPTS, 13, NEW, temperature=0.0)
    with pytest.raises(ValueError):  # the call's other checks come first too
        m.generate_batch(PROMPTS, BLOCK, NEW, temperature=0.0, stop=[[V]])


def test_the_fallback_is_logged_once(monkeypatch, tiny, caplog):
    m, _ = tiny
    monkeypatch.setattr(ragged, "_fallback_logged", False)
    with caplog.at_level(logging.INFO, logger=ragged.log.name):
        m.generate_batch(PROMPTS, BLOCK, 2, temperature=0.0)
        m.generate_batch(PROMPTS, BLOCK, 2, temperature=0.0)
    assert sum("one at a time" in r.getMessage() for r in caplog.records) == 1


def test_the_fallback_is_decided_as_the_decoder_lookup_decides(tiny):
    """``_ragged_fallback`` names ``get_decoder``'s reasons for None before the call's options are checked:
    it gives a reason exactly where the lookup gives no ragged decoder (here: no GPU)."""
    from penroz.models import graph_decode as gd
    m, _ = tiny
    assert gd.get_decoder(m, len(PROMPTS), BLOCK, 0.0, None, ragged=True) is None
    assert "no captured decode step here" in m._ragged_fallback()


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": PROMPTS, "block_size": BLOCK, "max_new_tokens": NEW, "temperature": 0.0}


@pytest.fixture
def served(tiny):
    m, _ = tiny
    with patch.object(A, "load_for_serving", return_value=m):
        yield m


def test_api_batch_returns_every_row(served, tiny):
    _, singles = tiny
    r = client.post("/generate/", json={**BODY, "batch": True})
    assert r.status_code == 200 and r.json() == {"sequences": singles}
    gen = singles[1][len(PROMPTS[1]):]
    r = client.post("/generate/", json={**BODY, "batch": True, "stop": [gen[2:4]], "logprobs": 1})
    out = r.json()
    assert r.status_code == 200 and set(out) == {"sequences", "finish_reason", "stop_sequence", "logprobs"}
    assert len(out["sequences"]) == len(out["finish_reason"]) == len(out["stop_sequence"]) == len(out["logprobs"]) == 3
    assert out["finish_reason"][1] == "stop" and out["stop_sequence"][1] == 0
    for seq, p, info in zip(out["sequences"], PROMPTS, out["logprobs"]):
        assert set(info) == {"token_logprobs", "top_logprobs"} and len(info["token_logprobs"]) == len(seq) - len(p)
    # a rectangular batch: every row as well
    r = client.post("/generate/", json={**BODY, "input": [[1, 2], [3, 4]], "batch": True})
    assert r.status_code == 200 and [s[:2] for s in r.json()["sequences"]] == [[1, 2], [3, 4]]


def test_api_batch_with_stream_is_400(served):
    assert client.post("/generate/", json={**BODY, "batch": True, "stream": True}).status_code == 400


def test_api_without_batch_is_what_it_was(served):
    assert client.post("/generate/", json=BODY).status_code == 400  # a ragged input without batch: an error
    r = client.post("/generate/", json={**BODY, "input": [PROMPTS[0]]})
    assert r.status_code == 200 and set(r.json()) == {"tokens"}
    r = client.post("/generate/", json={**BODY, "input": [PROMPTS[0]], "batch": False, "logprobs": 0, "stop": [[7]]})
    assert r.status_code == 200 and set(r.json()) == {"tokens", "finish_reason", "stop_sequence", "logprobs"}
