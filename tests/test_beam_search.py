"""Beam search (ops/beam_search.py) on the CPU: the definition on a table worked out by hand, every refusal, and
``generate_tokens(num_beams=...)`` / ``/generate`` through the reference loop."""
import math
from unittest.mock import patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import beam_search as bs
from penroz.ops.decode_options import check_options
from penroz.serve import app as A

# Next-token probabilities by last token (row 5: the prompt); token 4 is the stop token; W = 2, T = 3.
#   step 1  0 and 1 tie at .4 -> slot 0 = [0], slot 1 = [1] (token ascending); 2 (.1) and 3 (.05, in front of its
#           tie 4) are walked with every slot full.
#   step 2  [0]+4 = .4 * .6 = .24 finishes (A, two tokens); live [1,0] = .4 * .52 = .208 and [1,1] = .08; the
#           fourth candidate is the first of the .04 ties, beam 0 token 0, dropped.
#   step 3  [1,0]+4 = .208 * .6 = .1248 finishes (B); live C = [1,1,0] = .08 * .52 = .0416 and D = [1,0,0] = .0208
#           (in front of its tie [1,0,1]: token ascending).
#   length_penalty 0: scores are log p: A > B > C > D -> A, B.
#   length_penalty 2: A = ln .24 / 4 = -.3568, B = ln .1248 / 9 = -.2312, C = ln .0416 / 9 = -.3533 -> B, then the
#           live C in front of the finished A.
TABLE = torch.tensor([[.10, .10, .10, .10, .60],
                      [.52, .20, .10, .10, .08],
                      [.20, .20, .20, .20, .20],
                      [.20, .20, .20, .20, .20],
                      [.20, .20, .20, .20, .20],
                      [.40, .40, .10, .05, .05]], dtype=torch.float64).log()


def _table_logits(seqs, parents):
    return torch.stack([TABLE[s[-1] if s else 5] for s in seqs])


@pytest.mark.parametrize("penalty, want", [
    (0.0, [([0, 4], .24, True), ([1, 0, 4], .1248, True)]),
    (2.0, [([1, 0, 4], .1248, True), ([1, 1, 0], .0416, False)])])
def test_reference_on_the_hand_worked_table(penalty, want):
    beams = bs.reference_generate(_table_logits, 2, 3, stop_token=4, length_penalty=penalty)
    assert [(b["tokens"], b["finished"]) for b in beams] == [(t, f) for t, _, f in want]
    for b, (tokens, p, _) in zip(beams, want):
        assert b["cum_logprob"] == pytest.approx(math.log(p), abs=1e-12)
        assert b["score"] == pytest.approx(math.log(p) * float(bs.inv_norm_table(3, penalty)[len(tokens)]), abs=1e-12)


def test_reference_tie_order_and_no_stop_token():
    beams = bs.reference_generate(_table_logits, 2, 1)
    assert [b["tokens"] for b in beams] == [[0], [1]] and not any(b["finished"] for b in beams)
    beams = bs.reference_generate(_table_logits, 2, 3)  # nothing finishes: 4 is a token like any other
    # live after step 2: [0,4] = .24 and [1,0] = .208; step 3: [1,0,4] = .1248, then the five-way tie [0,4,*] = .048
    assert [b["tokens"] for b in beams] == [[1, 0, 4], [0, 4, 0]]


SHAPE = {"rows": 1, "prompt_len": 5, "block_size": 32, "stream": False}
REFUSED = [({"num_beams": 1}, {}), ({"num_beams": 9}, {}), ({"num_beams": True}, {}), ({"num_beams": 2.0}, {}),
           ({"length_penalty": float("inf")}, {}), ({"length_penalty": float("nan")}, {}), ({"length_penalty": "1"}, {}),
           ({}, {"rows": 2}), ({}, {"prompt_len": 27}), ({}, {"stream": True}), ({}, {"batch": True}),
           ({"top_p": 0.9}, {}), ({"min_p": 0.1}, {}), ({"repetition_penalty": 1.2}, {}), ({"presence_penalty": 0.5}, {}),
           ({"frequency_penalty": 0.5}, {}), ({"logit_bias": {3: 1.0}}, {}), ({"banned_token_ids": [3]}, {}),
           ({"allowed_token_ids": [3, 4]}, {}), ({"min_tokens": 2}, {}), ({"stop": [[3]]}, {}), ({"logprobs": 0}, {}),
           ({"prompt_logprobs": True}, {}), ({"speculate": 1}, {}), ({"n": 2}, {}), ({"share_prefix": True}, {"batch": True})]


@pytest.mark.parametrize("options, shape", REFUSED, ids=lambda d: "-".join(d) or "x")
def test_refusals(options, shape):
    kw = {"num_beams": 2, **options}
    with pytest.raises(ValueError):
        check_options(256, 6, 0.0 if "speculate" in options else 1.0, None, 7 if "min_tokens" in options else None, **kw,
                      call_shape={**SHAPE, **shape})


def test_refuses_temperature_and_top_k_and_takes_neutral_values():
    for temperature, top_k in ((0.0, None), (0.7, None), (1.0, 5)):
        with pytest.raises(ValueError):
            check_options(256, 6, temperature, top_k, num_beams=2, call_shape=SHAPE)
    o = check_options(256, 6, 1.0, None, 7, num_beams=4, length_penalty=0.5, top_p=1.0, min_p=0.0, call_shape=SHAPE)
    assert (o.num_beams, o.length_penalty, o.stop_token) == (4, 0.5, 7)
    assert check_options(256, 6, 1.0, None, length_penalty=2.0) == check_options(256, 6, 1.0, None)  # no beams: neutral


V, BLOCK, NEW, PROMPT = 256, 32, 6, [3, 1, 4, 1, 5]


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return NeuralNetworkModel("bm", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 3e-3}}))


def test_generate_tokens_returns_beams_best_first(tiny):
    tokens, info = tiny.generate_tokens([PROMPT], BLOCK, NEW, num_beams=2, length_penalty=1.0)
    beams = info["beams"]
    assert tiny.last_beam_search["path"] == "reference" and len(beams) == 2
    assert tokens == PROMPT + beams[0]["tokens"] and beams[0]["score"] >= beams[1]["score"]
    assert beams[0]["tokens"] != beams[1]["tokens"] and all(len(b["tokens"]) == NEW for b in beams)
    # the cached rows, re-parented with index_select, score what a cache-free pass scores
    with torch.inference_mode():
        for b in beams:
            x = torch.tensor([PROMPT + b["tokens"]])
            logp = torch.log_softmax(tiny._forward_nocache(x)[0][-1][0].double(), dim=-1)
            want = logp[torch.arange(len(PROMPT) - 1, x.shape[1] - 1), x[0, len(PROMPT):]].sum().item()
            assert b["cum_logprob"] == pytest.approx(want, abs=1e-3)
    with pytest.raises(ValueError):
        tiny.generate_batch([PROMPT], BLOCK, NEW, num_beams=2)
    with pytest.raises(ValueError):
        list(tiny.generate_tokens_stream([PROMPT], BLOCK, NEW, num_beams=2))
    with pytest.raises(ValueError):
        tiny.generate_tokens([PROMPT], BLOCK, BLOCK, num_beams=2)  # the window would slide


def test_api_answers_with_beams_and_refuses_before_loading(tiny):
    client = TestClient(main.app, raise_server_exceptions=False)
    body = {"model_id": "t", "input": PROMPT, "block_size": BLOCK, "max_new_tokens": NEW, "temperature": 1.0, "num_beams": 3}
    with patch.object(A, "load_for_serving", return_value=tiny):
        r = client.post("/generate/", json=body)
        assert r.status_code == 200
        out = r.json()
        assert len(out["beams"]) == 3 and out["tokens"] == PROMPT + out["beams"][0]["tokens"]
    with patch.object(A, "load_for_serving", side_effect=AssertionError("loaded before the check")):
        for bad in ({"stream": True}, {"batch": True}, {"num_beams": 9}, {"top_k": 5}, {"length_penalty": "x"}):
            assert client.post("/generate/", json={**body, **bad}).status_code in (400, 422), bad
