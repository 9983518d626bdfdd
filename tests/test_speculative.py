"""Prompt-lookup speculative decoding on the CPU (ops/speculative.py): ``draft`` and ``accept`` on hand-made
cases, ``reference_generate`` against the plain greedy loop, every refusal through ``check_options``, the
public methods and /generate, neutral values, and the plain-path fallback."""
import logging
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import speculative as spec
from penroz.ops.decode_options import KEYWORDS, NOT_LOADED, DecodeOptions, check_options
from penroz.serve import app as A

V = 64


# ------------------------------------------------------------------ draft / accept
def test_draft_on_one_token_repeats_it():
    assert spec.draft([5], 3) == [5, 5, 5]
    assert spec.draft([5], 1) == [5]


def test_draft_without_a_match_repeats_the_last_token():
    assert spec.draft([1, 2, 3, 4], 2) == [4, 4]


def test_draft_match_only_at_one_token():
    # the suffixes [9, 3] and [4, 9, 3] occur nowhere earlier; 3 does, at 1: what followed is 7, 8
    assert spec.draft([0, 3, 7, 8, 4, 9, 3], 2) == [7, 8]


def test_draft_longest_ngram_wins_over_a_later_shorter_match():
    # [1, 2, 3] occurs at 0 (followed by 50); the later matches of [2, 3] at 5 and of [3] at 6 are followed by 60
    hist = [1, 2, 3, 50, 51, 2, 3, 60, 1, 2, 3]
    assert spec.draft(hist, 2) == [50, 51]
    assert spec.draft(hist, 2, max_ngram=2) == [60, 1]
    assert spec.draft(hist, 1, max_ngram=1) == [60]


def test_draft_latest_start_wins():
    hist = [1, 2, 3, 40, 1, 2, 3, 41, 1, 2, 3]
    assert spec.draft(hist, 1) == [41]


def test_draft_continues_through_itself():
    # the only match of [7, 8] ends right in front of the suffix: the continuation runs into the draft
    assert spec.draft([7, 8, 7, 8], 3) == [7, 8, 7]
    # a one-token loop
    assert spec.draft([4, 4], 3) == [4, 4, 4]
    # a match whose continuation has one real token, then the draft's own
    assert spec.draft([1, 2, 9, 1, 2], 3) == [9, 1, 2]


def test_draft_never_matches_the_suffix_with_itself():
    # j ranges to n - m - 1: the suffix itself (j = n - m) is no match
    assert spec.draft([1, 2, 3], 2) == [3, 3]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_accept_counts_the_leading_confirmed_drafts(k):
    drafts = [10, 11, 12][:k]
    for a in range(k + 1):
        cand = drafts[:a] + [99] * (k + 1 - a)  # rows 0..a-1 confirm their draft, row a does not
        assert spec.accept(drafts, cand) == a
    # a later agreement behind a rejection does not count
    if k >= 2:
        assert spec.accept(drafts, [99] + drafts[1:] + [0]) == 0


def test_advance_emits_up_to_the_limit_and_the_room():
    hist = [1, 2, 3]
    assert spec.advance(hist, [7, 8], [7, 8, 9], emitted=0, limit=10, capacity=32) == (3, 2) and hist == [1, 2, 3, 7, 8, 9]
    assert spec.advance(hist, [7, 8], [7, 8, 9], emitted=9, limit=10, capacity=32) == (1, 0) and hist[-1] == 7
    assert spec.advance(hist, [7, 8], [7, 8, 9], emitted=10, limit=10, capacity=32) == (0, 0)  # frozen
    full = list(range(8))
    assert spec.advance(full, [7, 8], [7, 8, 9], emitted=0, limit=10, capacity=11) == (1, 0)  # 11 - 2 - 8
    assert spec.advance(full, [7, 8], [7, 8, 9], emitted=0, limit=10, capacity=11) == (0, 0)


# ------------------------------------------------------------------ the loop
def _plain(fn, prompt, max_new):
    hist = list(prompt)
    for _ in range(max_new):
        hist.append(fn(hist))
    return hist


TOYS = {
    "two-mod-7": lambda h: (3 * h[-1] + (h[-2] if len(h) > 1 else 0) + 1) % 7,
    "period-3": lambda h: [4, 5, 6][len(h) % 3],
    "counter": lambda h: (len(h) * len(h)) % 11,
}


@pytest.mark.parametrize("k", [1, 2, 3])
def test_reference_generate_is_the_plain_greedy_loop(k):
    accepted = drafted = 0
    for name, fn in TOYS.items():
        for prompt in ([3], [1, 2], [1, 2, 3, 1, 2]):
            for max_new in (1, 5, 40):
                stats = {}
                got = spec.reference_generate(fn, prompt, max_new, k, stats)
                assert got == _plain(fn, prompt, max_new), (name, prompt, max_new)
                assert stats["drafted"] == stats["steps"] * k and 0 <= stats["accepted"] <= stats["drafted"]
                assert stats["steps"] + stats["accepted"] == max_new  # every step emits one token more than it accepted
                accepted, drafted = accepted + stats["accepted"], drafted + stats["drafted"]
    assert 0 < accepted < drafted  # some drafts were accepted, some rejected


def test_reference_generate_accepts_everything_on_a_loop():
    stats = {}
    got = spec.reference_generate(lambda h: h[-1], [9], 16, 3, stats)
    assert got == [9] * 17 and stats == {"steps": 4, "drafted": 12, "accepted": 12}


# ------------------------------------------------------------------ the checks
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return NeuralNetworkModel("spec", Mapper(bench.gpt2_layers(V=V, C=32, L=1, H=2, P=16), {"adamw": {"lr": 1e-3}}))


SHAPE = dict(rows=1, prompt_len=2, block_size=16, stream=False)
REFUSED = [
    (dict(speculate=4), "speculate must be None, 0 or an integer in [1, 3], got 4"),
    (dict(speculate=-1), "speculate must be None, 0 or an integer in [1, 3], got -1"),
    (dict(speculate=True), "speculate must be None, 0 or an integer in [1, 3], got True"),
    (dict(speculate=1.5), "speculate must be None, 0 or an integer in [1, 3], got 1.5"),
    (dict(speculate=2, repetition_penalty=1.3), "speculate does not compose with repetition_penalty"),
    (dict(speculate=2, presence_penalty=0.5), "speculate does not compose with presence_penalty"),
    (dict(speculate=2, frequency_penalty=0.5), "speculate does not compose with frequency_penalty"),
    (dict(speculate=2, logprobs=0), "speculate does not compose with logprobs"),
    (dict(speculate=2, stop=[[1, 2]]), "speculate does not compose with stop"),
    (dict(speculate=2, logit_bias={1: 2.0}), "speculate does not compose with logit_bias"),
    (dict(speculate=2, banned_token_ids=[3]), "speculate does not compose with banned_token_ids"),
    (dict(speculate=2, allowed_token_ids=[3, 4]), "speculate does not compose with allowed_token_ids"),
]


def _text(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize("bad,text", REFUSED, ids=[" ".join(f"{k}" for k in b) + f" {b['speculate']}" for b, _ in REFUSED])
def test_refusals_in_the_checker_and_the_public_methods(model, bad, text):
    assert _text(lambda: check_options(V, 4, 0.0, None, **bad, call_shape=SHAPE)) == text
    assert _text(lambda: check_options(NOT_LOADED, 4, 0.0, None, **bad)) == text
    assert _text(lambda: model.generate_tokens([[1, 2]], 16, 4, temperature=0.0, **bad)) == text
    assert _text(lambda: model.generate_batch([[1, 2]], 16, 4, temperature=0.0, **bad)) == text


def test_refusals_that_depend_on_the_call(model):
    with patch.object(model, "forward", side_effect=AssertionError("a forward pass ran")):
        # min_tokens needs an end token to be an option at all
        assert _text(lambda: model.generate_tokens([[1, 2]], 16, 4, 0.0, None, 5, speculate=2, min_tokens=2)) \
            == "speculate does not compose with min_tokens"
        assert "greedy decoding (temperature 0), got temperature 0.7" in \
            _text(lambda: model.generate_tokens([[1, 2]], 16, 4, temperature=0.7, speculate=2))
        assert _text(lambda: model.generate_tokens([[1, 2], [3, 4]], 16, 4, temperature=0.0, speculate=2)) \
            == "speculate takes one sequence, got 2 rows"
        assert _text(lambda: model.generate_batch([[1, 2], [3, 4]], 16, 4, temperature=0.0, speculate=2)) \
            == "speculate takes one sequence, got 2 rows"
        assert _text(lambda: model.generate_batch([[1, 2], [3]], 16, 4, temperature=0.0, speculate=2)) \
            == "speculate takes one sequence, got 2 rows"
        assert "does not stream" in _text(lambda: list(model.generate_tokens_stream([[1, 2]], 16, 4, temperature=0.0, speculate=1)))
        window = ("a speculative call does not slide its window: prompt (2) + max_new_tokens (12) + speculate (3) "
                  "must be <= block_size (16)")
        assert _text(lambda: model.generate_tokens([[1, 2]], 16, 12, temperature=0.0, speculate=3)) == window
        assert _text(lambda: model.generate_tokens([1, 2], 16, 12, temperature=0.0, speculate=3)) == window
        assert _text(lambda: model.generate_batch([[1, 2]], 16, 12, temperature=0.0, speculate=3)) == window
    assert len(model.generate_tokens([[1, 2]], 16, 11, temperature=0.0, speculate=3)) == 13  # 2 + 11 + 3 == 16 fits


def test_neutral_values_give_the_unchanged_options():
    plain = check_options(V, 4, 0.0, None)
    assert plain == DecodeOptions(temperature=0.0) and plain.speculate is None
    for off in (None, 0):
        o = check_options(V, 4, 0.0, None, speculate=off, call_shape=SHAPE)
        assert o == plain and o.describe() == ""
    assert check_options(V, 4, 1.0, 5, speculate=0, call_shape=dict(rows=3, stream=True)) == check_options(V, 4, 1.0, 5)
    on = check_options(V, 4, 0.0, None, 7, speculate=2, weight_quant="int8", repetition_penalty=1.0, stop=[],
                       logit_bias={}, banned_token_ids=[], min_tokens=0, call_shape=SHAPE)
    assert on.speculate == 2 and on.stop_token == 7 and on.weight_quant == "int8" and on != plain
    assert on.describe() == " repetition_penalty 1.0 speculate 2"
    assert "speculate" in KEYWORDS and "call_shape" not in KEYWORDS


def test_cpu_fallback_returns_the_plain_calls_tokens(model, caplog):
    spec._fallback_logged = False
    with caplog.at_level(logging.INFO, logger="penroz.ops.speculative"):
        plain = model.generate_tokens([[1, 2, 3]], 16, 8, temperature=0.0)
        for k in (1, 3):
            assert model.generate_tokens([[1, 2, 3]], 16, 8, temperature=0.0, speculate=k) == plain
        assert model.generate_batch([[1, 2, 3]], 16, 8, temperature=0.0, speculate=2) == [plain]
    assert model.last_speculation == {"steps": 0, "drafted": 0, "accepted": 0}
    assert sum("plain decode path" in m for m in caplog.messages) == 1  # logged once per process
    stop = plain[5]
    cut = model.generate_tokens([[1, 2, 3]], 16, 8, temperature=0.0, stop_token=stop)
    assert model.generate_tokens([[1, 2, 3]], 16, 8, temperature=0.0, stop_token=stop, speculate=2) == cut


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1, 2]], "block_size": 16, "max_new_tokens": 4, "temperature": 0.0}


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m) as load:
        m.load = load
        yield m


def test_api_forwards_speculate_only_when_set_and_reports_the_statistics(served):
    served.generate_tokens.return_value = [1, 2, 3]
    served.last_speculation = {"steps": 1, "drafted": 2, "accepted": 0}
    r = client.post("/generate/", json={**BODY, "speculate": 2, "stop_token": 9, "weight_quant": "int8"})
    assert r.status_code == 200
    assert r.json() == {"tokens": [1, 2, 3], "speculation": {"steps": 1, "drafted": 2, "accepted": 0}}
    assert served.generate_tokens.call_args.kwargs["speculate"] == 2
    for body in (BODY, {**BODY, "speculate": None}, {**BODY, "speculate": 0}):
        r = client.post("/generate/", json=body)
        assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
        assert "speculate" not in served.generate_tokens.call_args.kwargs
    served.generate_batch.return_value = [[1, 2, 3]]
    r = client.post("/generate/", json={**BODY, "speculate": 1, "batch": True})
    assert r.json() == {"sequences": [[1, 2, 3]], "speculation": {"steps": 1, "drafted": 2, "accepted": 0}}
    assert served.generate_batch.call_args.kwargs["speculate"] == 1


@pytest.mark.parametrize("bad", [
    {"speculate": 4}, {"speculate": -1}, {"speculate": True}, {"speculate": 1.5}, {"speculate": 2, "temperature": 0.7},
    {"speculate": 2, "input": [[1, 2], [3, 4]]}, {"speculate": 2, "input": [[1, 2], [3]], "batch": True},
    {"speculate": 2, "stream": True}, {"speculate": 2, "repetition_penalty": 1.3}, {"speculate": 2, "presence_penalty": 0.5},
    {"speculate": 2, "frequency_penalty": 0.5}, {"speculate": 2, "logprobs": 0}, {"speculate": 2, "stop": [[1, 2]]},
    {"speculate": 2, "logit_bias": {"1": 2.0}}, {"speculate": 2, "banned_token_ids": [3]},
    {"speculate": 2, "allowed_token_ids": [3, 4]}, {"speculate": 2, "min_tokens": 2, "stop_token": 5},
    {"speculate": 3, "max_new_tokens": 12},
], ids=["k>3", "k<0", "bool", "float", "temperature", "rows", "ragged", "stream", "repetition", "presence", "frequency",
        "logprobs", "stop", "logit_bias", "banned", "allowed", "min_tokens", "window"])
def test_api_refusal_is_400_before_the_model_is_loaded(served, bad):
    # (a value that is no integer fails the schema, as for every integer field of the request: 422)
    assert client.post("/generate/", json={**BODY, **bad}).status_code == (422 if bad["speculate"] in (True, 1.5) else 400)
    served.load.assert_not_called()
    served.generate_tokens.assert_not_called()
    served.generate_tokens_stream.assert_not_called()
    served.generate_batch.assert_not_called()
