"""The generate calls' checked options (ops/decode_options.py): every refusal with the text the public
methods have always given, in the order they have always been reached; neutral values; the log line."""
import inspect

import pytest
import torch

import bench
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.decode_options import KEYWORDS, NOT_LOADED, DecodeCall, DecodeOptions, check_options

V, NEW = 256, 4
BOTH = "give stop_token or stop, not both (a stop_token s is the stop sequence [s])"
NO_VOCABULARY = ("logit_bias / banned_token_ids / allowed_token_ids / min_tokens need a model whose layer list ends "
                 "with the vocabulary projection")

# one per check, in the order the checks run; the texts are those of the commit before this module existed
REFUSED = [
    (dict(top_p=0.0), "top_p must be in (0, 1], got 0.0"),
    (dict(min_p=1.0), "min_p must be in [0, 1), got 1.0"),
    (dict(weight_quant="int4"), "weight_quant must be one of ('int8',) (or empty for bf16 weights), got 'int4'"),
    (dict(repetition_penalty=0.0), "repetition_penalty must be finite and > 0, got 0.0"),
    (dict(presence_penalty=float("inf")), "presence_penalty must be finite, got inf"),
    (dict(frequency_penalty=float("nan")), "frequency_penalty must be finite, got nan"),
    (dict(logprobs=21), "logprobs must be in [0, 20], got 21"),
    (dict(logprobs=1.5), "logprobs must be None or an integer in [0, 20], got 1.5"),
    (dict(stop=[[1], []]), "stop[1] must hold 1 to 8 token ids, got 0"),
    (dict(stop=[[V]]), f"stop[0]: token id {V} is outside [0, {V})"),
    (dict(stop=[[1]], stop_token=1), BOTH),
    (dict(logit_bias={1: 101}), "logit_bias[1] must be finite and in [-100, 100], got 101"),
    (dict(banned_token_ids=[V]), f"banned_token_ids: token id {V} is outside [0, {V})"),
    (dict(allowed_token_ids=[]), "allowed_token_ids must hold at least one token id (None: no restriction)"),
    (dict(min_tokens=NEW + 1), f"min_tokens must be in [0, max_new_tokens = {NEW}], got {NEW + 1}"),
    (dict(allowed_token_ids=[1], banned_token_ids=[1]),
     "no token would stay unmasked: the allowed set (or the vocabulary) minus the banned ids is empty"),
]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return NeuralNetworkModel("opts", Mapper(bench.gpt2_layers(V=V, C=32, L=1, H=2, P=16), {"adamw": {"lr": 1e-3}}))


def _text(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize("bad,text", REFUSED, ids=[" ".join(b) for b, _ in REFUSED])
def test_refusals_keep_their_texts_in_the_checker_and_the_public_methods(model, bad, text):
    assert _text(lambda: check_options(V, NEW, 0.0, None, **bad)) == text
    assert _text(lambda: model.generate_tokens([[1, 2]], 8, NEW, temperature=0.0, **bad)) == text
    assert _text(lambda: list(model.generate_tokens_stream([[1, 2]], 8, NEW, temperature=0.0, **bad))) == text
    assert _text(lambda: model.generate_batch([[1, 2]], 8, NEW, temperature=0.0, **bad)) == text


def test_of_two_bad_values_the_first_check_in_order_speaks():
    order = [bad for bad, _ in REFUSED if "stop_token" not in bad]
    for i, (first, text) in enumerate(REFUSED):
        for later in order[i + 1:]:
            if set(first) & set(later) or ("stop" in first and "stop" in later):
                continue
            assert _text(lambda: check_options(V, NEW, 0.0, None, **first, **later)) == text, (first, later)
    # stop_token with stop comes behind the stop set's own check and in front of the logit bias'
    assert _text(lambda: check_options(V, NEW, 0.0, None, 1, stop=[[1]], logit_bias={1: 101})) == BOTH
    assert _text(lambda: check_options(V, NEW, 0.0, None, 1, stop=[[V]])) == REFUSED[9][1]


def test_unknown_keyword_is_a_type_error(model):
    with pytest.raises(TypeError):
        check_options(V, NEW, 0.0, None, no_such_option=1)
    with pytest.raises(TypeError):
        list(model._generate_eager([[1, 2]], 8, NEW, 0.0, None, None, True, no_such_option=1))


def test_keywords_are_the_public_methods_own():
    for method in (NeuralNetworkModel.generate_tokens, NeuralNetworkModel.generate_tokens_stream,
                   NeuralNetworkModel.generate_batch):
        own = [n for n, p in inspect.signature(method).parameters.items() if p.kind is p.KEYWORD_ONLY]
        assert sorted(own) == sorted(KEYWORDS), method.__name__


def test_neutral_values_are_the_defaults():
    plain = check_options(V, NEW, 1.0, 5)
    assert plain == DecodeOptions(temperature=1.0, top_k=5)
    neutral = check_options(V, NEW, 1.0, 5, None, top_p=None, min_p=None, weight_quant="", repetition_penalty=1.0,
                            presence_penalty=0.0, frequency_penalty=0.0, logprobs=None, stop=[], logit_bias={},
                            banned_token_ids=[], allowed_token_ids=None, min_tokens=0)
    assert neutral == plain
    assert check_options(V, NEW, 1.0, 5, logit_bias={3: 0.0}, min_tokens=2).bias is None  # (no end token to hold back)
    assert (plain.penalties, plain.logprobs, plain.stop, plain.bias, plain.min_tokens) == (None, None, None, None, 0)
    call = DecodeCall(plain, 2, "cpu")
    assert (call.penalties, call.stop, call.bias, call.logprobs, call.produced) == (None, None, None, None, 0)


def test_canonical_fields():
    o = check_options(V, 8, 1.0, 20, top_p=0.9, repetition_penalty=1.3, logprobs=3, stop=[(7,), [8, 9]],
                      logit_bias={"5": 2.0}, banned_token_ids=[3], min_tokens=2)
    assert (o.temperature, o.top_k, o.top_p, o.min_p, o.weight_quant) == (1.0, 20, 0.9, None, None)
    assert o.penalties == (1.3, 0.0, 0.0) and o.logprobs == 3 and o.stop == [[7], [8, 9]] and o.min_tokens == 2
    assert o.bias.entries == [(3, -float("inf"), 0), (5, 2.0, 0), (7, 0.0, 2)] and o.bias.V == V
    assert check_options(V, 8, 0.0, None, 7, min_tokens=2).bias.entries == [(7, 0.0, 2)]  # stop_token is an end token
    call = DecodeCall(o, 2, "cpu")
    assert call.penalties.values == o.penalties and call.stop.stop == o.stop and call.bias.canonical == o.bias


def test_without_a_vocabulary():
    """V NOT_LOADED: the service's early check takes any int32 id; V None, a model that shows no
    vocabulary, refuses what rewrites logits by id, behind every other check."""
    early = check_options(NOT_LOADED, NEW, 0.0, None, banned_token_ids=[2 ** 31 - 1], stop=[[2 ** 31 - 1]])
    assert early.bias.V is None and early.bias.ids == (2 ** 31 - 1,)
    assert _text(lambda: check_options(NOT_LOADED, NEW, 0.0, None, banned_token_ids=[2 ** 31])) \
        == f"banned_token_ids: token id {2 ** 31} is outside [0, {2 ** 31})"
    assert _text(lambda: check_options(None, NEW, 0.0, None, banned_token_ids=[1])) == NO_VOCABULARY
    assert _text(lambda: check_options(None, NEW, 0.0, None, banned_token_ids=[1], min_tokens=NEW + 1)) == REFUSED[14][1]
    assert check_options(None, NEW, 0.0, None, stop=[[5]], logprobs=1).bias is None


def test_describe_is_the_log_line_fragment(model, caplog):
    asked = dict(top_p=0.9, min_p=0.05, weight_quant="", repetition_penalty=1.3, presence_penalty=0.2,
                 frequency_penalty=0.1, logprobs=3, stop=[[7], [8, 9]], logit_bias={5: 2.0, "9": -1.0},
                 banned_token_ids=[3], allowed_token_ids=list(range(64)), min_tokens=2)
    want = (" top 20 top_p 0.9 min_p 0.05 repetition_penalty 1.3 presence_penalty 0.2 frequency_penalty 0.1 logprobs 3"
            " stop 2 sequences logit bias 4 entries 64 allowed ids min_tokens 2")
    assert check_options(V, 8, 1.0, 20, **asked).describe() == want
    assert check_options(V, 8, 0.0, None).describe() == ""
    # the values as given: a neutral one that was spelled out is named, min_tokens without an effect is not
    assert check_options(V, 8, 0.0, None, 4, min_tokens=0, repetition_penalty=1.0, stop=[]).describe() \
        == " repetition_penalty 1.0"
    with caplog.at_level("INFO", logger="penroz.models.model"):
        model._prepare_generation([[1, 2]], 8, 1.0, 20, **asked)
    assert caplog.messages[-1] == f"Generating at most 8{want} tokens with 1.0 temperature using device cpu"
