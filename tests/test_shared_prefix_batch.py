"""``share_prefix`` (ops/shared_prefix.py): the split, what the option refuses, and the CPU call, which is the plain one."""
import pytest
import torch

import bench
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import shared_prefix as sp

HEAD = [3, 1, 4, 1, 5]
PROMPTS = [HEAD + [9], HEAD + [2, 6], HEAD + [5, 3, 5]]


@pytest.mark.parametrize("prompts, want", [
    (PROMPTS, 5),
    ([[1, 2, 3], [1, 2, 3]], 2),        # equal rows keep a remainder of one token
    ([[1, 2], [1, 2, 3, 4]], 1),        # the shortest row bounds the split
    ([[1, 2, 3], [4, 2, 3]], 0),        # nothing in common
    ([[7], [7, 8]], 0)])                # a one-token row has no prefix to give
def test_split(prompts, want):
    assert sp.split_prompts(prompts) == want


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(2)
    return NeuralNetworkModel("spb", Mapper(bench.gpt2_layers(V=64, C=32, L=1, H=2, P=16), {"adamw": {"lr": 1e-3}})).eval()


@pytest.mark.parametrize("call, options, text", [
    ("generate_batch", {"n": 2}, "not both"),
    ("generate_batch", {"speculate": 2, "temperature": 0.0}, "speculate"),
    ("generate_tokens", {}, "generate_batch"),
    ("generate_tokens_stream", {}, "generate_batch"),
    ("generate_batch", {"rows": [HEAD + [9]]}, "2 to 64"),
    ("generate_batch", {"new": 9}, "slide")])
def test_refusals_come_before_any_forward_pass(model, monkeypatch, call, options, text):
    monkeypatch.setattr(model, "forward", lambda *a, **k: pytest.fail("a forward pass ran"))
    options = dict(options)
    rows, new = options.pop("rows", PROMPTS), options.pop("new", 4)
    rows = rows if call == "generate_batch" else rows[:1]
    with pytest.raises(ValueError, match=text):
        out = getattr(model, call)(rows, 16, new, **{"temperature": 1.0, **options}, share_prefix=True)
        list(out)  # (the stream is a generator)
    with pytest.raises(ValueError, match="stream"):
        sp.check_share_prefix(True, rows=3, stream=True)


def test_the_cpu_call_is_the_plain_call(model):
    torch.manual_seed(7)
    plain = model.generate_batch(PROMPTS, 16, 4, temperature=1.0, top_k=8, logprobs=0)
    torch.manual_seed(7)
    shared = model.generate_batch(PROMPTS, 16, 4, temperature=1.0, top_k=8, logprobs=0, share_prefix=True)
    assert shared == plain and model.last_shared_prefix is None
    assert [c[:len(p)] for c, p in zip(shared[0], PROMPTS)] == PROMPTS
