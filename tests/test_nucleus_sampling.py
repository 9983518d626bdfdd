"""Nucleus (top-p) and min-p sampling on the CPU: ``reference_sample`` against an fp64 oracle
written here from the definition, generation through a tiny model, and the /generate schema."""
import math
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.sampling import reference_sample
from penroz.serve import app as A


def oracle_kept(row, T, top_k=None, top_p=None, min_p=None):
    """fp64, from the definition: (kept indices in descending-logit order, their probabilities).
    S = the top_k largest; w = exp((x - max)/T); top-p keeps i iff the mass of the strictly
    larger logits is < top_p * Z; min-p keeps i iff w_i >= min_p."""
    x = [float(v) for v in row]
    order = sorted(range(len(x)), key=lambda i: (-x[i], i))
    if top_k is not None and top_k < len(x):
        order = order[:top_k]
    mx = x[order[0]]
    w = {i: math.exp((x[i] - mx) / T) for i in order}
    Z = sum(w.values())
    kept = []
    for i in order:
        above = sum(w[j] for j in order if x[j] > x[i])
        if top_p is not None and top_p < 1.0 and not above < top_p * Z:
            continue
        if min_p is not None and w[i] < min_p:
            continue
        kept.append(i)
    tot = sum(w[i] for i in kept)
    return kept, [w[i] / tot for i in kept]


def sweep(row, T, top_k, n=4001, **kw):
    """tokens drawn for n uniforms spread over [0, 1)"""
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    logits = torch.tensor(row, dtype=torch.float32).repeat(n, 1)
    return reference_sample(logits, T, top_k, u.float(), **kw).view(-1).tolist()


ROW = [2.0, -1.0, 0.5, 1.5, -3.0, 1.0, 0.0, -0.5]


@pytest.mark.parametrize("top_p", [0.3, 0.6, 0.9, 0.99])
def test_kept_set_and_frequencies_match_the_oracle(top_p):
    T = 0.7
    kept, probs = oracle_kept(ROW, T, top_p=top_p)
    assert len(kept) < len(ROW)
    drawn = sweep(ROW, T, None, top_p=top_p)
    assert set(drawn) == set(kept)
    for i, p in zip(kept, probs):  # the sweep is a quadrature of the inverse CDF: 1/n per cell
        assert abs(drawn.count(i) / len(drawn) - p) < 2e-3, (i, p)
    # descending-logit draw order: the smallest uniform draws the maximum
    assert drawn[0] == 0


def test_tie_straddling_the_cut_keeps_both():
    # w = 1, 1/2, 1/2, 1/8 (T = 1, logits ln-spaced): the mass above the tied pair is 1 of Z = 2.125
    row = [0.0, math.log(0.5), math.log(0.5), math.log(0.125), -30.0]
    for top_p in (0.5, 0.6, 0.7):  # 0.47 < top_p: the pair is in; one of the pair alone reaches 0.706
        kept, _ = oracle_kept(row, 1.0, top_p=top_p)
        assert kept == [0, 1, 2]
        assert set(sweep(row, 1.0, None, top_p=top_p)) == {0, 1, 2}
    assert set(sweep(row, 1.0, None, top_p=0.4)) == {0}  # the pair leaves together
    assert set(sweep(row, 1.0, None, top_p=0.95)) == {0, 1, 2, 3}


def test_off_values_equal_the_plain_call():
    torch.manual_seed(0)
    logits = torch.randn(16, 50) * 2
    u = torch.rand(16)
    for k in (None, 7):
        base = reference_sample(logits, 0.8, k, u)
        assert torch.equal(reference_sample(logits, 0.8, k, u, top_p=1.0, min_p=0.0), base)
        assert torch.equal(reference_sample(logits, 0.8, k, u, None, None), base)


def test_min_p_alone():
    T = 0.7
    for min_p in (0.05, 0.3, 0.6):
        kept, probs = oracle_kept(ROW, T, min_p=min_p)
        assert 1 <= len(kept) < len(ROW)
        drawn = sweep(ROW, T, None, min_p=min_p)
        assert set(drawn) == set(kept)
        for i, p in zip(kept, probs):
            assert abs(drawn.count(i) / len(drawn) - p) < 2e-3
    assert set(sweep(ROW, T, None, min_p=0.999999)) == {0}


def test_top_k_then_top_p_renormalises_over_the_top_k_set():
    T = 1.0
    # over the whole row top_p = 0.8 keeps more than over the top-3 set, whose Z is smaller
    kept_all, _ = oracle_kept(ROW, T, top_p=0.8)
    kept_k, probs_k = oracle_kept(ROW, T, top_k=3, top_p=0.8)
    assert set(kept_k) < set(kept_all) and set(kept_k) <= {0, 3, 5}
    drawn = sweep(ROW, T, 3, top_p=0.8)
    assert set(drawn) == set(kept_k)
    for i, p in zip(kept_k, probs_k):
        assert abs(drawn.count(i) / len(drawn) - p) < 2e-3
    both, _ = oracle_kept(ROW, T, top_k=5, top_p=0.95, min_p=0.3)
    assert set(sweep(ROW, T, 5, top_p=0.95, min_p=0.3)) == set(both)


def test_temperature_zero_ignores_both_and_ranges_are_checked():
    logits = torch.tensor([ROW, ROW[::-1]])
    u = torch.tensor([0.9, 0.9])
    assert reference_sample(logits, 0.0, None, u, top_p=0.1, min_p=0.9).view(-1).tolist() == [0, 7]
    for bad in ({"top_p": 0.0}, {"top_p": 1.5}, {"min_p": -0.1}, {"min_p": 1.0}):
        with pytest.raises(ValueError):
            reference_sample(logits, 1.0, None, u, **bad)


# ------------------------------------------------------------------ tiny model
def gpt():
    torch.manual_seed(0)
    return NeuralNetworkModel("gpt", Mapper(bench.gpt2_layers(V=64, C=32, L=2, H=2, P=32), {"adamw": {"lr": 3e-3}}))


def test_generation_with_a_vanishing_nucleus_is_greedy():
    m = gpt()
    greedy = m.generate_tokens([[1, 2, 3]], 8, 10, temperature=0.0)
    assert m.generate_tokens([[1, 2, 3]], 8, 10, temperature=1.0, top_p=1e-6) == greedy
    assert m.generate_tokens([[1, 2, 3]], 8, 10, temperature=1.0, min_p=0.999999) == greedy
    assert list(m.generate_tokens_stream([[1, 2, 3]], 8, 10, temperature=1.0, top_p=1e-6)) == greedy[3:]
    assert m.generate_batch([[1, 2, 3], [1, 2, 3]], 8, 4, temperature=1.0, top_p=1e-6) == [greedy[:7]] * 2
    with pytest.raises(ValueError):
        m.generate_tokens([[1]], 8, 2, temperature=1.0, top_p=0.0)


def test_stream_equals_non_stream_under_one_seed():
    m = gpt()
    torch.manual_seed(5)
    a = m.generate_tokens([[1, 2]], 8, 8, temperature=1.0, top_p=0.9, min_p=0.01)
    torch.manual_seed(5)
    b = [1, 2] + list(m.generate_tokens_stream([[1, 2]], 8, 8, temperature=1.0, top_p=0.9, min_p=0.01))
    assert a == b


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1]], "block_size": 8, "max_new_tokens": 2}


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m):
        yield m


def test_api_forwards_top_p_and_min_p(served):
    served.generate_tokens.return_value = [1, 2, 3]
    r = client.post("/generate/", json={**BODY, "temperature": 0.8, "top_p": 0.9, "min_p": 0.05})
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
    kw = served.generate_tokens.call_args.kwargs
    assert kw["top_p"] == 0.9 and kw["min_p"] == 0.05
    served.generate_tokens_stream.return_value = iter([4, 5])
    r = client.post("/generate/", json={**BODY, "top_p": 0.5, "stream": True})
    assert r.text == "4\n5\n"
    kw = served.generate_tokens_stream.call_args.kwargs
    assert kw["top_p"] == 0.5 and kw["min_p"] is None


@pytest.mark.parametrize("bad", [{"top_p": 0}, {"top_p": 1.5}, {"min_p": -0.1}, {"min_p": 1.0}])
def test_api_out_of_range_is_422(served, bad):
    assert client.post("/generate/", json={**BODY, **bad}).status_code == 422
    served.generate_tokens.assert_not_called()


def test_api_without_the_filters_still_succeeds(served):
    served.generate_tokens.return_value = [1, 2, 3]
    r = client.post("/generate/", json=BODY)
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
    kw = served.generate_tokens.call_args.kwargs
    assert kw["top_p"] is None and kw["min_p"] is None
    assert client.post("/generate/", json={**BODY, "top_p": 1.0, "min_p": 0.0}).status_code == 200
