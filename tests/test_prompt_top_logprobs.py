"""``prompt_top_logprobs`` on the CPU: the chunked torch path against ``reference_top_n``, ``to_dicts``, the refusals."""
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.prompt_logprobs import reference_top_n, score_rows, to_dicts
from penroz.serve import app as A


@pytest.mark.parametrize("n", [1, 5, 20])
@pytest.mark.parametrize("V", [17, 301])
def test_torch_path_matches_the_reference(monkeypatch, n, V):
    """Small integers: every logit is exact in fp32 and ties abound, so ids and order are the reference's exactly."""
    g = torch.Generator().manual_seed(n + V)
    h, W = (torch.randint(-2, 3, (s, 48), generator=g).float() for s in (37, V))
    b = torch.where(torch.arange(V) % 2 == 0, 5.0, torch.randint(-3, 4, (V,), generator=g).float())
    h[5] = 0  # every even id an equal maximum: more than n of them, the cut falls inside the tie
    t = torch.randint(0, V, (37,), generator=g)
    monkeypatch.setattr("penroz.ops.prompt_logprobs.CHUNK_ELEMS", V * 8)  # five chunks of rows
    lp, top, top_lp, ids, lps = score_rows(h, W, b, t, top_n=n)
    r_ids, r_lps = reference_top_n(h, W, b, n)
    k = min(n, V)  # (fp32 logsumexp over |x| < 300: within 1e-4)
    assert ids.dtype == torch.int64 and lps.dtype == torch.float32 and torch.equal(ids, r_ids)
    assert ids[5, :min(n, 9)].tolist() == list(range(0, 18, 2))[:n] and (lps[:, :k].double() - r_lps[:, :k]).abs().max() < 1e-4
    assert (ids[:, k:] == -1).all() and (lps[:, k:] == float("-inf")).all()
    assert torch.equal(ids[:, 0], top) and torch.equal(lps[:, 0], top_lp)
    assert all(torch.equal(a, c) for a, c in zip(score_rows(h, W, b, t), (lp, top, top_lp)))  # without n: as before


def test_to_dicts_with_and_without_n():
    three = torch.tensor([-1.0, -2.0, -3.0]), torch.tensor([4, 5, 6]), torch.tensor([-0.5, -0.25, -0.125])
    ids, lps = torch.tensor([[4, 1], [5, 2], [6, -1]]), torch.tensor([[-0.5, -1.5], [-0.25, -2.5], [-0.125, float("-inf")]])
    plain, with_n = to_dicts([3, 2], *three), to_dicts([3, 2], *three, ids, lps)
    assert plain == [{"token_logprobs": [None, -1.0, -2.0], "top_tokens": [None, 4, 5], "top_logprobs": [None, -0.5, -0.25]},
                     {"token_logprobs": [None, -3.0], "top_tokens": [None, 6], "top_logprobs": [None, -0.125]}]
    assert [{**d, "top_n": t} for d, t in zip(plain, [[None, [[4, -0.5], [1, -1.5]], [[5, -0.25], [2, -2.5]]], [None, [[6, -0.125]]]])] == with_n


@pytest.mark.parametrize("options, text, status", [
    ({"prompt_top_logprobs": 3}, "needs prompt_logprobs", 400),
    ({"prompt_logprobs": True, "prompt_top_logprobs": 21}, "in \\[0, 20\\]", 422),
    ({"prompt_logprobs": True, "prompt_top_logprobs": -1}, "in \\[0, 20\\]", 422),
    ({"prompt_logprobs": True, "prompt_top_logprobs": True}, "in \\[0, 20\\]", 422),
    ({"prompt_logprobs": True, "prompt_top_logprobs": 3, "speculate": 1}, "speculate", 400),
    ({"prompt_logprobs": True, "prompt_top_logprobs": 3, "stream": True}, "stream", 400)])
def test_refused_before_any_forward_and_before_the_model_is_loaded(monkeypatch, options, text, status):
    torch.manual_seed(0)
    m = NeuralNetworkModel("gpt", Mapper(bench.gpt2_layers(V=64, C=32, L=1, H=2, P=32), {"adamw": {"lr": 3e-3}}))
    monkeypatch.setattr(torch.nn.Embedding, "forward", MagicMock(side_effect=AssertionError("a layer ran before validation")))
    kw = {k: v for k, v in options.items() if k != "stream"}
    for method in [m.generate_tokens_stream] if "stream" in options else [m.generate_tokens, m.generate_batch]:
        with pytest.raises(ValueError, match=text):
            list(method([[1, 2]], 8, 2, temperature=0.0, **kw))
    with patch.object(A, "load_for_serving") as load:
        body = {"model_id": "t", "input": [[1, 2]], "block_size": 8, "max_new_tokens": 2, "temperature": 0.0, **options}
        assert TestClient(main.app, raise_server_exceptions=False).post("/generate/", json=body).status_code == status
        load.assert_not_called()

