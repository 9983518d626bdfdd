"""Per-token log-probabilities on the CPU: ``reference_logprobs`` against values worked by hand,
validation before any forward pass, generation through a tiny model (the three entry points and the
per-token loop), the /generate schema and stream format, and the kernels' launch plan."""
import math
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext
from penroz.ops import logprobs as lp_ops
from penroz.ops.logprobs import LogprobState, check_logprobs, reference_logprobs
from penroz.serve import app as A


# ------------------------------------------------------------------ the definition
def test_reference_against_values_worked_by_hand():
    # x = log [1, 2, 4, 1]: Σ exp(x) = 8, so the log-probabilities are log [1/8, 1/4, 1/2, 1/8]
    x = torch.tensor([[1.0, 2.0, 4.0, 1.0]]).log()
    lp, ids, top = reference_logprobs(x, torch.tensor([1]), 3)
    assert lp.dtype == torch.float32 and ids.dtype == torch.int64 and top.dtype == torch.float32
    assert lp.shape == (1,) and ids.shape == (1, 3) and top.shape == (1, 3)
    assert lp.item() == pytest.approx(math.log(0.25), abs=1e-6)
    assert ids.tolist() == [[2, 1, 0]]  # 4, then 2, then the first of the two 1s
    assert top[0].tolist() == pytest.approx([math.log(0.5), math.log(0.25), math.log(0.125)], abs=1e-6)
    # tokens [B, 1] as well; the chosen token need not be among the top n; n = 0 gives empty tops
    lp, ids, top = reference_logprobs(x, torch.tensor([[3]]), 1)
    assert lp.item() == pytest.approx(math.log(0.125), abs=1e-6) and ids.tolist() == [[2]]
    lp0, ids0, top0 = reference_logprobs(x, torch.tensor([3]), 0)
    assert lp0.item() == lp.item() and ids0.shape == (1, 0) and top0.shape == (1, 0)
    # a shift of the row changes nothing, nor does the logits' dtype beyond its rounding
    lp2, ids2, top2 = reference_logprobs(x + 100.0, torch.tensor([1]), 3)
    assert ids2.tolist() == [[2, 1, 0]] and lp2.item() == pytest.approx(math.log(0.25), abs=1e-5)


def test_equal_logits_are_ordered_by_token_id():
    V, n = 7, 5
    lp, ids, top = reference_logprobs(torch.full((2, V), 3.5), torch.tensor([6, 0]), n)
    assert ids.tolist() == [list(range(n))] * 2
    assert top.flatten().tolist() == pytest.approx([-math.log(V)] * (2 * n), abs=1e-6)
    assert lp.tolist() == pytest.approx([-math.log(V)] * 2, abs=1e-6)
    # ties below a maximum: the maximum first, then the tied ids ascending
    x = torch.tensor([[1.0, 1.0, 2.0, 1.0]], dtype=torch.bfloat16)
    assert reference_logprobs(x, torch.tensor([0]), 4)[1].tolist() == [[2, 0, 1, 3]]


def test_n_above_the_vocabulary_is_clipped():
    x = torch.randn(3, 4, generator=torch.Generator().manual_seed(0))
    lp, ids, top = reference_logprobs(x, torch.tensor([0, 1, 2]), 20)
    assert ids.shape == (3, 4) and top.shape == (3, 4)
    assert all(sorted(r) == [0, 1, 2, 3] for r in ids.tolist())
    assert torch.allclose(top.exp().sum(dim=1), torch.ones(3), atol=1e-6)


def test_check_logprobs():
    assert check_logprobs(None) is None
    assert [check_logprobs(n) for n in (0, 1, 20)] == [0, 1, 20]
    for bad in (-1, 21, 1.5, "3", True):
        with pytest.raises(ValueError):
            check_logprobs(bad)


def test_state_without_the_kernels_fills_the_column_behind_the_step_counter():
    st = LogprobState(2, 4, "cpu")
    st.set_n(3)
    x = torch.randn(2, 10, generator=torch.Generator().manual_seed(1))
    idx = torch.tensor([[3], [9]])
    lp_ops.step_logprobs(st, x, idx, torch.tensor([2]))
    lp, ids, top = reference_logprobs(x, idx, 3)
    got_lp, got_id, got_top = st.burst(2)
    assert torch.allclose(got_lp[:, 1], lp, atol=1e-6)
    assert got_id[:, 1, :3].tolist() == ids.tolist() and torch.allclose(got_top[:, 1, :3], top, atol=1e-6)
    assert (got_id[:, 1, 3:] == -1).all() and (got_top[:, 1, 3:] == -math.inf).all()
    assert lp_ops.to_lists(got_lp[:, 1:], got_id[:, 1:], got_top[:, 1:], 3)[1][0][0][0][0] == ids[0, 0].item()


# ------------------------------------------------------------------ tiny model
V_MODEL, BLOCK, NEW = 64, 8, 20
CTX = [[1, 2, 3], [4, 5, 6]]


def gpt(seed=0):
    torch.manual_seed(seed)
    return NeuralNetworkModel("gpt", Mapper(bench.gpt2_layers(V=V_MODEL, C=32, L=2, H=2, P=32),
                                            {"adamw": {"lr": 3e-3}}))


def check_info(info, tokens, n, greedy):
    assert set(info) == {"token_logprobs", "top_logprobs"}
    assert len(info["token_logprobs"]) == len(info["top_logprobs"]) == len(tokens)
    for tok, lp, top in zip(tokens, info["token_logprobs"], info["top_logprobs"]):
        assert isinstance(lp, float) and lp <= 0.0
        assert len(top) == n and all(isinstance(i, int) and isinstance(v, float) for i, v in top)
        # the definition's order: log-probability descending, ids ascending among equals
        assert all(a[1] > b[1] or (a[1] == b[1] and a[0] < b[0]) for a, b in zip(top, top[1:]))
        assert len({i for i, _ in top}) == n
        if greedy:
            assert top[0] == [tok, lp]
        hit = [v for i, v in top if i == tok]
        assert not hit or hit[0] == lp


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.0, top_k=8)], ids=["greedy", "sampled"])
def test_generate_with_logprobs_returns_the_same_tokens_and_one_entry_each(kw):
    m = gpt()
    torch.manual_seed(3)
    plain = m.generate_tokens(CTX, BLOCK, NEW, **kw)  # 3 + 20 > block_size 8: through the re-prefill
    torch.manual_seed(3)
    tokens, info = m.generate_tokens(CTX, BLOCK, NEW, logprobs=3, **kw)
    assert tokens == plain and len(tokens) == 3 + NEW
    check_info(info, tokens[3:], 3, greedy=not kw["temperature"])
    # the stream, the batch form and the per-token loop agree with it
    torch.manual_seed(3)
    streamed = list(m.generate_tokens_stream(CTX, BLOCK, NEW, logprobs=3, **kw))
    assert [s[0] for s in streamed] == tokens[3:]
    assert [s[1] for s in streamed] == info["token_logprobs"] and [s[2] for s in streamed] == info["top_logprobs"]
    torch.manual_seed(3)
    contexts, infos = m.generate_batch(CTX, BLOCK, NEW, logprobs=3, **kw)
    assert contexts[0] == tokens and infos[0] == info and len(infos) == 2
    check_info(infos[1], contexts[1][3:], 3, greedy=not kw["temperature"])
    torch.manual_seed(3)
    eager = list(m._generate_eager(CTX, BLOCK, NEW, kw["temperature"], kw.get("top_k"), None, True, logprobs=3))[-1]
    assert eager == (tokens, info)
    # n = 0: the chosen tokens' log-probabilities alone, the same numbers
    torch.manual_seed(3)
    t0, i0 = m.generate_tokens(CTX, BLOCK, NEW, logprobs=0, **kw)
    assert t0 == tokens and i0["token_logprobs"] == info["token_logprobs"] and i0["top_logprobs"] == [[]] * NEW


def test_logprobs_are_those_of_the_logits_the_sampler_saw():
    m = gpt()
    tokens, info = m.generate_tokens([[1, 2, 3]], BLOCK, 2, temperature=0.0, logprobs=20)
    acts, _ = m(torch.tensor([[1, 2, 3]]), skip_softmax=True)
    lp, ids, top = reference_logprobs(acts[-1][:, -1, :], torch.tensor([tokens[3]]), 20)
    # (the prefill attends through the KV cache, this forward does not: the logits agree to rounding)
    assert info["token_logprobs"][0] == pytest.approx(lp.item(), abs=1e-5)
    assert [i for i, _ in info["top_logprobs"][0]] == ids[0].tolist()
    assert [v for _, v in info["top_logprobs"][0]] == pytest.approx(top[0].tolist(), abs=1e-5)
    # a repetition penalty changes the distribution the log-probabilities describe
    _, pen = m.generate_tokens([[1, 2, 3]], BLOCK, 2, temperature=0.0, logprobs=20, repetition_penalty=1.5)
    assert pen["top_logprobs"][0] != info["top_logprobs"][0]


def test_stop_token_is_included_and_the_batch_infos_end_with_the_contexts():
    m = gpt()
    plain = m.generate_tokens(CTX, BLOCK, NEW, temperature=0.0)
    stop = plain[3 + 4]  # a token the greedy run does produce
    tokens, info = m.generate_tokens(CTX, BLOCK, NEW, temperature=0.0, stop_token=stop, logprobs=2)
    assert tokens == m.generate_tokens(CTX, BLOCK, NEW, temperature=0.0, stop_token=stop)
    assert tokens[-1] == stop and len(info["token_logprobs"]) == len(tokens) - 3
    assert info["top_logprobs"][-1][0][0] == stop
    contexts, infos = m.generate_batch(CTX, BLOCK, NEW, temperature=0.0, stop_token=stop, logprobs=2)
    assert contexts == m.generate_batch(CTX, BLOCK, NEW, temperature=0.0, stop_token=stop)
    for ctx, inf in zip(contexts, infos):
        assert len(inf["token_logprobs"]) == len(inf["top_logprobs"]) == len(ctx) - 3


@pytest.mark.parametrize("bad", [-1, 21, 1.5])
def test_bad_values_fail_before_any_forward(monkeypatch, bad):
    m = gpt()

    def no_forward(*a, **k):
        raise AssertionError("forward ran before validation")

    monkeypatch.setattr(NeuralNetworkModel, "forward", no_forward)
    with pytest.raises(ValueError):
        m.generate_tokens([[1, 2]], 8, 2, temperature=0.0, logprobs=bad)
    with pytest.raises(ValueError):
        list(m.generate_tokens_stream([[1, 2]], 8, 2, temperature=0.0, logprobs=bad))
    with pytest.raises(ValueError):
        m.generate_batch([[1, 2]], 8, 2, temperature=0.0, logprobs=bad)


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1]], "block_size": 8, "max_new_tokens": 2}
INFO = {"token_logprobs": [-0.5, -1.25], "top_logprobs": [[[2, -0.5], [7, -2.0]], [[9, -0.125], [3, -1.25]]]}


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m):
        yield m


def test_api_forwards_logprobs_and_returns_them_only_when_asked(served):
    served.generate_tokens.return_value = ([1, 2, 3], INFO)
    r = client.post("/generate/", json={**BODY, "logprobs": 2})
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3], "logprobs": INFO}
    assert served.generate_tokens.call_args.kwargs["logprobs"] == 2
    served.generate_tokens.return_value = [1, 2, 3]
    r = client.post("/generate/", json=BODY)
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
    assert served.generate_tokens.call_args.kwargs.get("logprobs") is None
    served.generate_tokens.return_value = ([1, 2, 3], {"token_logprobs": [-0.5, -1.25], "top_logprobs": [[], []]})
    r = client.post("/generate/", json={**BODY, "logprobs": 0})
    assert r.json()["logprobs"]["top_logprobs"] == [[], []]
    assert served.generate_tokens.call_args.kwargs["logprobs"] == 0


def test_api_stream_lines(served):
    served.generate_tokens_stream.return_value = iter([(4, -0.1, [[4, -0.1], [11, -2.5]]), (5, -3.0, [[6, -0.25], [4, -1.5]])])
    r = client.post("/generate/", json={**BODY, "logprobs": 2, "stream": True})
    assert r.status_code == 200
    assert r.text == "4\t-0.1\t4:-0.1\t11:-2.5\n5\t-3.0\t6:-0.25\t4:-1.5\n"
    assert served.generate_tokens_stream.call_args.kwargs["logprobs"] == 2
    tok, lp, *top = r.text.splitlines()[0].split("\t")  # floats written by repr read back exactly
    assert (int(tok), float(lp)) == (4, -0.1) and [float(t.split(":")[1]) for t in top] == [-0.1, -2.5]
    served.generate_tokens_stream.return_value = iter([(4, -0.1, [])])
    assert client.post("/generate/", json={**BODY, "logprobs": 0, "stream": True}).text == "4\t-0.1\n"
    served.generate_tokens_stream.return_value = iter([4, 5])
    assert client.post("/generate/", json={**BODY, "stream": True}).text == "4\n5\n"
    assert served.generate_tokens_stream.call_args.kwargs.get("logprobs") is None


@pytest.mark.parametrize("bad", [21, -1])
def test_api_bad_logprobs_is_422(served, bad):
    assert client.post("/generate/", json={**BODY, "logprobs": bad}).status_code == 422
    assert client.post("/generate/", json={**BODY, "logprobs": bad, "stream": True}).status_code == 422
    served.generate_tokens.assert_not_called()
    served.generate_tokens_stream.assert_not_called()


# ------------------------------------------------------------------ the kernels' launch plan
@pytest.mark.skipif(not _ext.available(), reason="needs the built extension")
def test_launch_plan():
    plan = _ext.kernels().token_logprobs_plan
    per_part = 2 + 2 * lp_ops.MAX_LOGPROBS  # m, s and 20 candidates of 64 bits, in floats
    for V, parts in ((1, 1), (4096, 1), (4097, 2), (50257, 13), (262144, 64), (1 << 20, 256)):
        assert plan(V) == (parts, parts * per_part)
    for V in ((1 << 20) + 1, 0):
        with pytest.raises(RuntimeError):
            plan(V)
