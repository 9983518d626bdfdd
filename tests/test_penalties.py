"""Repetition, presence and frequency penalties on the CPU: ``reference_penalise`` against a
per-element loop written here from the definition, ``PenaltyState``'s bookkeeping, validation
before any forward pass, generation through a tiny model, and the /generate schema."""
import math
import struct
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.penalties import PenaltyState, check_penalties, reference_penalise
from penroz.serve import app as A


def f32(v: float) -> float:
    """v rounded to fp32 (the loop below rounds after every operation, as fp32 arithmetic does)."""
    return struct.unpack("f", struct.pack("f", v))[0]


def by_hand(logits, in_prompt, count, r, p, f):
    """The definition, element by element: fp32 after every operation (a product or a quotient of two
    fp32 numbers is exact in fp64, so rounding it to fp32 is the correctly rounded fp32 result; so is
    a sum or a difference)."""
    r, p, f = f32(r), f32(p), f32(f)
    out = []
    for xs, ps, cs in zip(logits, in_prompt, count):
        row = []
        for x, ip, c in zip(xs, ps, cs):
            y = f32(x)
            if ip or c > 0:
                y = f32(y / r) if y > 0 else f32(y * r)
            if c > 0:
                y = f32(y - f32(p + f32(f * float(c))))
            row.append(y)
        out.append(row)
    return out


LOGITS = [[2.5, -1.25, 0.0, 0.75, -3.0, 1.0, 0.0, -0.5, 4.0, -0.1, 0.3, 7.5, -6.0, 0.0, 1.1, -2.2],
          [-0.7, 3.3, 0.0, -4.5, 0.9, 0.0, 2.2, -1.0, 0.05, -0.05, 5.0, -5.0, 1.7, 0.0, -0.3, 0.6]]
# per row: tokens of the prompt, and how often each token was generated — prompt only (ids 0-3),
# generated only (4-7: zero, positive and negative logits among them), both (8-11), neither (12-15)
IN_PROMPT = [[i < 4 or 8 <= i < 12 for i in range(16)]] * 2
COUNT = [[0, 0, 0, 0, 1, 2, 3, 1, 1, 4, 2, 1, 0, 0, 0, 0],
         [0, 0, 0, 0, 2, 1, 1, 5, 3, 1, 1, 2, 0, 0, 0, 0]]


@pytest.mark.parametrize("r,p,f", [(1.3, 0.0, 0.0), (0.8, 0.0, 0.0), (1.0, 0.37, 0.0), (1.0, 0.0, 0.11),
                                   (1.0, -0.4, 0.0), (1.3, 0.37, 0.11), (2.0, 0.5, 0.25)])
def test_reference_matches_the_definition_element_by_element(r, p, f):
    x = torch.tensor(LOGITS, dtype=torch.float32)
    got = reference_penalise(x, torch.tensor(IN_PROMPT), torch.tensor(COUNT), r, p, f)
    assert got.dtype == torch.float32
    want = torch.tensor(by_hand(LOGITS, IN_PROMPT, COUNT, r, p, f), dtype=torch.float32)
    assert torch.equal(got, want)
    # rounded once to a 16-bit logits dtype, from the fp32 result
    xb = x.to(torch.bfloat16)
    want_b = torch.tensor(by_hand(xb.float().tolist(), IN_PROMPT, COUNT, r, p, f)).to(torch.bfloat16)
    got_b = reference_penalise(xb, torch.tensor(IN_PROMPT), torch.tensor(COUNT), r, p, f)
    assert got_b.dtype == torch.bfloat16 and torch.equal(got_b, want_b)


def test_prompt_tokens_get_repetition_only_and_generated_tokens_get_all_three():
    x = torch.tensor(LOGITS, dtype=torch.float32)
    ip, cnt = torch.tensor(IN_PROMPT), torch.tensor(COUNT)
    y = reference_penalise(x, ip, cnt, 2.0, 0.5, 0.25)
    for b in range(2):
        for v in range(16):
            xv, c = f32(LOGITS[b][v]), COUNT[b][v]
            rep = xv / 2.0 if xv > 0 else xv * 2.0  # (exact: a power of two)
            if v < 4:      # prompt only: repetition, no presence / frequency
                assert y[b, v].item() == rep
            elif v < 12:   # generated (8-11: in the prompt too — repetition still once)
                assert y[b, v].item() == f32(rep - (0.5 + 0.25 * c))
            else:          # never seen: untouched
                assert y[b, v].item() == f32(xv)
    # presence / frequency alone leave prompt-only tokens untouched
    y = reference_penalise(x, ip, cnt, 1.0, 0.5, 0.25)
    assert torch.equal(y[:, :4], x[:, :4]) and torch.equal(y[:, 12:], x[:, 12:])
    assert not torch.equal(y[:, 4:12], x[:, 4:12])


def test_check_penalties_folds_neutral_values_and_refuses_bad_ones():
    assert check_penalties(None, None, None) is None
    assert check_penalties(1.0, 0.0, 0.0) is None
    assert check_penalties(1, 0, None) is None
    assert check_penalties(1.2, None, None) == (1.2, 0.0, 0.0)
    assert check_penalties(None, -0.5, 2) == (1.0, -0.5, 2.0)
    for bad in ((0, 0, 0), (-1.0, 0, 0), (math.inf, 0, 0), (math.nan, 0, 0), (1.0, math.nan, 0),
                (1.0, 0, math.nan), (1.0, math.inf, 0), (1.0, 0, -math.inf)):
        with pytest.raises(ValueError):
            check_penalties(*bad)


# ------------------------------------------------------------------ PenaltyState on the CPU
def test_state_follows_dense_bookkeeping_done_by_hand():
    V, r, p, f = 16, 1.3, 0.37, 0.11
    prompt = torch.tensor([[3, 3, 5, 9], [0, 15, 15, 1]])
    st = PenaltyState()
    st.set_params(r, p, f)
    st.begin(prompt)
    in_prompt = [[v in row for v in range(V)] for row in prompt.tolist()]
    count = [[0] * V for _ in range(2)]
    gen = torch.Generator().manual_seed(0)
    steps = [None, [5, 2], [5, 2], [7, 15], [5, 0]]  # repeats, prompt tokens and fresh ones
    for new in steps:
        x = torch.randn(2, V, generator=gen) * 3
        if new is not None:
            for b, t in enumerate(new):
                count[b][t] += 1
        y = st.apply(x.clone(), None if new is None else torch.tensor(new).view(2, 1))
        assert torch.equal(y, torch.tensor(by_hand(x.tolist(), in_prompt, count, r, p, f)))
        ip, oc = st.dense()
        assert ip.tolist() == in_prompt and oc.tolist() == count
    assert oc[0, 5].item() == 3 and oc[1, 2].item() == 2

    # a second call forgets the first
    prompt2 = torch.tensor([[8], [8]])
    st.begin(prompt2)
    x = torch.randn(2, V, generator=gen)
    y = st.apply(x.clone(), None)
    ip, oc = st.dense()
    assert ip.tolist() == [[v == 8 for v in range(V)]] * 2 and int(oc.sum()) == 0
    assert torch.equal(y, torch.tensor(by_hand(x.tolist(), ip.tolist(), oc.tolist(), r, p, f)))


def test_state_refuses_prompt_ids_outside_the_vocabulary():
    for bad in ([[1, 16]], [[-1, 2]]):
        st = PenaltyState()
        st.set_params(1.3, 0.0, 0.0)
        st.begin(torch.tensor(bad))
        with pytest.raises(ValueError):
            st.apply(torch.zeros(1, 16), None)


# ------------------------------------------------------------------ tiny model
V_MODEL = 64


def gpt(seed=0):
    torch.manual_seed(seed)
    return NeuralNetworkModel("gpt", Mapper(bench.gpt2_layers(V=V_MODEL, C=32, L=2, H=2, P=32),
                                            {"adamw": {"lr": 3e-3}}))


@pytest.mark.parametrize("bad", [{"repetition_penalty": 0}, {"repetition_penalty": -1.5},
                                 {"repetition_penalty": math.inf}, {"repetition_penalty": math.nan},
                                 {"presence_penalty": math.nan}, {"frequency_penalty": math.nan}])
def test_bad_values_fail_before_any_forward(monkeypatch, bad):
    m = gpt()

    def no_forward(*a, **k):
        raise AssertionError("forward ran before validation")

    monkeypatch.setattr(NeuralNetworkModel, "forward", no_forward)
    with pytest.raises(ValueError):
        m.generate_tokens([[1, 2]], 8, 2, temperature=0.0, **bad)
    with pytest.raises(ValueError):
        list(m.generate_tokens_stream([[1, 2]], 8, 2, temperature=0.0, **bad))
    with pytest.raises(ValueError):
        m.generate_batch([[1, 2]], 8, 2, temperature=0.0, **bad)


CTX = [[1, 2, 3], [4, 5, 6]]


def test_a_huge_frequency_penalty_makes_greedy_tokens_distinct_across_the_window():
    m = gpt()
    plain = m.generate_batch(CTX, 8, 20, temperature=0.0)
    # the property below is vacuous unless the unpenalised model does repeat itself (seed 0 does)
    assert all(len(set(row[3:])) < 20 for row in plain)
    pen = m.generate_batch(CTX, 8, 20, temperature=0.0, frequency_penalty=1e4)
    assert all(len(row) == 23 for row in pen)  # 3 + 20 > block_size 8: through the window-full re-prefill
    for row in pen:
        assert len(set(row[3:])) == 20, row
    # the three entry points agree (generate_tokens and the stream return row 0)
    assert m.generate_tokens(CTX, 8, 20, temperature=0.0, frequency_penalty=1e4) == pen[0]
    assert list(m.generate_tokens_stream(CTX, 8, 20, temperature=0.0, frequency_penalty=1e4)) == pen[0][3:]
    # and so does the per-token loop
    eager = list(m._generate_eager(CTX, 8, 20, 0.0, None, None, True, frequency_penalty=1e4))[-1]
    assert eager == pen[0]
    # the same call again: the state is per call
    assert m.generate_batch(CTX, 8, 20, temperature=0.0, frequency_penalty=1e4) == pen


def test_the_whole_prompt_counts_for_repetition_and_not_for_presence():
    """The first generated token: nothing is generated yet, so presence / frequency cannot move it,
    whatever the prompt holds; repetition sees every prompt token, those beyond block_size included."""
    m = gpt()
    prompt = [list(range(V_MODEL - 1))]  # every token but the last, far longer than the window of 8
    plain = m.generate_tokens(prompt, 8, 1, temperature=0.0)[-1]
    assert m.generate_tokens(prompt, 8, 1, temperature=0.0, presence_penalty=1e4, frequency_penalty=1e4)[-1] == plain
    # r = 1e4 pushes every prompt token's logit towards -inf or to ~0; token V-1 alone keeps its logit.
    # Its logit is what the model gives it, so compare with the penalised row computed by hand
    acts, _ = m(torch.tensor(prompt)[:, -8:], skip_softmax=True)
    row = acts[-1][:, -1, :]
    in_prompt = torch.ones(1, V_MODEL, dtype=torch.bool)
    in_prompt[0, -1] = False
    want = int(reference_penalise(row, in_prompt, torch.zeros(1, V_MODEL, dtype=torch.long), 1e4, 0.0, 0.0).argmax())
    assert m.generate_tokens(prompt, 8, 1, temperature=0.0, repetition_penalty=1e4)[-1] == want
    in_window = torch.zeros(1, V_MODEL, dtype=torch.bool)
    in_window[0, prompt[0][-8:]] = True
    short = reference_penalise(row, in_window, torch.zeros(1, V_MODEL, dtype=torch.long), 1e4, 0.0, 0.0)
    assert not torch.equal(short, reference_penalise(row, in_prompt, torch.zeros(1, V_MODEL, dtype=torch.long),
                                                     1e4, 0.0, 0.0))


def test_neutral_values_are_the_call_without_them():
    m = gpt()
    for kw in (dict(temperature=0.0), dict(temperature=1.0, top_k=5)):
        torch.manual_seed(3)
        plain = m.generate_batch(CTX, 8, 20, **kw)
        torch.manual_seed(3)
        assert m.generate_batch(CTX, 8, 20, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                                **kw) == plain
        torch.manual_seed(3)
        assert m.generate_batch(CTX, 8, 20, repetition_penalty=None, presence_penalty=None, **kw) == plain


def test_neutral_values_never_touch_the_penalty_code(monkeypatch):
    m = gpt()

    def no_state(*a, **k):
        raise AssertionError("a penalty state was made for neutral values")

    monkeypatch.setattr(PenaltyState, "__init__", no_state)
    m.generate_tokens(CTX, 8, 4, temperature=0.0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    m.generate_tokens(CTX, 8, 4, temperature=0.0)


def test_seeded_stream_equals_non_stream_with_penalties():
    m = gpt()
    kw = dict(temperature=1.0, top_k=8, repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
    torch.manual_seed(5)
    a = m.generate_tokens([[1, 2]], 8, 14, **kw)
    torch.manual_seed(5)
    b = [1, 2] + list(m.generate_tokens_stream([[1, 2]], 8, 14, **kw))
    assert a == b
    torch.manual_seed(5)
    assert m.generate_tokens([[1, 2]], 8, 14, temperature=1.0, top_k=8) != a  # (the penalties did act)


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1]], "block_size": 8, "max_new_tokens": 2}
NAMES = ("repetition_penalty", "presence_penalty", "frequency_penalty")


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m):
        yield m


def test_api_forwards_the_three_penalties_as_keywords(served):
    served.generate_tokens.return_value = [1, 2, 3]
    r = client.post("/generate/", json={**BODY, "repetition_penalty": 1.2, "presence_penalty": 0.5,
                                        "frequency_penalty": -0.25})
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
    kw = served.generate_tokens.call_args.kwargs
    assert [kw[n] for n in NAMES] == [1.2, 0.5, -0.25]
    served.generate_tokens_stream.return_value = iter([4, 5])
    r = client.post("/generate/", json={**BODY, "presence_penalty": 0.7, "stream": True})
    assert r.text == "4\n5\n"
    kw = served.generate_tokens_stream.call_args.kwargs
    assert [kw[n] for n in NAMES] == [None, 0.7, None]


def test_api_absent_penalties_arrive_as_none(served):
    served.generate_tokens.return_value = [1, 2, 3]
    assert client.post("/generate/", json=BODY).status_code == 200
    kw = served.generate_tokens.call_args.kwargs
    assert [kw[n] for n in NAMES] == [None, None, None]
    assert client.post("/generate/", json={**BODY, "repetition_penalty": 1.0, "presence_penalty": 0.0,
                                           "frequency_penalty": 0.0}).status_code == 200


@pytest.mark.parametrize("bad", [{"repetition_penalty": 0}, {"repetition_penalty": -2.0}])
def test_api_bad_repetition_penalty_is_422(served, bad):
    assert client.post("/generate/", json={**BODY, **bad}).status_code == 422
    assert client.post("/generate/", json={**BODY, **bad, "stream": True}).status_code == 422
    served.generate_tokens.assert_not_called()
    served.generate_tokens_stream.assert_not_called()


@pytest.mark.parametrize("name", NAMES)
def test_api_non_finite_penalty_is_422(served, name):
    # JSON has no literal for them; Python's encoder writes NaN / Infinity, which the schema refuses
    for bad in ("NaN", "Infinity"):
        body = ('{"model_id": "t", "input": [[1]], "block_size": 8, "max_new_tokens": 2, "%s": %s}' % (name, bad))
        r = client.post("/generate/", content=body, headers={"content-type": "application/json"})
        assert r.status_code == 422
    served.generate_tokens.assert_not_called()
