"""Logit bias, banned and allowed tokens and ``min_tokens`` on the CPU: ``check_logit_bias``' limits and
canonical form, ``reference_bias`` at V = 8 written out by hand, generation through a tiny model, and the
/generate schema."""
import math
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.logit_bias import MAX_ENTRIES, BiasState, Canonical, check_logit_bias, floor_of, reference_bias
from penroz.serve import app as A

INF = math.inf
FLOOR = -(2.0 ** 100)


def check(logit_bias=None, banned=None, allowed=None, min_tokens=None, ends=(), V=256, max_new=40, **kw):
    return check_logit_bias(logit_bias, banned, allowed, min_tokens, ends, V, max_new, **kw)


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("kw", [
    {}, dict(logit_bias={}, banned=[], min_tokens=0), dict(logit_bias={3: 0.0}),
    dict(min_tokens=5),                 # no end token: nothing to suppress
    dict(min_tokens=0, ends=[7]),
], ids=["none", "empty", "zero_bias", "min_tokens_without_end", "ends_without_min_tokens"])
def test_neutral_forms_give_none(kw):
    assert check(**kw) is None


@pytest.mark.parametrize("kw", [
    dict(logit_bias={1: 100.5}), dict(logit_bias={1: -100.5}),
    dict(logit_bias={1: INF}), dict(logit_bias={1: math.nan}),
    dict(logit_bias={1: "2"}), dict(logit_bias={1: True}), dict(logit_bias=[1, 2]),
    dict(logit_bias={"x": 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={True: 1.0}),
    dict(logit_bias={-1: 1.0}), dict(logit_bias={256: 1.0}), dict(logit_bias={"7": 1.0, 7: 2.0}),
    dict(banned=[256]), dict(banned=[-1]), dict(banned=[1.0]), dict(banned=[True]), dict(banned=3), dict(banned="12"),
    dict(allowed=[]), dict(allowed=[256]), dict(allowed=[False]), dict(allowed="1"),
    dict(min_tokens=-1), dict(min_tokens=1.0), dict(min_tokens=True),
], ids=["bias>100", "bias<-100", "bias_inf", "bias_nan", "bias_str", "bias_bool", "bias_list", "key_word", "key_float",
        "key_bool", "key_negative", "key_beyondV", "key_twice", "ban_beyondV", "ban_negative", "ban_float", "ban_bool",
        "ban_int", "ban_str", "allowed_empty", "allowed_beyondV", "allowed_bool", "allowed_str", "min_negative",
        "min_float", "min_bool"])
def test_check_refuses(kw):
    with pytest.raises(ValueError):
        check(**kw)


def test_bias_bounds_are_inclusive():
    assert check(logit_bias={1: 100, 2: -100.0}).entries == [(1, 100.0, 0), (2, -100.0, 0)]


def test_entry_cap():
    assert len(check(banned=list(range(MAX_ENTRIES)), V=4096).ids) == MAX_ENTRIES
    with pytest.raises(ValueError):
        check(banned=list(range(MAX_ENTRIES + 1)), V=4096)
    # bias, banned ids and end tokens count together
    with pytest.raises(ValueError):
        check(logit_bias={i: 1.0 for i in range(1000)}, banned=list(range(1000, 1024)), min_tokens=1, ends=[2000], V=4096)
    # entries outside the allowed set are dropped before they are counted
    assert len(check(banned=list(range(2000)), allowed=[0, 1, 3000], V=4096).ids) == 2


def test_temperature_floor():
    for t in (1e-7, -1e-7, 9.9e-7):
        with pytest.raises(ValueError):
            check(banned=[1], temperature=t)
    for t in (0, 0.0, 1e-6, 1.0, None):
        assert check(banned=[1], temperature=t) is not None
    assert check(temperature=1e-7) is None  # nothing active: not this check's to refuse


def test_min_tokens_is_at_most_max_new_tokens():
    assert check(min_tokens=40, ends=[3], max_new=40).until == (40,)
    with pytest.raises(ValueError):
        check(min_tokens=41, ends=[3], max_new=40)
    with pytest.raises(ValueError):
        check(min_tokens=41, max_new=40)  # with nothing to suppress as well


def test_nothing_left_unmasked_is_refused():
    with pytest.raises(ValueError):
        check(allowed=[1, 2], banned=[2, 1])
    with pytest.raises(ValueError):
        check(allowed=[1, 2], banned=[2], min_tokens=1, ends=[1])
    assert check(allowed=[1, 2], banned=[2], min_tokens=0, ends=[1]) is not None
    with pytest.raises(ValueError):
        check(banned=list(range(8)), V=8)
    with pytest.raises(ValueError):
        check(banned=list(range(7)), min_tokens=2, ends=[7], V=8)
    assert check(banned=list(range(7)), V=8) is not None


def test_string_keys_are_accepted():
    assert check(logit_bias={"7": 1.5, " 12 ": -2, "+3": 1}).entries == [(3, 1.0, 0), (7, 1.5, 0), (12, -2.0, 0)]


def test_canonical_form():
    c = check(logit_bias={9: 2.0, 4: -1.0, 200: 3.0, 6: 0.0}, banned=[200, 5, 5], min_tokens=3, ends=[9, 11, 999, 5])
    # sorted, unique; the banned id wins over its bias; end tokens carry until and their bias, or 0; an end
    # token that is banned stays banned; one outside the vocabulary is left aside; a zero bias is no entry
    assert c.entries == [(4, -1.0, 0), (5, -INF, 0), (9, 2.0, 3), (11, 0.0, 3), (200, -INF, 0)]
    assert c.allowed is None and c.V == 256
    assert list(c.ids) == sorted(set(c.ids))
    # entries outside the allowed set are dropped: the mask writes those ids
    c = check(logit_bias={9: 2.0, 4: -1.0}, banned=[5, 6], allowed=[9, 5, 7, 7], min_tokens=3, ends=[11, 7])
    assert c.entries == [(5, -INF, 0), (7, 0.0, 3), (9, 2.0, 0)] and c.allowed == (5, 7, 9)
    # an allowed set alone is on, with no entries
    c = check(allowed=[0, 31, 32, 255])
    assert c.entries == [] and c.mask_words().tolist() == [1 - 2 ** 31, 1, 0, 0, 0, 0, 0, -2 ** 31]
    assert check(allowed=[0, 32], V=33).mask_words().tolist() == [1, 1]


def test_ids_are_checked_against_2_31_while_the_vocabulary_is_unknown():
    c = check(banned=[2 ** 31 - 1], allowed=[5, 2 ** 31 - 1], V=None)
    assert c.V is None and c.allowed == (5, 2 ** 31 - 1)
    with pytest.raises(ValueError):
        check(banned=[2 ** 31], V=None)


# ------------------------------------------------------------------ the definition, V = 8
X = torch.tensor([[0.5, -1.0, 2.0, 3.0, -0.25, 0.0, 1.5, -2.0],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])


def test_reference_a_bias():
    c = check(logit_bias={2: 1.25, 7: -0.5}, V=8)
    assert reference_bias(X, c, 0).tolist() == [[0.5, -1.0, 3.25, 3.0, -0.25, 0.0, 1.5, -2.5],
                                                [1.0, 1.0, 2.25, 1.0, 1.0, 1.0, 1.0, 0.5]]
    assert reference_bias(X, None, 0).tolist() == X.tolist()


def test_reference_a_banned_id():
    c = check(logit_bias={3: 5.0}, banned=[3, 0], V=8)
    assert reference_bias(X, c, 4).tolist() == [[FLOOR, -1.0, 2.0, FLOOR, -0.25, 0.0, 1.5, -2.0],
                                                [FLOOR, 1.0, 1.0, FLOOR, 1.0, 1.0, 1.0, 1.0]]


def test_reference_an_allowed_set():
    c = check(logit_bias={1: 1.0, 6: 2.0}, banned=[4], allowed=[6, 4, 2], V=8)
    assert reference_bias(X, c, 0).tolist() == [[FLOOR, FLOOR, 2.0, FLOOR, FLOOR, FLOOR, 3.5, FLOOR],
                                                [FLOOR, FLOOR, 1.0, FLOOR, FLOOR, FLOOR, 3.0, FLOOR]]


def test_reference_min_tokens_lifts_at_t_equal_to_min_tokens():
    c = check(logit_bias={5: 0.75}, min_tokens=3, ends=[5, 1], V=8)
    held = [[0.5, FLOOR, 2.0, 3.0, -0.25, FLOOR, 1.5, -2.0], [1.0, FLOOR, 1.0, 1.0, 1.0, FLOOR, 1.0, 1.0]]
    free = [[0.5, -1.0, 2.0, 3.0, -0.25, 0.75, 1.5, -2.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.75, 1.0, 1.0]]
    assert reference_bias(X, c, 0).tolist() == held and reference_bias(X, c, 2).tolist() == held
    assert reference_bias(X, c, 3).tolist() == free and reference_bias(X, c, 30).tolist() == free


def test_reference_rounds_once_to_the_dtype_and_floor_is_exact():
    c = check(logit_bias={0: 0.3}, banned=[1], V=8)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        x = X.to(dtype)
        y = reference_bias(x, c, 0)
        assert y.dtype == dtype and y[0, 0] == (x[0, 0].float() + torch.tensor(0.3)).to(dtype)
        assert float(y[0, 1]) == floor_of(dtype) and math.isfinite(floor_of(dtype))
        assert torch.equal(x, X.to(dtype))  # the input is left as it is
    assert floor_of(torch.float16) == -32768.0 and floor_of(torch.bfloat16) == FLOOR == floor_of(torch.float32)


def test_state_on_the_cpu_runs_the_reference():
    st = BiasState("cpu")
    assert st.form == "off" and st.apply(X, 0) is X
    c = check(logit_bias={5: 0.75}, min_tokens=3, ends=[5], V=8)
    st.set(c)
    assert st.form == "entries" and st.n_entries.tolist() == [2 - 1]
    assert torch.equal(st.apply(X, 2), reference_bias(X, c, 2)) and st.base_t.tolist() == [2]
    assert torch.equal(st.step(X, torch.tensor([1])), reference_bias(X, c, 3))  # t = base_t + step_t
    c = check(allowed=[1, 2], V=8)
    st.set(c)
    assert st.form == "mask" and st.allow.tolist() == [6]
    assert torch.equal(st.apply(X, 0), reference_bias(X, c, 0))
    with pytest.raises(ValueError):
        st.apply(torch.zeros(1, 9), 0)  # another vocabulary than the one checked against
    st.set(None)
    assert st.form == "off" and st.step(X, torch.tensor([0])) is X


# ------------------------------------------------------------------ through a tiny model
V_MODEL, BLOCK, NEW = 256, 16, 40
CTX = [[1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12], [13, 14, 15, 16, 17, 18]]
P = 6


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    m = NeuralNetworkModel("bias", Mapper(bench.gpt2_layers(V=V_MODEL, C=128, L=2, H=2, P=64), {"adamw": {"lr": 3e-3}}))
    greedy = m.generate_batch(CTX, BLOCK, NEW, temperature=0.0)
    return m, greedy


def test_a_bias_of_100_wins_every_step(tiny):
    m, _ = tiny
    rows = m.generate_batch(CTX, BLOCK, NEW, temperature=0.0, logit_bias={7: 100})
    assert [r[P:] for r in rows] == [[7] * NEW] * 3
    assert m.generate_tokens(CTX[:1], BLOCK, NEW, temperature=0.0, logit_bias={"7": 100.0})[P:] == [7] * NEW


def test_allowed_set_holds_for_every_row_and_token(tiny):
    m, _ = tiny
    allowed = [3, 77, 250]
    torch.manual_seed(5)
    rows = m.generate_batch(CTX, BLOCK, NEW, temperature=1.0, top_k=50, allowed_token_ids=allowed)
    assert all(len(r) == P + NEW and set(r[P:]) <= set(allowed) for r in rows)
    assert len({t for r in rows for t in r[P:]}) > 1  # (it does sample among them)


def test_banned_first_token_changes_it(tiny):
    m, greedy = tiny
    first = greedy[0][P]
    rows = m.generate_batch(CTX, BLOCK, NEW, temperature=0.0, banned_token_ids=[first])
    assert rows[0][P] != first and all(first not in r[P:] for r in rows)
    eager = list(m._generate_eager(CTX, BLOCK, NEW, 0.0, None, None, True, banned_token_ids=[first]))[-1]
    assert eager == rows[0]


def test_min_tokens_holds_the_stop_token_back(tiny):
    m, greedy = tiny
    s = greedy[0][P]
    assert m.generate_tokens(CTX[:1], BLOCK, NEW, temperature=0.0, stop_token=s) == CTX[0] + [s]
    for kw in (dict(stop_token=s), dict(stop=[[s]])):
        out = m.generate_tokens(CTX[:1], BLOCK, NEW, temperature=0.0, min_tokens=5, **kw)
        toks = (out[0] if isinstance(out, tuple) else out)[P:]
        assert len(toks) >= 5 and s not in toks[:5]
        if s in toks:
            assert toks.index(s) == len(toks) - 1  # and it still ends the call once it may come out
    streamed = list(m.generate_tokens_stream(CTX[:1], BLOCK, NEW, temperature=0.0, stop_token=s, min_tokens=5))
    assert streamed == m.generate_tokens(CTX[:1], BLOCK, NEW, temperature=0.0, stop_token=s, min_tokens=5)[P:]
    # a longer stop sequence is not held back
    seq = greedy[0][P:P + 2]
    tokens, info = m.generate_tokens(CTX[:1], BLOCK, NEW, temperature=0.0, stop=[seq], min_tokens=5)
    assert tokens[P:] == seq and info["finish_reason"] == "stop"


def test_neutral_forms_return_the_plain_tokens(tiny):
    m, _ = tiny
    kw = dict(temperature=1.0, top_k=5)
    torch.manual_seed(11)
    plain = m.generate_batch(CTX, BLOCK, NEW, **kw)
    for neutral in (dict(logit_bias=None, banned_token_ids=None, allowed_token_ids=None, min_tokens=None),
                    dict(logit_bias={}, banned_token_ids=[], min_tokens=0), dict(logit_bias={9: 0.0}),
                    dict(min_tokens=7)):
        torch.manual_seed(11)
        assert m.generate_batch(CTX, BLOCK, NEW, **neutral, **kw) == plain
    torch.manual_seed(11)
    assert m.generate_tokens(CTX, BLOCK, NEW, logit_bias={}, **kw) == plain[0]
    torch.manual_seed(11)
    assert list(m.generate_tokens_stream(CTX, BLOCK, NEW, banned_token_ids=[], **kw)) == plain[0][P:]


def test_logprobs_see_the_rewritten_logits(tiny):
    m, greedy = tiny
    first = greedy[0][P]
    tokens, info = m.generate_tokens(CTX[:1], BLOCK, 4, temperature=0.0, banned_token_ids=[first],
                                     allowed_token_ids=[first, 3, 77], logprobs=3)
    assert set(tokens[P:]) <= {3, 77}
    for top in info["top_logprobs"]:  # three ids asked for, two unmasked: the third is a masked one, far below
        assert [i for i, lp in top if lp > -1e29] and {i for i, lp in top if lp > -1e29} <= {3, 77}
        assert sum(lp < -1e29 for _, lp in top) == 1 and all(math.isfinite(lp) for _, lp in top)


@pytest.mark.parametrize("bad", [dict(logit_bias={1: 101}), dict(banned_token_ids=[V_MODEL]),
                                 dict(allowed_token_ids=[]), dict(min_tokens=3), dict(allowed_token_ids=[1], banned_token_ids=[1]),
                                 dict(banned_token_ids=[1], temperature=1e-7)],
                         ids=["bias", "beyondV", "allowed_empty", "min>max_new", "nothing_left", "temperature"])
def test_bad_values_fail_before_any_forward(monkeypatch, tiny, bad):
    m, _ = tiny

    def no_forward(*a, **k):
        raise AssertionError("forward ran before validation")

    monkeypatch.setattr(NeuralNetworkModel, "forward", no_forward)
    bad = dict(bad)
    t = bad.pop("temperature", 0.0)
    with pytest.raises(ValueError):
        m.generate_tokens([[1, 2]], 8, 2, temperature=t, **bad)
    with pytest.raises(ValueError):
        list(m.generate_tokens_stream([[1, 2]], 8, 2, temperature=t, **bad))
    with pytest.raises(ValueError):
        m.generate_batch([[1, 2]], 8, 2, temperature=t, **bad)
    with pytest.raises(ValueError):
        list(m._generate_eager([[1, 2]], 8, 2, t, None, None, True, **bad))


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1]], "block_size": 8, "max_new_tokens": 4}
FIELDS = ("logit_bias", "banned_token_ids", "allowed_token_ids", "min_tokens")


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m) as load:
        m.load = load
        yield m


def test_api_forwards_the_fields_only_when_set(served):
    served.generate_tokens.return_value = [1, 2, 3]
    body = {**BODY, "logit_bias": {"7": 1.5}, "banned_token_ids": [3], "allowed_token_ids": [7, 9], "min_tokens": 2}
    r = client.post("/generate/", json=body)
    assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}  # the response shape does not change
    kw = served.generate_tokens.call_args.kwargs
    assert kw["logit_bias"] == {"7": 1.5} and kw["banned_token_ids"] == [3]
    assert kw["allowed_token_ids"] == [7, 9] and kw["min_tokens"] == 2
    for body in (BODY, {**BODY, **{f: None for f in FIELDS}},
                 {**BODY, "logit_bias": {}, "banned_token_ids": [], "min_tokens": 0}):
        r = client.post("/generate/", json=body)
        assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
        assert not set(FIELDS) & set(served.generate_tokens.call_args.kwargs)
    served.generate_tokens_stream.return_value = iter([4, 5])
    r = client.post("/generate/", json={**BODY, "banned_token_ids": [5], "stream": True})
    assert r.text == "4\n5\n" and served.generate_tokens_stream.call_args.kwargs["banned_token_ids"] == [5]
    assert "logit_bias" not in served.generate_tokens_stream.call_args.kwargs


@pytest.mark.parametrize("bad", [{"logit_bias": {"7": 100.5}}, {"logit_bias": {"x": 1.0}}, {"banned_token_ids": [-1]},
                                 {"banned_token_ids": [True]}, {"allowed_token_ids": []}, {"min_tokens": 5},
                                 {"min_tokens": -1}, {"banned_token_ids": [1], "temperature": 1e-7},
                                 {"allowed_token_ids": [1], "banned_token_ids": [1]}],
                         ids=["bias", "key", "negative", "bool", "allowed_empty", "min>max_new", "min<0", "temperature",
                              "nothing_left"])
def test_api_bad_value_is_400_before_the_model_is_loaded(served, bad):
    assert client.post("/generate/", json={**BODY, **bad}).status_code == 400
    assert client.post("/generate/", json={**BODY, **bad, "stream": True}).status_code == 400
    served.load.assert_not_called()
    served.generate_tokens.assert_not_called()
    served.generate_tokens_stream.assert_not_called()
