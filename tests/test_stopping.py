"""Stop sequences on the CPU: ``check_stop``'s limits, ``reference_stop`` on streams written by hand,
the dense ``StopState`` against it, generation through a tiny model, and the /generate schema."""
from unittest.mock import MagicMock, patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.stopping import MAX_LEN, MAX_SEQS, StopState, check_stop, reference_stop
from penroz.serve import app as A


# ------------------------------------------------------------------ validation
def test_check_stop_normalises_and_means_off_when_empty():
    assert check_stop(None) is None and check_stop([]) is None
    assert check_stop([[1], (2, 3)]) == [[1], [2, 3]]
    assert check_stop([[0, 255]], V=256) == [[0, 255]]
    assert check_stop([list(range(MAX_LEN))] * MAX_SEQS, V=MAX_LEN) == [list(range(MAX_LEN))] * MAX_SEQS


@pytest.mark.parametrize("bad", [
    [[1]] * (MAX_SEQS + 1),            # 17 sequences
    [list(range(MAX_LEN + 1))],        # 9 tokens
    [[1], []],                         # an empty sequence
    [[-1]], [[3, 256]],                # ids outside [0, V)
    [[1.5]], [[True]], [3], "12", [["1"]], 5,
], ids=["17seqs", "9tokens", "empty", "negative", "beyondV", "float", "bool", "flat", "str", "strid", "int"])
def test_check_stop_refuses(bad):
    with pytest.raises(ValueError):
        check_stop(bad, V=256)


def test_check_stop_without_a_vocabulary_takes_any_int32_id():
    assert check_stop([[2 ** 31 - 1]]) == [[2 ** 31 - 1]]
    with pytest.raises(ValueError):
        check_stop([[2 ** 31]])


# ------------------------------------------------------------------ the definition
def test_reference_overlapping_prefix():
    # [5, 5, 7] against 5 5 5 7: a matcher that restarts on a mismatch misses it
    assert reference_stop([[5, 5, 5, 7]], [[5, 5, 7]]) == ([4], [0])
    assert reference_stop([[5, 5, 5, 7, 5, 5, 7]], [[5, 5, 7]]) == ([4], [0])  # the first finish counts


def test_reference_lowest_index_among_sequences_ending_together():
    assert reference_stop([[1, 2, 3]], [[9], [2, 3], [3], [1, 2, 3]]) == ([3], [1])
    assert reference_stop([[1, 2, 3]], [[3], [2, 3]]) == ([3], [0])


def test_reference_sequence_longer_than_the_generated_tokens_never_matches():
    assert reference_stop([[1, 2]], [[0, 1, 2]]) == ([0], [-1])
    assert reference_stop([[]], [[1]]) == ([0], [-1])
    assert reference_stop([[4, 4, 4]], [[4, 4, 4, 4]]) == ([0], [-1])


def test_reference_smallest_t_across_lengths_and_rows_independent():
    # the long sequence [1, 2, 3, 4] would end at t = 4, the short [3] ends at t = 3 first
    assert reference_stop([[1, 2, 3, 4]], [[1, 2, 3, 4], [3]]) == ([3], [1])
    gen = torch.tensor([[1, 2, 3, 4], [4, 3, 2, 1], [0, 0, 0, 0]])
    assert reference_stop(gen, [[1, 2, 3, 4], [3]]) == ([3, 2, 0], [1, 1, -1])


# ------------------------------------------------------------------ the dense state
def feed(state: StopState, gen: torch.Tensor):
    """Feed [B, T] column by column; returns the tokens as ``observe`` left them."""
    out = gen.clone()
    for t in range(gen.shape[1]):
        col = out[:, t].clone()
        assert state.observe(col) is col
        out[:, t] = col
    return out


def expect_frozen(gen: torch.Tensor, finish_at):
    want = gen.clone()
    for b, at in enumerate(finish_at):
        if at:
            want[b, at:] = gen[b, at - 1]
    return want


STOP_SETS = [
    [[5, 5, 7]],
    [[9], [2, 3], [3], [1, 2, 3]],
    [[1, 2, 3, 4], [3]],
    [[(i + j) % 4 for j in range(MAX_LEN)] for i in range(MAX_SEQS)],
]


@pytest.mark.parametrize("stop", STOP_SETS, ids=["overlap", "ties", "lengths", "16x8"])
def test_dense_state_equals_the_reference_and_freezes(stop):
    g = torch.Generator().manual_seed(len(stop))
    gen = torch.randint(0, 4 if len(stop) == MAX_SEQS else 10, (33, 24), generator=g)
    gen[0, :4] = torch.tensor([5, 5, 5, 7])
    gen[1, :3] = torch.tensor([1, 2, 3])
    gen[2, 5:13] = torch.tensor(STOP_SETS[3][6])  # (equal to sequence 2 of that set: the lower index wins)
    gen[3] = 8  # never finishes under any of the sets
    finish_at, which = reference_stop(gen, stop)
    assert any(finish_at) and not all(finish_at)
    st = StopState(gen.shape[0], "cpu")
    st.set_stop(stop)
    st.begin()
    seen = feed(st, gen)
    done, fin = st.read()
    assert fin == finish_at and done == [w + 1 for w in which]
    assert torch.equal(seen, expect_frozen(gen, finish_at))
    toks, done2, fin2 = st.read(seen[:, -3:])
    assert toks == seen[:, -3:].tolist() and (done2, fin2) == (done, fin)


def test_begin_forgets_the_previous_call_and_sets_replace_each_other():
    st = StopState(2, "cpu")
    st.set_stop([[1, 2]])
    st.begin()
    feed(st, torch.tensor([[7, 1], [1, 2]]))
    assert st.read() == ([0, 1], [0, 2])
    st.begin()  # the 1 that ended the previous call's row 0 is forgotten: 2 alone completes nothing
    feed(st, torch.tensor([[2], [2]]))
    assert st.read() == ([0, 0], [0, 0])
    st.set_stop([[3], [2]])
    st.begin()
    seen = feed(st, torch.tensor([[2, 4], [3, 5]]))
    assert st.read() == ([2, 1], [1, 1]) and seen.tolist() == [[2, 2], [3, 3]]


def test_step_form_rewrites_idx_and_the_burst_column():
    st = StopState(2, "cpu")
    st.set_stop([[4]])
    st.begin()
    out = torch.zeros(2, 3, dtype=torch.long)
    for t, col in enumerate([[4, 1], [6, 2], [7, 4]]):
        idx = torch.tensor(col).view(2, 1)
        out[:, t] = idx.view(-1)  # (the sampler's write)
        st.step(idx, out, torch.tensor([t + 1]))
        assert idx.view(-1).tolist() == out[:, t].tolist()
    assert out.tolist() == [[4, 4, 4], [1, 2, 4]] and st.read() == ([1, 1], [1, 3])


# ------------------------------------------------------------------ through a tiny model
V_MODEL, BLOCK, NEW = 256, 16, 40
CTX = [[1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12], [13, 14, 15, 16, 17, 18]]
KW = dict(temperature=1.0, top_k=5)


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    m = NeuralNetworkModel("stop", Mapper(bench.gpt2_layers(V=V_MODEL, C=128, L=2, H=2, P=64), {"adamw": {"lr": 3e-3}}))
    torch.manual_seed(11)
    plain = m.generate_batch(CTX, BLOCK, NEW, **KW)
    return m, plain


def stops_from(plain):
    """Row 0's generated tokens 9-11, row 1's generated token 20; row 2 runs to length unless it meets them."""
    g = [r[6:] for r in plain]
    return [g[0][8:11], [g[1][19]]]


def cut(plain, stop):
    finish_at, which = reference_stop([r[6:] for r in plain], stop)
    rows = [r[:6 + at] if at else r for r, at in zip(plain, finish_at)]
    return rows, finish_at, which


def test_generate_batch_rows_finish_on_their_own(tiny):
    m, plain = tiny
    stop = stops_from(plain)
    want, finish_at, which = cut(plain, stop)
    assert finish_at[0] and finish_at[1]  # the sets were cut from these rows
    torch.manual_seed(11)
    contexts, infos = m.generate_batch(CTX, BLOCK, NEW, stop=stop, **KW)
    assert contexts == want
    for info, at, w in zip(infos, finish_at, which):
        assert info == ({"finish_reason": "stop", "stop_sequence": w} if at else
                        {"finish_reason": "length", "stop_sequence": None})


def test_generate_tokens_stream_eager_and_logprobs_agree(tiny):
    m, plain = tiny
    stop = stops_from(plain)
    want, finish_at, which = cut(plain, stop)
    torch.manual_seed(11)
    tokens, info = m.generate_tokens(CTX, BLOCK, NEW, stop=stop, **KW)
    assert tokens == want[0] and info == {"finish_reason": "stop", "stop_sequence": which[0]}
    torch.manual_seed(11)
    assert list(m.generate_tokens_stream(CTX, BLOCK, NEW, stop=stop, **KW)) == want[0][6:]
    torch.manual_seed(11)
    eager = list(m._generate_eager(CTX, BLOCK, NEW, 1.0, 5, None, True, stop=stop))[-1]
    assert eager == (tokens, info)
    torch.manual_seed(11)
    tokens2, info2 = m.generate_tokens(CTX, BLOCK, NEW, stop=stop, logprobs=2, **KW)
    assert tokens2 == tokens and info2["finish_reason"] == "stop" and info2["stop_sequence"] == which[0]
    assert len(info2["token_logprobs"]) == len(info2["top_logprobs"]) == finish_at[0]
    torch.manual_seed(11)
    contexts, infos = m.generate_batch(CTX, BLOCK, NEW, stop=stop, logprobs=2, **KW)
    assert contexts == want
    for ctx, inf in zip(contexts, infos):
        assert len(inf["token_logprobs"]) == len(inf["top_logprobs"]) == len(ctx) - 6


def test_nothing_is_sampled_past_the_finish(tiny):
    m, plain = tiny
    stop = [[plain[0][6]], [plain[1][6]], [plain[2][7]]]  # every row done after two tokens
    calls = []
    real = NeuralNetworkModel._generate_next_token

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    with patch.object(NeuralNetworkModel, "_generate_next_token", counted):
        torch.manual_seed(11)
        contexts, infos = m.generate_batch(CTX, BLOCK, NEW, stop=stop, **KW)
    assert max(len(c) for c in contexts) <= 8 and len(calls) <= 2
    assert all(i["finish_reason"] == "stop" for i in infos)


def test_stop_token_returns_what_it_did(tiny):
    m, plain = tiny
    torch.manual_seed(11)
    one = m.generate_tokens(CTX[:1], BLOCK, NEW, **KW)  # (one row draws other uniforms than three)
    s = one[6 + 4]
    torch.manual_seed(11)
    routed = m.generate_tokens(CTX[:1], BLOCK, NEW, stop_token=s, **KW)
    assert routed == one[:6 + one[6:].index(s) + 1]
    torch.manual_seed(11)
    assert list(m._generate_eager(CTX[:1], BLOCK, NEW, 1.0, 5, s, True))[-1] == routed
    torch.manual_seed(11)
    tokens, info = m.generate_tokens(CTX[:1], BLOCK, NEW, stop_token=s, logprobs=1, **KW)
    assert tokens == routed and set(info) == {"token_logprobs", "top_logprobs"}
    assert len(info["token_logprobs"]) == len(routed) - 6


@pytest.mark.parametrize("bad", [[[1]] * 17, [list(range(9))], [[]], [[V_MODEL]], [[-1]]],
                         ids=["17seqs", "9tokens", "empty", "beyondV", "negative"])
def test_bad_stop_fails_before_any_forward(monkeypatch, tiny, bad):
    m, _ = tiny

    def no_forward(*a, **k):
        raise AssertionError("forward ran before validation")

    monkeypatch.setattr(NeuralNetworkModel, "forward", no_forward)
    with pytest.raises(ValueError):
        m.generate_tokens([[1, 2]], 8, 2, temperature=0.0, stop=bad)
    with pytest.raises(ValueError):
        list(m.generate_tokens_stream([[1, 2]], 8, 2, temperature=0.0, stop=bad))
    with pytest.raises(ValueError):
        m.generate_batch([[1, 2]], 8, 2, temperature=0.0, stop=bad)
    with pytest.raises(ValueError):
        list(m._generate_eager([[1, 2]], 8, 2, 0.0, None, None, True, stop=bad))
    with pytest.raises(ValueError):
        m._generate_next_token(torch.tensor([[1, 2]]), 8, 0.0, None, stop=bad)
    with pytest.raises(ValueError):  # one stop condition per call
        m.generate_tokens([[1, 2]], 8, 2, temperature=0.0, stop=[[1]], stop_token=1)


def test_next_token_takes_stop_and_empty_stop_is_off(tiny):
    m, _ = tiny
    ctx = torch.tensor(CTX)
    plain = m._generate_next_token(ctx, BLOCK, 0.0, None)
    assert torch.equal(m._generate_next_token(ctx, BLOCK, 0.0, None, stop=[[int(plain[0])]]), plain)
    assert m.generate_tokens(CTX, BLOCK, 3, temperature=0.0, stop=[]) == m.generate_tokens(CTX, BLOCK, 3, temperature=0.0)


# ------------------------------------------------------------------ API
client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": [[1]], "block_size": 8, "max_new_tokens": 2}


@pytest.fixture
def served():
    m = MagicMock()
    with patch.object(A, "load_for_serving", return_value=m) as load:
        m.load = load
        yield m


def test_api_forwards_stop_and_returns_the_finish_only_when_asked(served):
    served.generate_tokens.return_value = ([1, 2, 3], {"finish_reason": "stop", "stop_sequence": 1})
    r = client.post("/generate/", json={**BODY, "stop": [[9], [2, 3]]})
    assert r.status_code == 200
    assert r.json() == {"tokens": [1, 2, 3], "finish_reason": "stop", "stop_sequence": 1}
    assert served.generate_tokens.call_args.kwargs["stop"] == [[9], [2, 3]]
    # with log-probabilities: both, the finish at the top level
    served.generate_tokens.return_value = ([1, 2], {"token_logprobs": [-0.5], "top_logprobs": [[]],
                                                    "finish_reason": "length", "stop_sequence": None})
    r = client.post("/generate/", json={**BODY, "stop": [[9]], "logprobs": 0})
    assert r.json() == {"tokens": [1, 2], "finish_reason": "length", "stop_sequence": None,
                        "logprobs": {"token_logprobs": [-0.5], "top_logprobs": [[]]}}
    # without stop (absent, null or empty) the call and the response are what they were
    served.generate_tokens.return_value = [1, 2, 3]
    for body in (BODY, {**BODY, "stop": None}, {**BODY, "stop": []}):
        r = client.post("/generate/", json=body)
        assert r.status_code == 200 and r.json() == {"tokens": [1, 2, 3]}
        assert "stop" not in served.generate_tokens.call_args.kwargs
    served.generate_tokens_stream.return_value = iter([4, 5])
    r = client.post("/generate/", json={**BODY, "stop": [[5]], "stream": True})
    assert r.text == "4\n5\n" and served.generate_tokens_stream.call_args.kwargs["stop"] == [[5]]


@pytest.mark.parametrize("bad", [[[1]] * 17, [list(range(9))], [[]], [[-1]]], ids=["17seqs", "9tokens", "empty", "negative"])
def test_api_bad_stop_is_400_before_the_model_is_loaded(served, bad):
    assert client.post("/generate/", json={**BODY, "stop": bad}).status_code == 400
    assert client.post("/generate/", json={**BODY, "stop": bad, "stream": True}).status_code == 400
    served.load.assert_not_called()
    served.generate_tokens.assert_not_called()
    served.generate_tokens_stream.assert_not_called()


def test_api_stop_with_stop_token_is_400(served):
    assert client.post("/generate/", json={**BODY, "stop": [[1]], "stop_token": 1}).status_code == 400
    served.load.assert_not_called()
