"""Logit penalties on the device (csrc/kernels/logit_penalty.hip): the two kernels against
``reference_penalise`` on bookkeeping done here in dense torch, step by step, and the decode path
(graph replay, eager steps, streaming) through tiny bf16 GPT and Gemma models.

The kernel's arithmetic is fp32 without contraction, the reference's is torch's on the CPU (IEEE,
one rounding per operation), and both round once to the logits' dtype: the comparison is bitwise.
The case with arbitrary parameters allows the one unit in the last place of the logits' dtype that
contracting the frequency product into the sum could cost in the cases' value range."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode as gd
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops.penalties import PenaltyState, reference_penalise

DEV = "cuda"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16


def bits(t):
    """The elements' bit patterns as int64."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16).long()


def ordinal(t):
    """Position of each element on the number line of its dtype: adjacent values differ by 1."""
    b = bits(t)
    mask = 0x7FFFFFFF if t.dtype == F32 else 0x7FFF
    return torch.where(b < 0, -(b & mask), b)


class Dense:
    """The bookkeeping from the definition, dense and on the CPU."""

    def __init__(self, prompt, V):
        B = prompt.shape[0]
        self.in_prompt = torch.zeros(B, V, dtype=torch.bool)
        if prompt.numel():
            self.in_prompt.scatter_(1, prompt.cpu(), True)
        self.count = torch.zeros(B, V, dtype=torch.long)

    def add(self, new):
        if new is not None:
            self.count.scatter_add_(1, new.cpu().view(-1, 1), torch.ones(new.numel(), 1, dtype=torch.long))


def check_state(st, d):
    ip, oc = st.dense()
    assert torch.equal(ip.cpu(), d.in_prompt) and torch.equal(oc.cpu(), d.count)
    # the list holds exactly the tokens with a non-zero entry, each once
    for b, n in enumerate(st.n_uniq.tolist()):
        listed = st.uniq[b, :n].long().sort().values.cpu()
        assert torch.equal(listed, (d.in_prompt[b] | (d.count[b] > 0)).nonzero().view(-1))


def run_steps(V, dtype, prompt, news, params, ulp=0, seed=0):
    """begin(prompt), then one apply per entry of ``news`` (None or int64 [B]); after each, the
    logits against the reference (bitwise, or within ``ulp`` and untouched where nothing was seen) and
    dense() against the bookkeeping. Returns the state."""
    B = prompt.shape[0]
    st = PenaltyState()
    st.set_params(*params)
    st.begin(prompt.to(DEV))
    d = Dense(prompt, V)
    g = torch.Generator().manual_seed(seed)
    for new in news:
        x = (torch.randn(B, V, generator=g) * 4).to(dtype)
        x[:, ::7] = 0.0  # zeros among the positive and negative logits
        d.add(new)
        want = reference_penalise(x, d.in_prompt, d.count, *params)
        xd = x.to(DEV)
        got = st.apply(xd, None if new is None else new.to(DEV).view(B, 1))
        assert got is xd and got.dtype == dtype
        got = got.cpu()
        if ulp == 0:
            assert torch.equal(bits(got), bits(want))
        else:
            assert int((ordinal(got) - ordinal(want)).abs().max()) <= ulp
            unseen = ~(d.in_prompt | (d.count > 0))
            assert torch.equal(bits(got)[unseen], bits(x)[unseen])
        check_state(st, d)
    return st


EXACT = [(1.25, 0.5, 0.25), (2.0, 0.5, 0.25)]  # every product exact: contraction could not change a bit


@pytest.mark.parametrize("params", EXACT)
def test_smallest_case_step_by_step(params):
    prompt = torch.tensor([[3, 3, 5]])
    news = [None] + [torch.tensor([t]) for t in (5, 0, 7, 7)]
    st = run_steps(8, F32, prompt, news, params)
    ip, oc = st.dense()
    assert ip[0].tolist() == [v in (3, 5) for v in range(8)]
    assert oc[0].tolist() == [1, 0, 0, 0, 0, 1, 0, 2]
    assert st.n_uniq.tolist() == [4]


@pytest.mark.parametrize("params", EXACT)
def test_gpt2_vocabulary_odd_row_stride_bf16(params):
    B, V = 3, 50257
    g = torch.Generator().manual_seed(1)
    sub = torch.randperm(V, generator=g)[:300]
    prompt = sub[torch.randint(0, 300, (B, 700), generator=g)]  # 700 draws of 300 ids: duplicates
    prompt[0, 0], prompt[1, 5], prompt[2, 699] = 0, V - 1, 0
    prompt[0, 699] = V - 1
    news = [None] + [torch.randint(0, V, (B,), generator=g) for _ in range(3)]
    news += [news[-1].clone(), torch.tensor([0, V - 1, int(prompt[2, 3])])]  # a repeat; the edges; a prompt token
    st = run_steps(V, BF, prompt, news, params)
    assert all(n <= 300 + 2 + 5 for n in st.n_uniq.tolist())


def test_prompt_holding_every_token_fills_the_list():
    B, V = 2, 4096
    g = torch.Generator().manual_seed(2)
    prompt = torch.stack([torch.randperm(V, generator=g) for _ in range(B)])
    prompt = torch.cat([prompt, prompt[:, :100]], dim=1)  # and some twice
    news = [None] + [torch.randint(0, V, (B,), generator=g) for _ in range(2)]
    st = run_steps(V, BF, prompt, news, EXACT[0])
    assert st.n_uniq.tolist() == [V, V]


def test_sixty_four_rows_fp16():
    B, V = 64, 512
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, V, (B, 37), generator=g)
    news = [None] + [torch.randint(0, V // 8, (B,), generator=g) for _ in range(3)]  # a narrow range: repeats
    run_steps(V, F16, prompt, news, EXACT[1])


def test_second_begin_equals_a_fresh_state():
    B, V = 3, 1000
    g = torch.Generator().manual_seed(4)
    p1 = torch.randint(0, V, (B, 400), generator=g)
    news = [None] + [torch.randint(0, V, (B,), generator=g) for _ in range(3)]
    st = run_steps(V, BF, p1, news, EXACT[0])
    buffers = (st.cnt.data_ptr(), st.uniq.data_ptr(), st.n_uniq.data_ptr(), st.params.data_ptr())
    p2 = torch.randint(0, V, (B, 50), generator=g)  # shorter, mostly other tokens
    st.begin(p2.to(DEV))
    assert (st.cnt.data_ptr(), st.uniq.data_ptr(), st.n_uniq.data_ptr(), st.params.data_ptr()) == buffers
    d = Dense(p2, V)
    check_state(st, d)  # nothing of the first call is left: the sparse clear reached every entry
    fresh = PenaltyState()
    fresh.set_params(*EXACT[0])
    fresh.begin(p2.to(DEV))
    x = torch.randn(B, V, generator=g).to(BF)
    a, b = st.apply(x.to(DEV), None), fresh.apply(x.to(DEV), None)
    assert torch.equal(bits(a), bits(b))
    assert all(torch.equal(u, v) for u, v in zip(st.dense(), fresh.dense()))
    # other values reach the device without new buffers
    st.set_params(2.0, 0.0, 0.0)
    assert st.params.tolist() == [2.0, 0.0, 0.0] and st.params.data_ptr() == buffers[3]


@pytest.mark.parametrize("dtype", [BF, F32])
def test_arbitrary_parameters_within_one_unit_in_the_last_place(dtype):
    B, V = 4, 3001
    g = torch.Generator().manual_seed(5)
    prompt = torch.randint(0, V, (B, 200), generator=g)
    news = [None] + [torch.randint(0, 40, (B,), generator=g) for _ in range(5)]
    run_steps(V, dtype, prompt, news, (1.3, 0.37, 0.11), ulp=1)


def test_launcher_refuses_mismatched_operands():
    from penroz.ops import _ext
    K = _ext.kernels()
    cnt = torch.zeros(2, 16, dtype=torch.int32, device=DEV)
    uniq, n = torch.zeros_like(cnt), torch.zeros(2, dtype=torch.int32, device=DEV)
    par = torch.tensor([1.3, 0.0, 0.0], device=DEV)
    x = torch.zeros(2, 16, device=DEV)
    for bad in (lambda: K.penalty_apply(torch.zeros(2, 17, device=DEV), cnt, uniq, n, par, None),
                lambda: K.penalty_apply(x, cnt, uniq, n[:1], par, None),
                lambda: K.penalty_apply(x, cnt.long(), uniq, n, par, None),
                lambda: K.penalty_apply(x, cnt, uniq, n, par.cpu(), None),
                lambda: K.penalty_apply(x, cnt, uniq, n, par, torch.zeros(3, 1, dtype=torch.long, device=DEV)),
                lambda: K.penalty_apply(x.double(), cnt, uniq, n, par, None),
                lambda: K.penalty_begin(cnt, uniq, n, torch.zeros(3, 4, dtype=torch.long, device=DEV)),
                lambda: K.penalty_begin(cnt, uniq, n, torch.zeros(2, 4, dtype=torch.int32, device=DEV))):
        with pytest.raises(RuntimeError):
            bad()
    st = PenaltyState()
    st.set_params(1.3, 0.0, 0.0)
    st.begin(torch.tensor([[1, 16]], device=DEV))  # an id outside the vocabulary: refused on the host
    with pytest.raises(ValueError):
        st.apply(torch.zeros(1, 16, device=DEV), None)


# ------------------------------------------------------------------ the decode path
def _gpt():
    torch.manual_seed(11)
    m = NeuralNetworkModel("gd", Mapper(bench.gpt2_layers(V=256, C=128, L=2, H=2, P=64),
                                        {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=BF)


def _gemma():
    from types import SimpleNamespace
    tc = SimpleNamespace(vocab_size=256, hidden_size=64, num_attention_heads=4, num_key_value_heads=1,
                         head_dim=64, num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6,
                         rope_theta=10000.0, attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh",
                         model_type="gemma3_text")
    torch.manual_seed(5)
    m = NeuralNetworkModel("gg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=BF)


MODELS = {"gpt": _gpt, "gemma": _gemma}
ROWS = [1, 6, 40]  # one per kernel range of the decode programs


def _ctx(rows, seed=2):
    return torch.randint(0, 256, (rows, 5), generator=torch.Generator().manual_seed(seed)).tolist()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_greedy_with_a_huge_frequency_penalty_never_repeats(kind, rows):
    m = MODELS[kind]()
    out = m.generate_batch(_ctx(rows), 16, 40, temperature=0.0, frequency_penalty=1e4)
    assert len(out) == rows
    for row in out:
        assert len(row) == 45 and len(set(row[5:])) == 40, row
    decs = list(m._graph_decoders.values())
    assert len(decs) == 1 and decs[0].program is not None
    assert decs[0]._penalised and isinstance(decs[0].graph, torch.cuda.CUDAGraph), "graph path not taken"


class _EagerGraph:
    """Stands in for a captured graph: replay() runs the decode step eagerly."""

    def __init__(self, dec):
        self.dec = dec

    def replay(self):
        self.dec._step()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_graph_replay_matches_the_same_step_run_eagerly(monkeypatch, kind, rows):
    m = MODELS[kind]()
    kw = dict(temperature=0.0, repetition_penalty=1.3, presence_penalty=0.5)
    ctx = _ctx(rows)
    graphed = m.generate_batch(ctx, 16, 40, **kw)  # through the sliding window too
    assert all(isinstance(d.graph, torch.cuda.CUDAGraph) and d._penalised for d in m._graph_decoders.values())
    assert graphed != m.generate_batch(ctx, 16, 40, temperature=0.0), "the penalties changed nothing"
    m.__dict__.pop("_graph_decoders")

    def eager_capture(self, last_tok, cache_len, start=0):
        self._set_state(last_tok, cache_len, start)
        self.graph = _EagerGraph(self)

    monkeypatch.setattr(gd.GraphDecoder, "_capture", eager_capture)
    assert m.generate_batch(ctx, 16, 40, **kw) == graphed


@pytest.mark.parametrize("rows", ROWS)
def test_seeded_stream_equals_non_stream_with_penalties(rows):
    m = _gpt()
    kw = dict(temperature=1.0, top_k=20, repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)
    ctx = _ctx(rows)
    torch.manual_seed(7)
    whole = m.generate_tokens(ctx, 16, 40, **kw)  # one burst per window
    torch.manual_seed(7)
    streamed = list(m.generate_tokens_stream(ctx, 16, 40, **kw))  # bursts of 1
    assert ctx[0] + streamed == whole
    torch.manual_seed(7)
    assert m.generate_tokens(ctx, 16, 40, temperature=1.0, top_k=20) != whole


@pytest.mark.parametrize("rows", [1, 6])
def test_one_decoder_two_graphs_and_values_never_recapture(monkeypatch, rows):
    m = _gpt()
    captures, applies = [], []
    capture, apply = gd.GraphDecoder._capture, PenaltyState.apply

    def counting_capture(self, *a, **k):
        captures.append(self._penalised)
        return capture(self, *a, **k)

    def counting_apply(self, *a, **k):
        applies.append(1)
        return apply(self, *a, **k)

    monkeypatch.setattr(gd.GraphDecoder, "_capture", counting_capture)
    monkeypatch.setattr(PenaltyState, "apply", counting_apply)
    ctx = _ctx(rows)

    def gen(**kw):
        return m.generate_batch(ctx, 16, 40, temperature=0.0, **kw)

    plain = gen()
    (dec,) = m._graph_decoders.values()
    g_plain = dec.graph
    assert captures == [False] and not applies and dec.penalties is None
    a = gen(repetition_penalty=1.3)
    g_pen = dec.graph
    assert captures == [False, True] and g_pen is not g_plain and a != plain
    b = gen(repetition_penalty=2.0, presence_penalty=0.5)
    assert dec.graph is g_pen and b != a
    assert dec.penalties.params.tolist() == [2.0, 0.5, 0.0]
    assert list(m._graph_decoders.values()) == [dec]

    n = len(applies)
    neutral = gen(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    assert neutral == plain and dec.graph is g_plain and len(applies) == n  # the graph without the kernel
    assert gen(repetition_penalty=1.3) == a and dec.graph is g_pen  # per-call state: the same tokens again
    assert gen(repetition_penalty=2.0, presence_penalty=0.5) == b
    assert gen() == plain
    assert captures == [False, True]
