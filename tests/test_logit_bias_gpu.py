"""Logit bias, banned and allowed tokens and ``min_tokens`` on the device (csrc/kernels/logit_bias.hip):
the kernel against ``reference_bias`` through ``BiasState``, step by step and bitwise — the add is one fp32
sum rounded once on both sides, FLOOR is exact — and the decode path (graph bursts, eager steps, the
window's re-prefill, streaming, penalties, log-probabilities, stop sequences) through tiny bf16 GPT and
Gemma models."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode as gd
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext
from penroz.ops.logit_bias import MAX_ENTRIES, BiasState, check_logit_bias, floor_of, reference_bias

DEV = "cuda"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
MIN_TOKENS = 3


def bits(t):
    """The elements' bit patterns as int64."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16).long()


# ------------------------------------------------------------------ the kernel
def make_case(V, n, mask, seed):
    """A canonical form of exactly ``n`` entries over V, ids 0 and V - 1 among them (n >= 2): by turns a
    bias, a banned id, an end token with a bias and an end token without; with ``mask`` an allowed set
    of the entries' ids and about a third of the others."""
    g = torch.Generator().manual_seed(seed)
    perm = [v for v in torch.randperm(V, generator=g).tolist() if v not in (0, V - 1)]
    ids = ([0, V - 1] + perm)[:n] if n >= 2 else perm[:n]
    rest = perm[max(n - 2, 0) if n >= 2 else n:]
    bias, banned, ends = {}, [], []
    for i, v in enumerate(ids):
        b = float(torch.empty(1).uniform_(-100, 100, generator=g)) if i % 8 else 0.25 * (i % 64 - 32)
        if i % 4 == 1:
            banned.append(v)
        if i % 4 in (0, 2) or i % 8 == 1:  # (one banned id in two has a bias as well: the ban wins)
            bias[v] = b or 1.0
        if i % 4 >= 2:
            ends.append(v)
    allowed = None
    if mask:
        allowed = ids + rest[:max(1, len(rest) // 3)]
    c = check_logit_bias(bias, banned, allowed, MIN_TOKENS, ends, V, 10)
    assert len(c.ids) == n and (c.allowed is not None) == mask
    if n >= 2:
        assert c.ids[0] == 0 and c.ids[-1] == V - 1
    return c


def run_steps(st, c, B, V, dtype, seed):
    """set(c), then eager applies at t = 0 and MIN_TOKENS - 1 and captured-form steps at t = MIN_TOKENS and
    beyond: each against the reference, bitwise, and bit-identical to the input outside the write set."""
    st.set(c)
    assert st.form == ("mask" if c.allowed is not None else "entries")
    g = torch.Generator().manual_seed(seed)
    touched = torch.zeros(V, dtype=torch.bool)
    touched[torch.tensor(c.ids, dtype=torch.long)] = True
    if c.allowed is not None:
        keep = torch.zeros(V, dtype=torch.bool)
        keep[torch.tensor(c.allowed, dtype=torch.long)] = True
        touched |= ~keep
    step_t = torch.zeros(1, dtype=torch.long, device=DEV)
    for t, base, step in ((0, None, None), (MIN_TOKENS - 1, None, None), (MIN_TOKENS, MIN_TOKENS - 1, 1), (7, 2, 5)):
        x = (torch.randn(B, V, generator=g) * 4).to(dtype)
        x[:, ::7] = 0.0
        want = reference_bias(x, c, t)
        xd = x.to(DEV)
        if base is None:
            got = st.apply(xd, t)
            assert st.base_t.tolist() == [t]
        else:
            st.base_t.fill_(base)
            step_t.fill_(step)
            got = st.step(xd, step_t)
        assert got is xd and got.dtype == dtype
        got = got.cpu()
        assert torch.equal(bits(got), bits(want)), (t, (bits(got) != bits(want)).nonzero()[:8].tolist())
        assert torch.equal(bits(got)[:, ~touched], bits(x)[:, ~touched])
        assert bool((got[:, touched] != x[:, touched]).any()) or not touched.any()


CASES = [  # B, V, dtype, entries
    (1, 8, F32, 3),           # the smallest
    (2, 31, F32, 1),          # one partial mask word
    (2, 33, F32, 5),          # a full word and one bit
    (3, 50257, BF, 257),      # odd row stride; 25 mask parts, the last ragged; a second round of entries
    (2, 262144, BF, 1024),    # every entry slot; 128 mask parts per row
    (2, 4099, F16, 257),      # fp16: FLOOR -2^15; three mask parts, the last of 3 tokens
    (3, 2048, BF, 0),         # no entries: the mask alone, exactly one part
]


# both launch forms of every case; no entries and no mask is "off", which launches nothing
FORMS = [(*c, mask) for c in CASES for mask in (False, True) if c[3] or mask]


@pytest.mark.parametrize("B,V,dtype,n,mask", FORMS,
                         ids=[f"V{c[1]}-n{c[3]}-{'mask' if c[4] else 'entries'}" for c in FORMS])
def test_kernel_equals_the_reference(B, V, dtype, n, mask):
    st = BiasState(DEV)
    c = make_case(V, n, mask, seed=V + n)
    run_steps(st, c, B, V, dtype, seed=1)
    if n:
        # t on both sides of until, on an end token: FLOOR at t = MIN_TOKENS - 1, the sum at t = MIN_TOKENS
        end = next((v for v, b, u in c.entries if u == MIN_TOKENS), None)
        if end is not None:
            x = torch.ones(B, V, dtype=dtype, device=DEV)
            assert float(st.apply(x.clone(), MIN_TOKENS - 1)[0, end]) == floor_of(dtype)
            assert float(st.apply(x.clone(), MIN_TOKENS)[0, end]) != floor_of(dtype)
    # another call on the same buffers: other values, another set, the other entry count
    other = make_case(V, min(n + 2, V - 1, MAX_ENTRIES) if n else 0, mask, seed=V + n + 1)
    run_steps(st, other, B, V, dtype, seed=2)


def test_one_state_serves_both_forms_in_turn():
    st = BiasState(DEV)
    for mask in (True, False, True):
        run_steps(st, make_case(4099, 9, mask, seed=int(mask)), 2, 4099, BF, seed=3)
    x = torch.randn(2, 4099, device=DEV)
    st.set(None)
    assert st.form == "off" and st.apply(x, 0) is x and st.step(x, torch.zeros(1, dtype=torch.long, device=DEV)) is x


def test_kernel_refuses_operands_of_another_shape():
    k = _ext.kernels()
    st = BiasState(DEV)
    st.set(check_logit_bias({1: 1.0}, None, [1, 2], 0, (), 40, 4))
    x = torch.zeros(2, 40, device=DEV)
    step = torch.zeros(1, dtype=torch.long, device=DEV)

    def call(logits=x, ids=st.ids, bias=st.bias, until=st.until, n=st.n_entries, allow=st.allow, allow_on=True,
             base=st.base_t, step_t=step):
        k.logit_bias_apply(logits, ids, bias, until, n, allow, allow_on, base, step_t)

    call()
    call(allow=None, allow_on=False, step_t=None)
    for bad in (dict(logits=torch.zeros(2, 40)),                               # a host tensor
                dict(logits=torch.zeros(2, 80, device=DEV)[:, ::2]),           # strided
                dict(logits=torch.zeros(40, device=DEV)),                      # one dimension
                dict(logits=torch.zeros(2, 40, dtype=torch.int32, device=DEV)),
                dict(logits=torch.zeros(2, 80, device=DEV)),                   # a mask of another vocabulary
                dict(ids=st.ids[:512]), dict(ids=st.ids.long()), dict(ids=st.ids.cpu()),
                dict(bias=st.bias.double()), dict(bias=st.bias[:1000]),
                dict(until=st.until.view(2, 512)), dict(n=torch.zeros(2, dtype=torch.int32, device=DEV)),
                dict(allow=None), dict(allow=st.allow.long()), dict(allow=torch.zeros(3, dtype=torch.int32, device=DEV)),
                dict(base=st.base_t.int()), dict(base=st.base_t.cpu()), dict(step_t=step.int())):
        with pytest.raises(RuntimeError):
            call(**bad)
    with pytest.raises(ValueError):  # the state checks the vocabulary it was set for
        st.apply(torch.zeros(2, 41, device=DEV), 0)
    assert k.logit_bias_plan(64, 262144, True) == (129, 64 * 129, 8192) and k.logit_bias_plan(0, 8, True) == (0, 0, 0)


# ------------------------------------------------------------------ graph decode
BLOCK, NEW, P = 16, 40, 6  # 6 + 40 tokens through a window of 16: it re-prefills twice
KW = dict(temperature=1.0, top_k=5)
SEED = 7
ROWS = [1, 3]


def _ctx(nrows):
    return torch.randint(0, 256, (nrows, P), generator=torch.Generator().manual_seed(2)).tolist()


def _gpt():
    torch.manual_seed(11)
    m = NeuralNetworkModel("bias", Mapper(bench.gpt2_layers(V=256, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    return m.to(DEV).to(dtype=BF)


def _gemma():
    from types import SimpleNamespace
    tc = SimpleNamespace(vocab_size=256, hidden_size=64, num_attention_heads=4, num_key_value_heads=1,
                         head_dim=64, num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6,
                         rope_theta=10000.0, attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh",
                         model_type="gemma3_text")
    torch.manual_seed(5)
    m = NeuralNetworkModel("gg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=BF)


@pytest.fixture(scope="module")
def gpt():
    return _gpt()


def _dec(m, rows, temperature=1.0, top_k=5):
    (dec,) = [d for d in m._graph_decoders.values()
              if d.rows == rows and d.temperature == temperature and d.top_k == (top_k if temperature else None)]
    return dec


@pytest.fixture(scope="module")
def plain(gpt):
    """The runs without constraints, per row count: sampled (KW, SEED) and greedy. Computed once."""
    out = {}
    for rows in ROWS:
        torch.manual_seed(SEED)
        out[rows] = gpt.generate_batch(_ctx(rows), BLOCK, NEW, **KW)
        out[rows, "greedy"] = gpt.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0)
    return out


def graph_taken(m, rows, temperature, form, top_k=5):
    dec = _dec(m, rows, temperature, top_k)
    assert dec._bias_form == form and isinstance(dec.graph, torch.cuda.CUDAGraph), "graph path not taken"
    return dec


@pytest.mark.parametrize("rows", ROWS)
def test_a_bias_of_100_wins_every_step(gpt, plain, rows):
    out = gpt.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0, logit_bias={7: 100})
    assert [r[P:] for r in out] == [[7] * NEW] * rows
    graph_taken(gpt, rows, 0.0, "entries")


@pytest.mark.parametrize("rows", ROWS)
def test_allowed_set_holds_for_every_row_and_token(gpt, plain, rows):
    allowed = [3, 77, 250]
    torch.manual_seed(SEED)
    out = gpt.generate_batch(_ctx(rows), BLOCK, NEW, temperature=1.0, top_k=50, allowed_token_ids=allowed)
    assert all(len(r) == P + NEW and set(r[P:]) <= set(allowed) for r in out)
    assert len({t for r in out for t in r[P:]}) > 1  # (it does sample among them)
    graph_taken(gpt, rows, 1.0, "mask", top_k=50)


@pytest.mark.parametrize("rows", ROWS)
def test_banned_first_token_changes_it(gpt, plain, rows):
    first = plain[rows, "greedy"][0][P]
    out = gpt.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0, banned_token_ids=[first])
    assert out[0][P] != first and all(first not in r[P:] for r in out)
    graph_taken(gpt, rows, 0.0, "entries")


@pytest.mark.parametrize("rows", ROWS)
def test_min_tokens_holds_the_stop_token_back(gpt, plain, rows):
    """``generate_batch`` checks the stop token on the host, per burst; ``generate_tokens`` with one row on
    the device, as the sequence [s]; with three rows on the host, per token."""
    s = plain[rows][0][P]
    torch.manual_seed(SEED)
    out = gpt.generate_batch(_ctx(rows), BLOCK, NEW, stop_token=s, min_tokens=5, **KW)
    assert all(len(r) >= P + 5 and s not in r[P:P + 5] for r in out)
    graph_taken(gpt, rows, 1.0, "entries")
    torch.manual_seed(SEED)
    toks = gpt.generate_tokens(_ctx(rows), BLOCK, NEW, stop_token=s, min_tokens=5, **KW)[P:]
    assert len(toks) >= 5 and s not in toks[:5]
    torch.manual_seed(SEED)
    tokens, info = gpt.generate_tokens(_ctx(rows), BLOCK, NEW, stop=[[s]], min_tokens=5, **KW)
    assert len(tokens) >= P + 5 and s not in tokens[P:P + 5] and s not in tokens[P:-1]
    assert info["finish_reason"] == ("stop" if tokens[-1] == s else "length")
    if rows == 1:  # the routed stop token is the same device check: the same tokens, and it still ends the call
        torch.manual_seed(SEED)
        assert gpt.generate_tokens(_ctx(rows), BLOCK, NEW, stop_token=s, **KW) == plain[rows][0][:P + 1]
        assert tokens[P:] == toks


@pytest.mark.parametrize("rows", ROWS)
def test_graphed_run_equals_the_eager_loop_at_temperature_0(monkeypatch, rows):
    """(The module-forward graph: the same GEMMs as the eager loop, so the greedy choice cannot differ by a
    rounding — as in test_stopping_gpu's eager comparison. The decode programs run in every other test.)
    One row: the stop token takes the device check in the graphed run, the host check in the eager loop."""
    monkeypatch.setattr(gd, "DECODE_PROGRAM", False)
    m = _gpt()
    ctx = _ctx(rows)
    free = m.generate_batch(ctx, BLOCK, NEW, temperature=0.0)
    s = free[0][P + 1]
    for kw in (dict(logit_bias={5: 3.0, 9: -50.0, s: 1.5}, banned_token_ids=[free[0][P], free[-1][P + 3]], min_tokens=9,
                    stop_token=s),
               dict(allowed_token_ids=list(range(0, 256, 3)), logit_bias={3: 2.0, 4: 100.0}, banned_token_ids=[6])):
        got = m.generate_tokens(ctx, BLOCK, NEW, temperature=0.0, **kw)
        kw = dict(kw)
        eager = list(m._generate_eager(ctx, BLOCK, NEW, 0.0, None, kw.pop("stop_token", None), True, **kw))[-1]
        assert got == eager and got != free[0]
        dec = _dec(m, rows, 0.0, None)
        assert dec.program is None and isinstance(dec.graph, torch.cuda.CUDAGraph), "graph path not taken"
        assert dec._bias_form == ("mask" if "allowed_token_ids" in kw else "entries")


@pytest.mark.parametrize("rows", ROWS)
def test_gemma_pattern_model(rows):
    m = _gemma()
    free = m.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0)
    out = m.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0, logit_bias={7: 100})
    assert [r[P:] for r in out] == [[7] * NEW] * rows
    allowed = [3, 77, 250]
    torch.manual_seed(SEED)
    out = m.generate_batch(_ctx(rows), BLOCK, NEW, temperature=1.0, top_k=50, allowed_token_ids=allowed,
                           banned_token_ids=[77])
    assert all(set(r[P:]) <= {3, 250} for r in out)
    first = free[0][P]
    out = m.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0, banned_token_ids=[first])
    assert out[0][P] != first and all(first not in r[P:] for r in out)
    decs = list(m._graph_decoders.values())
    assert all(d.program is not None and isinstance(d.graph, torch.cuda.CUDAGraph) for d in decs)
    assert sorted(d._bias_form for d in decs) == ["entries", "mask"]
    assert m.generate_batch(_ctx(rows), BLOCK, NEW, temperature=0.0) == free


@pytest.mark.parametrize("rows", ROWS)
def test_with_penalties_logprobs_and_stop_together(gpt, plain, rows):
    banned = [plain[rows][0][P], plain[rows][0][P + 1]]
    allowed = sorted(set(range(0, 256, 2)) | set(banned))
    stop = [[254, 252, 250]]
    torch.manual_seed(SEED)
    contexts, infos = gpt.generate_batch(_ctx(rows), BLOCK, NEW, repetition_penalty=1.3, logprobs=2, stop=stop,
                                         banned_token_ids=banned, allowed_token_ids=allowed, logit_bias={8: 2.0},
                                         **KW)
    dec = graph_taken(gpt, rows, 1.0, "mask")
    assert dec._penalised and dec._lp_on and dec._stop_on
    unmasked = set(allowed) - set(banned)
    for ctx, info in zip(contexts, infos):
        assert set(ctx[P:]) <= unmasked and len(info["token_logprobs"]) == len(ctx) - P
        assert all(math.isfinite(lp) and lp > -1e29 for lp in info["token_logprobs"])
        for top in info["top_logprobs"]:
            assert len(top) == 2 and all(i in unmasked for i, lp in top if lp > -1e29)
    # a banned token's log-probability is below -1e29: ask for more ids than stay unmasked
    two = [v for v in (2, 4, 6, 8) if v not in banned][:2]
    torch.manual_seed(SEED)
    _, infos = gpt.generate_batch(_ctx(rows), BLOCK, 4, logprobs=3, banned_token_ids=banned,
                                  allowed_token_ids=banned + two, **KW)
    for info in infos:
        for top in info["top_logprobs"]:
            assert {i for i, lp in top if lp > -1e29} == set(two)
            assert all(lp < -1e29 and math.isfinite(lp) for i, lp in top if i not in two) and len(top) == 3


@pytest.mark.parametrize("rows", ROWS)
def test_other_values_replay_the_same_graph_and_the_plain_call_is_off(gpt, plain, rows):
    torch.manual_seed(SEED)
    gpt.generate_batch(_ctx(rows), BLOCK, NEW, logit_bias={5: 1.0}, min_tokens=2, stop_token=9, **KW)
    dec = graph_taken(gpt, rows, 1.0, "entries")
    g_entries = dec.graph
    torch.manual_seed(SEED)
    a = gpt.generate_batch(_ctx(rows), BLOCK, NEW, logit_bias={8: -3.0, 200: 4.5}, banned_token_ids=[1, 2, 3],
                           min_tokens=11, stop_token=9, **KW)
    assert dec.graph is g_entries and dec.bias.n_entries.tolist() == [6] and a != plain[rows]
    assert all(9 not in r[P:P + 11] and not {1, 2, 3} & set(r[P:]) for r in a)
    torch.manual_seed(SEED)
    b = gpt.generate_batch(_ctx(rows), BLOCK, NEW, allowed_token_ids=list(range(100)), **KW)
    g_mask = dec.graph
    assert dec._bias_form == "mask" and g_mask is not g_entries and isinstance(g_mask, torch.cuda.CUDAGraph)
    torch.manual_seed(SEED)
    c = gpt.generate_batch(_ctx(rows), BLOCK, NEW, allowed_token_ids=list(range(50, 256)), logit_bias={60: 1.0}, **KW)
    assert dec.graph is g_mask and all(max(r[P:]) < 100 for r in b) and all(min(r[P:]) >= 50 for r in c)
    # the plain call afterwards: the fixture's tokens, the mode off
    torch.manual_seed(SEED)
    assert gpt.generate_batch(_ctx(rows), BLOCK, NEW, **KW) == plain[rows]
    assert dec._bias_form == "off" and dec.graph is not g_mask and dec.graph is not g_entries
    torch.manual_seed(SEED)
    assert gpt.generate_batch(_ctx(rows), BLOCK, NEW, logit_bias={}, banned_token_ids=[], min_tokens=0, **KW) == plain[rows]
    assert dec._bias_form == "off"
    torch.manual_seed(SEED)
    assert gpt.generate_batch(_ctx(rows), BLOCK, NEW, logit_bias={8: -3.0, 200: 4.5}, banned_token_ids=[1, 2, 3],
                              min_tokens=11, stop_token=9, **KW) == a
    assert dec.graph is g_entries


@pytest.mark.parametrize("rows", ROWS)
def test_stream_equals_the_whole_call(gpt, plain, rows):
    kw = dict(logit_bias={5: 4.0, 6: -4.0}, banned_token_ids=[plain[rows][0][P]], allowed_token_ids=list(range(1, 256, 2)) +
              [plain[rows][0][P]], min_tokens=4, stop_token=plain[rows][0][P + 2], **KW)
    torch.manual_seed(SEED)
    whole = gpt.generate_tokens(_ctx(rows), BLOCK, NEW, **kw)
    torch.manual_seed(SEED)
    assert list(gpt.generate_tokens_stream(_ctx(rows), BLOCK, NEW, **kw)) == whole[P:]
    assert whole[P] != plain[rows][0][P] and set(whole[P:]) <= set(kw["allowed_token_ids"])
