"""Per-token log-probabilities on the device (csrc/kernels/token_logprobs.hip): the two kernels
against ``reference_logprobs`` on the CPU from the same rounded logits, and the decode path (graph
replay, eager steps, streaming) through tiny bf16 GPT and Gemma models.

Ids must match exactly. Values must be within ``1e-5 + 2^-22 (M + 13)``, M the row's largest |logit|:
a bound on fp32 rounding — a tree sum's worst case over <= 2^20 terms is about 5e-6 relative, two
units in ``log s <= 12.5``, and half-unit roundings of ``m + log s`` and ``x - lse``."""
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
from penroz.ops import logprobs as lp_ops
from penroz.ops.logprobs import LogprobState, reference_logprobs, token_logprobs

DEV = "cuda"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
NS = [0, 1, 5, 20]


def bound(x):
    """Per row [B, 1]."""
    return 1e-5 + 2.0 ** -22 * (x.float().abs().amax(dim=-1, keepdim=True) + 13.0)


def check(x, tok, n, got=None):
    """The kernels' (lp, top_id, top_lp) of CPU logits ``x`` against the reference; returns them (CPU)."""
    lp, ids, top = reference_logprobs(x, tok, n)
    if got is None:
        got = token_logprobs(x.to(DEV), tok.to(DEV), n)
    g_lp, g_id, g_top = (t.cpu() for t in got)
    assert g_lp.dtype == F32 and g_id.dtype == torch.int64 and g_top.dtype == F32
    assert g_lp.shape == lp.shape and g_id.shape == ids.shape and g_top.shape == top.shape
    assert torch.equal(g_id, ids)
    tol = bound(x)
    err_lp, err_top = (g_lp - lp).abs(), (g_top - top).abs()
    print(f"V={x.shape[1]} {x.dtype} n={n}: |lp err| {float(err_lp.max()):.3g}"
          f" |top err| {float(err_top.max()) if err_top.numel() else 0.0:.3g} bound {float(tol.min()):.3g}")
    assert bool((err_lp <= tol.view(-1)).all()) and bool((err_top <= tol).all())
    return g_lp, g_id, g_top


def rows(B, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * 4).to(dtype)  # bf16: full of exact ties


@pytest.mark.parametrize("n", NS)
def test_smallest_row_fp32(n):
    x = rows(1, 8, F32, 0)
    check(x, torch.tensor([5]), n)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V", [4095, 4096, 4097])
def test_part_edge_bf16(V, n):
    x = rows(2, V, BF, V)
    for toks in ([0, 4095], [4096, 0]):
        tok = torch.tensor(toks).clamp(max=V - 1)  # 0, 4095 and 4096 where the row has them
        check(x, tok, n)


@pytest.mark.parametrize("n", NS)
def test_gpt2_vocabulary_unaligned_rows_bf16(n):
    V = 50257
    x = rows(3, V, BF, 1)
    check(x, torch.tensor([0, V - 1, 12345]), n)


@pytest.mark.parametrize("n", [0, 20])
def test_gemma_vocabulary_64_parts_bf16(n):
    V = 262144
    x = rows(1, V, BF, 2)
    check(x, torch.tensor([V - 1]), n)


@pytest.mark.parametrize("n", NS)
def test_odd_row_fp16(n):
    x = rows(2, 3001, F16, 3)
    check(x, torch.tensor([[3000], [7]]), n)  # tokens [B, 1] as the sampler returns them


@pytest.mark.parametrize("dtype", [BF, F32])
def test_constant_row(dtype):
    V = 5000
    x = torch.full((2, V), -2.5).to(dtype)
    lp, ids, top = check(x, torch.tensor([V - 1, 0]), 20)
    assert ids.tolist() == [list(range(20))] * 2


@pytest.mark.parametrize("n", [1, 20])
def test_one_logit_far_above_the_rest(n):
    V = 4097
    x = rows(2, V, BF, 4).clamp(-8, 8)
    x[0, 4096] += 60.0
    x[1, 17] += 60.0
    lp, ids, top = check(x, torch.tensor([4096, 3]), n)
    assert ids[:, 0].tolist() == [4096, 17] and abs(lp[0].item()) < 1e-6 and lp[1].item() < -50.0


def test_n_above_a_tiny_vocabulary_is_clipped():
    x = rows(2, 5, F32, 5)
    lp, ids, top = check(x, torch.tensor([1, 4]), 20)
    assert ids.shape == (2, 5)


def test_two_runs_are_bitwise_equal():
    x = rows(3, 50257, BF, 6).to(DEV)
    tok = torch.tensor([1, 2, 3], device=DEV)
    a, b = token_logprobs(x, tok, 20), token_logprobs(x, tok, 20)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32) if u.dtype == F32 else u, v.view(torch.int32) if v.dtype == F32 else v)


def _step_args(B=2, V=16, cap=4):
    K = _ext.kernels()
    ws = torch.empty(B * K.token_logprobs_plan(V)[1], device=DEV)
    return dict(logits=torch.zeros(B, V, device=DEV), idx=torch.zeros(B, dtype=torch.long, device=DEV),
                step=torch.ones(1, dtype=torch.long, device=DEV), n_t=torch.full((1,), 3, dtype=torch.int32, device=DEV),
                lp_buf=torch.zeros(B, cap, device=DEV), top_id_buf=torch.zeros(B, cap, 20, dtype=torch.int32, device=DEV),
                top_lp_buf=torch.zeros(B, cap, 20, device=DEV), workspace=ws)


def test_step_form_writes_the_column_behind_the_counter_and_pads_the_slots():
    K = _ext.kernels()
    a = _step_args(B=2, V=16, cap=4)
    x = rows(2, 16, F32, 7)
    a["logits"], a["idx"], a["step"] = x.to(DEV), torch.tensor([3, 15], device=DEV), torch.tensor([3], device=DEV)
    before = a["lp_buf"].clone()
    K.token_logprobs_step(**a)
    lp, ids, top = reference_logprobs(x, torch.tensor([3, 15]), 3)
    assert torch.allclose(a["lp_buf"][:, 2].cpu(), lp, atol=2e-5)
    assert a["top_id_buf"][:, 2, :3].cpu().tolist() == ids.tolist()
    assert (a["top_id_buf"][:, 2, 3:] == -1).all() and (a["top_lp_buf"][:, 2, 3:] == float("-inf")).all()
    assert torch.equal(a["lp_buf"][:, [0, 1, 3]], before[:, [0, 1, 3]])  # no other column
    a["n_t"].fill_(20)  # n above V: the row's 16 logits, then empty slots
    K.token_logprobs_step(**a)
    assert sorted(a["top_id_buf"][0, 2, :16].tolist()) == list(range(16)) and (a["top_id_buf"][:, 2, 16:] == -1).all()


def test_launcher_refuses_mismatched_operands():
    K = _ext.kernels()
    x = torch.zeros(2, 16, device=DEV)
    tok = torch.zeros(2, dtype=torch.long, device=DEV)
    for bad in (lambda: K.token_logprobs(x, tok, 21),
                lambda: K.token_logprobs(x, tok, -1),
                lambda: K.token_logprobs(x.double(), tok, 3),
                lambda: K.token_logprobs(x, tok.int(), 3),
                lambda: K.token_logprobs(x, tok[:1], 3),
                lambda: K.token_logprobs(x, tok.cpu(), 3),
                lambda: K.token_logprobs(x.cpu(), tok, 3),
                lambda: K.token_logprobs(x.t(), tok, 3),
                lambda: K.token_logprobs(torch.zeros(1, (1 << 20) + 1, dtype=BF, device=DEV), tok[:1], 3)):
        with pytest.raises(RuntimeError):
            bad()
    good = _step_args()
    K.token_logprobs_step(**good)
    for name, wrong in (("workspace", good["workspace"][:-1]), ("workspace", good["workspace"].cpu()),
                        ("workspace", good["workspace"].double()), ("n_t", good["n_t"].long()),
                        ("n_t", good["n_t"].cpu()), ("step", good["step"].int()),
                        ("idx", good["idx"][:1]), ("idx", good["idx"].int()),
                        ("lp_buf", good["lp_buf"][:, :3]), ("lp_buf", good["lp_buf"].half()),
                        ("top_id_buf", good["top_id_buf"].long()), ("top_id_buf", good["top_id_buf"][:, :, :19]),
                        ("top_lp_buf", good["top_lp_buf"][:, :3]), ("logits", good["logits"][:1]),
                        ("logits", good["logits"].double())):
        with pytest.raises(RuntimeError):
            K.token_logprobs_step(**{**good, name: wrong})


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
BLOCK, NEW = 16, 40


def _ctx(nrows, seed=2):
    return torch.randint(0, 256, (nrows, 5), generator=torch.Generator().manual_seed(seed)).tolist()


class _EagerGraph:
    """Stands in for a captured graph: replay() runs the decode step eagerly."""

    def __init__(self, dec):
        self.dec = dec

    def replay(self):
        self.dec._step()


def _eager_capture(self, last_tok, cache_len, start=0):
    self._set_state(last_tok, cache_len, start)
    self.graph = _EagerGraph(self)


@pytest.mark.parametrize("nrows", ROWS)
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_graph_replay_eager_step_and_reference_agree(monkeypatch, kind, nrows):
    m = MODELS[kind]()
    ctx = _ctx(nrows)
    plain = m.generate_batch(ctx, BLOCK, NEW, temperature=0.0)  # through the sliding window too
    graphed, infos = m.generate_batch(ctx, BLOCK, NEW, temperature=0.0, logprobs=5)
    (dec,) = m._graph_decoders.values()
    assert dec.program is not None and dec._lp_on and isinstance(dec.graph, torch.cuda.CUDAGraph), "graph path not taken"
    assert graphed == plain and len(infos) == nrows
    for row, info in zip(graphed, infos):
        assert len(info["token_logprobs"]) == len(info["top_logprobs"]) == NEW
        for tok, lp, top in zip(row[5:], info["token_logprobs"], info["top_logprobs"]):
            assert len(top) == 5 and top[0] == [tok, lp] and lp <= 0.0  # greedy: the chosen token leads
            assert all(a[1] > b[1] or (a[1] == b[1] and a[0] < b[0]) for a, b in zip(top, top[1:]))
    # with a repetition penalty the distribution, and so the log-probabilities, differ
    _, pen = m.generate_batch(ctx, BLOCK, NEW, temperature=0.0, logprobs=5, repetition_penalty=1.3)
    assert pen != infos
    m.__dict__.pop("_graph_decoders")

    # the same step run eagerly: bitwise the same; and every step against the reference, from the
    # logits and the tokens the step function was handed
    seen = []
    step = lp_ops.step_logprobs

    def checking_step(state, logits, idx, step_t):
        step(state, logits, idx, step_t)
        col = int(step_t.item()) - 1
        seen.append(col)
        check(logits.cpu(), idx.cpu(), 5, got=(state.lp[:, col], state.top_id[:, col, :5].long(), state.top_lp[:, col, :5]))
        assert (state.top_id[:, col, 5:] == -1).all()

    monkeypatch.setattr(gd.GraphDecoder, "_capture", _eager_capture)
    monkeypatch.setattr(lp_ops, "step_logprobs", checking_step)
    assert m.generate_batch(ctx, BLOCK, NEW, temperature=0.0, logprobs=5) == (graphed, infos)
    assert 0 < len(seen) < NEW  # the decoder's steps; the prefill and the window-full re-prefills run eagerly


@pytest.mark.parametrize("nrows", [1, 6])
def test_one_decoder_a_graph_per_mode_and_n_never_recaptures(monkeypatch, nrows):
    m = _gpt()
    captures = []
    capture = gd.GraphDecoder._capture

    def counting_capture(self, *a, **k):
        captures.append((self._penalised, self._lp_on))
        return capture(self, *a, **k)

    monkeypatch.setattr(gd.GraphDecoder, "_capture", counting_capture)
    ctx = _ctx(nrows)

    def gen(**kw):
        return m.generate_batch(ctx, BLOCK, NEW, temperature=0.0, **kw)

    plain = gen()
    (dec,) = m._graph_decoders.values()
    g_plain = dec.graph
    assert captures == [(False, False)] and dec.logprobs is None
    five, info5 = gen(logprobs=5)
    g_lp = dec.graph
    assert captures == [(False, False), (False, True)] and g_lp is not g_plain and five == plain
    two, info2 = gen(logprobs=2)
    assert dec.graph is g_lp and two == plain and dec.logprobs.n_t.tolist() == [2]
    for a, b in zip(info2, info5):
        assert a["token_logprobs"] == b["token_logprobs"]
        assert a["top_logprobs"] == [t[:2] for t in b["top_logprobs"]]
    assert gen() == plain and dec.graph is g_plain
    assert list(m._graph_decoders.values()) == [dec]
    assert captures == [(False, False), (False, True)]


@pytest.mark.parametrize("nrows", ROWS)
def test_seeded_stream_equals_non_stream(nrows):
    m = _gpt()
    kw = dict(temperature=1.0, top_k=20, logprobs=4)
    ctx = _ctx(nrows)
    torch.manual_seed(7)
    whole, info = m.generate_tokens(ctx, BLOCK, NEW, **kw)  # one burst per window
    torch.manual_seed(7)
    streamed = list(m.generate_tokens_stream(ctx, BLOCK, NEW, **kw))  # bursts of 1
    assert ctx[0] + [s[0] for s in streamed] == whole
    assert [s[1] for s in streamed] == info["token_logprobs"] and [s[2] for s in streamed] == info["top_logprobs"]
    torch.manual_seed(7)
    assert m.generate_tokens(ctx, BLOCK, NEW, temperature=1.0, top_k=20) == whole
    # sampled: the chosen token is one of the 20 kept, not always the first
    assert all(lp <= top[0][1] for lp, top in zip(info["token_logprobs"], info["top_logprobs"]))
