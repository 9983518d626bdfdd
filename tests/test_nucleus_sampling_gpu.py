"""Nucleus (top-p) and min-p sampling on the device (csrc/kernels/sampling.hip) against an fp64
oracle written here from the definition, on every sampler path:

  reg      sample_reg_kernel, row in registers: V = 1024 fp32 (fewer occupied threads than the
           block) and V = 40 960 bf16 (the widest slice the nucleus instantiations take)
  stream   sample_kernel: V = 50 257 bf16 (odd V), V = 4096 fp16, and V = 50 304 bf16 (GPT-2's
           padded vocabulary: too wide for the nucleus register kernel), alone and with top_k = 100
  rank     sample_reg_kernel's rank-ordered top-k <= 512 path: V = 40 960, top_k = 100
  merge    sample_part_kernel + sample_merge_kernel: V = 8192 (two parts) and V = 262 144, top_k = 50

Definition (ops/sampling.py): S = the set the top-k stage keeps, w = exp((x - max)/T), Z = sum_S w;
top-p keeps i iff the mass of the strictly larger logits is < top_p * Z, min-p iff w_i >= min_p.

Error bound behind the margins: the fp32 weights carry ~30 * 2^-24 ~ 2e-6 relative error from the
exponent argument, a few ulp from __expf and a few 2^-24 from the sums, ~1e-5 in all (the kernel's
2^-40 fixed-point quantum adds < 3e-7). The planted rows keep every prefix mass 1e-3 * Z away from
the cut (a hundredfold), the random rows are checked against the nucleus of top_p + 1e-4 (tenfold).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext, sampling as Sa

DEV = "cuda"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16

# (V, dtype, top_k, exact_k). exact_k: the path keeps exactly k candidates (value descending,
# index ascending); the others keep every logit >= the k-th largest.
PATHS = {
    "reg-1024-fp32": (1024, F32, 0, False),
    "reg-40960-bf16": (40960, BF, 0, False),
    "stream-50304-bf16": (50304, BF, 0, False),
    "stream-50304-k100": (50304, BF, 100, False),
    "stream-50257-bf16": (50257, BF, 0, False),
    "stream-4096-fp16": (4096, F16, 0, False),
    "rank-40960-k100": (40960, BF, 100, True),
    "merge-8192-k50": (8192, F32, 50, False),
    "merge-262144-k50": (262144, BF, 50, False),
}
ALL = sorted(PATHS)


FREQ = {"reg": (1024, F32, 0), "stream": (4096, F16, 0), "rank": (1024, BF, 100), "merge": (8192, BF, 50)}
# sample_plan's path (0 two-stage, 1 register, 2 streaming) that each label's prefix stands for
LABEL_PATH = {"merge": 0, "reg": 1, "rank": 1, "stream": 2}


@pytest.mark.parametrize("path", ALL + sorted(FREQ))
def test_labels_name_the_kernel_the_launcher_picks(path):
    """The launcher's own plan for the case with top_p = 0.9, at every row count the tests below use."""
    V, dt, k = (PATHS[path] if path in PATHS else FREQ[path])[:3]
    for B in (1, 8, 32, 64, 256, 2048, 4000):
        assert _ext.kernels().sample_plan(dt, B, V, 0.8, k, True)[0] == LABEL_PATH[path.split("-")[0]], B


def oracle(logits, T, top_k, exact_k, top_p=1.0, min_p=0.0):
    """fp64: (kept mask [B, V], renormalised probabilities [B, V], prefix masses / Z in
    descending-logit order [B, V])."""
    x = logits.double()
    xs, order = torch.sort(x, dim=-1, descending=True, stable=True)
    in_s = torch.ones_like(xs, dtype=torch.bool)
    if top_k and top_k < x.shape[1]:
        if exact_k:
            in_s[:, top_k:] = False
        else:
            in_s = xs >= xs[:, top_k - 1:top_k]
    w = torch.exp((xs - xs[:, :1]) / T) * in_s
    Z = w.sum(-1, keepdim=True)
    cum = w.cumsum(-1)
    first = torch.searchsorted((-xs).contiguous(), (-xs).contiguous())  # first entry of each run of equals
    above = (cum - w).gather(1, first)
    keep = in_s & (above < top_p * Z) & (w >= min_p)
    p = w * keep
    p = p / p.sum(-1, keepdim=True)
    mask = torch.zeros_like(keep).scatter_(1, order, keep)
    probs = torch.zeros_like(p).scatter_(1, order, p)
    return mask, probs, cum / Z


def planted(V, dt, values, where):
    row = torch.full((1, V), -40.0, device=DEV)
    row[0, where] = torch.tensor(values, device=DEV)
    return row.to(dt)


def hot_indices(V):
    """12 scattered indices: both ends, a pair inside one register-kernel thread's 8-logit chunk
    (16, 17), a pair owned by one streaming-kernel thread (5, 5 + 1024 where it exists) and a
    pair across the 4096-logit part boundary (where it exists)."""
    cand = [0, V - 1, 16, 17, 5, 1029, 4095, 4096, V // 2 + 3, V // 3, V - 9, 200, 777, V // 5 + 1, 300]
    out = []
    for i in cand:
        if 0 <= i < V and i not in out:
            out.append(i)
    return out[:12]


def grid(G):
    return (torch.arange(G, device=DEV, dtype=torch.float32) + 0.5) / G


def draw_set(row, G, T, k, **kw):
    rows = row.expand(G, row.shape[1]).contiguous()
    t = _ext.kernels().sample_tokens(rows, grid(G), T, k, kw.get("top_p", 1.0), kw.get("min_p", 0.0))
    return set(t.view(-1).tolist())


@pytest.mark.parametrize("path", ALL)
def test_exact_kept_set(path):
    """Geometrically falling planted masses: the set of tokens drawn over a grid of G uniforms is
    exactly the fp64 nucleus, for two top_p that keep different counts."""
    V, dt, k, exact = PATHS[path]
    G = 256 if V > 100000 else 2048
    where = hot_indices(V)
    row = planted(V, dt, [j * math.log(0.6) for j in range(len(where))], where)
    counts = []
    for top_p in (0.7, 0.95):
        mask, probs, prefix = oracle(row, 1.0, k, exact, top_p=top_p)
        # asserted in fp64 before the GPU sampler runs: the cut is far from every prefix mass, and
        # the grid of G uniforms reaches every nucleus member
        assert float((prefix - top_p).abs().min()) > 1e-3
        assert float(probs[mask].min()) >= 4.0 / G
        nucleus = set(mask[0].nonzero().view(-1).tolist())
        assert nucleus <= set(where)
        counts.append(len(nucleus))
        assert draw_set(row, G, 1.0, k, top_p=top_p) == nucleus
    assert counts[0] < counts[1]


@pytest.mark.parametrize("path", ALL)
def test_ties_stay_or_go_together(path):
    """w = 1, 1/2, 1/2, 1/8, 1/8 (Z = 2.25), top_p = 0.6 (1.35): the first pair straddles the cut
    (1 < 1.35 <= 1.5) and both are drawn; the second pair lies below it and neither is."""
    V, dt, k, exact = PATHS[path]
    G = 256 if V > 100000 else 2048
    a, b, c, d, e = 40, 3, V - 2, 100, 101
    row = planted(V, dt, [0.0, math.log(0.5), math.log(0.5), math.log(0.125), math.log(0.125)], [a, b, c, d, e])
    assert row[0, b] == row[0, c] and row[0, d] == row[0, e]
    mask, probs, prefix = oracle(row, 1.0, k, exact, top_p=0.6)
    assert set(mask[0].nonzero().view(-1).tolist()) == {a, b, c}
    assert float((prefix - 0.6).abs().min()) > 1e-3 and float(probs[mask].min()) >= 4.0 / G
    assert draw_set(row, G, 1.0, k, top_p=0.6) == {a, b, c}


@pytest.mark.parametrize("path", ALL)
def test_random_rows_draw_inside_the_nucleus(path):
    V, dt, k, exact = PATHS[path]
    B = 8 if V > 100000 else 64
    torch.manual_seed(V + k)
    logits = (torch.randn(B, V, device=DEV) * 3).to(dt)
    mask, _, _ = oracle(logits, 0.8, k, exact, top_p=0.9 + 1e-4)
    assert int(mask.sum(-1).max()) < V // 2  # the check below cannot pass vacuously
    K = _ext.kernels()
    for u in (0.0, 0.37, 0.999):
        t = K.sample_tokens(logits, torch.full((B,), u, device=DEV), 0.8, k, 0.9, 0.0)
        assert bool(mask.gather(1, t).all()), (path, u)
        again = K.sample_tokens(logits, torch.full((B,), u, device=DEV), 0.8, k, 0.9, 0.0)
        assert torch.equal(t, again)  # same inputs, same tokens


@pytest.mark.parametrize("cut", ["top_p", "min_p"])
@pytest.mark.parametrize("path", sorted(FREQ))
def test_frequencies_follow_the_renormalised_softmax(path, cut):
    """Four planted logits, three kept (softmax 0.474, 0.287, 0.174 | 0.064: top_p = 0.9 cuts after
    the third; w = 1, 0.61, 0.37 | 0.14: so does min_p = 0.2). 4000 draws."""
    V, dt, k = FREQ[path]
    hot = [7, V - 1, V // 2 + 1, 300]
    row = planted(V, dt, [2.0, 1.5, 1.0, 0.0], hot)
    rows = row.expand(4000, V).contiguous()
    torch.manual_seed(3)
    kw = {"top_p": 0.9} if cut == "top_p" else {"min_p": 0.2}
    draws = Sa.sample(rows, 1.0, k or None, **kw).view(-1).cpu()
    assert bool(torch.isin(draws, torch.tensor(hot[:3])).all())
    freq = torch.stack([(draws == h).float().mean() for h in hot[:3]])
    assert torch.allclose(freq, torch.softmax(torch.tensor([2.0, 1.5, 1.0]), -1), atol=0.03), freq


@pytest.mark.parametrize("path", ALL)
def test_defaults_untouched_and_repeatable(path):
    V, dt, k, _ = PATHS[path]
    B = 8 if V > 100000 else 32
    torch.manual_seed(1)
    logits = (torch.randn(B, V, device=DEV) * 3).to(dt)
    u = torch.rand(B, device=DEV)
    K = _ext.kernels()
    for T in (0.0, 0.8):
        assert torch.equal(K.sample_tokens(logits, u, T, k), K.sample_tokens(logits, u, T, k, 1.0, 0.0))
    greedy = K.sample_tokens(logits, u, 0.0, k)
    assert torch.equal(K.sample_tokens(logits, u, 0.0, k, 0.5, 0.5), greedy)  # temperature 0 ignores both
    lf = logits.float()  # a vanishing nucleus: the maximum (or what ties with it)
    assert torch.equal(lf.gather(1, K.sample_tokens(logits, u, 0.8, k, 1e-6, 0.0)), lf.amax(-1, keepdim=True))
    assert torch.equal(lf.gather(1, K.sample_tokens(logits, u, 0.8, k, 1.0, 0.999999)), lf.amax(-1, keepdim=True))
    a = K.sample_tokens(logits, u, 0.8, k, 0.9, 0.05)
    assert torch.equal(a, K.sample_tokens(logits, u, 0.8, k, 0.9, 0.05))
    for bad in ((0.0, 0.0), (1.5, 0.0), (0.9, -0.1), (0.9, 1.0)):
        with pytest.raises(RuntimeError):
            K.sample_tokens(logits, u, 0.8, k, *bad)


@pytest.mark.parametrize("B,V,topk,exact", [(1, 50304, 0, False), (3, 40960, 100, True), (64, 50304, 50, False)])
def test_sample_step_nucleus_and_fused_advance(B, V, topk, exact):
    """sample_step with top_p: tokens inside the nucleus, placed in idx_out and out_buf[:, step];
    with the counters the same tokens, written at the OLD step, and (pos, len, step) advanced
    once per call (the manner of test_sample_step_fused_advance)."""
    K = _ext.kernels()
    n = 6
    torch.manual_seed(B + topk)
    logits = (torch.randn(B, V, device=DEV) * 3).to(BF)
    mask, _, _ = oracle(logits, 0.8, topk, exact, top_p=0.9 + 1e-4)
    seed = torch.tensor([99], device=DEV)
    ref_idx = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    ref_out = torch.full((B, n), -1, dtype=torch.long, device=DEV)
    idx = torch.zeros_like(ref_idx)
    out = torch.full_like(ref_out, -1)
    pos, ln, step = (torch.tensor([v], device=DEV) for v in (10, 11, 0))
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(4):
        K.sample_step(logits, 0.8, topk, seed, torch.tensor([s], device=DEV), ref_idx, ref_out, None, None, None,
                      0.9, 0.0)
        K.sample_step(logits, 0.8, topk, seed, step, idx, out, pos, ln, done, 0.9, 0.0)
        torch.cuda.synchronize()
        assert bool(mask.gather(1, ref_idx).all()), s
        assert torch.equal(ref_out[:, s], ref_idx.view(-1))
        assert torch.equal(idx, ref_idx), s
        assert (pos.item(), ln.item(), step.item(), done.item()) == (11 + s, 12 + s, 1 + s, 0)
    assert torch.equal(out[:, :4], ref_out[:, :4]) and bool((out[:, 4:] == -1).all())


# ------------------------------------------------------------------ graph decode
def _gpt(dtype):
    torch.manual_seed(11)
    m = NeuralNetworkModel("gd", Mapper(bench.gpt2_layers(V=256, C=128, L=2, H=2, P=64),
                                        {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=dtype) if dtype == BF else m


def _gemma(dtype):
    from types import SimpleNamespace
    tc = SimpleNamespace(vocab_size=256, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=64,
                         num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                         attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
    torch.manual_seed(5)
    m = NeuralNetworkModel("gg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=dtype) if dtype == BF else m


MODELS = [(_gpt, BF), (_gpt, F32), (_gemma, BF), (_gemma, F32)]
MODEL_IDS = ["gpt-bf16", "gpt-fp32", "gemma-bf16", "gemma-fp32"]


@pytest.mark.parametrize("make,dtype", MODELS, ids=MODEL_IDS)
def test_graph_decode_vanishing_nucleus_is_greedy(make, dtype):
    """top_p = 1e-6 keeps the maximum (and what ties with it) only, so the graph-sampled tokens
    equal the greedy ones for as long as the per-step maximum is unique."""
    m = make(dtype)
    ctx, n = [[7, 3, 9, 1]], 8
    greedy = m.generate_tokens(ctx, 32, n, temperature=0.0)
    with torch.inference_mode():
        acts, _ = m(torch.tensor([greedy[:-1]], device=DEV), skip_softmax=True)
    top2 = acts[-1][0, len(ctx[0]) - 1:].float().topk(2, dim=-1).values  # the n positions that were sampled
    unique = (top2[:, 0] > top2[:, 1]).tolist()
    steps = unique.index(False) if False in unique else n
    assert steps >= 1, "the very first maximum ties: pick another context"
    torch.manual_seed(0)
    nucleus = m.generate_tokens(ctx, 32, n, temperature=1.0, top_p=1e-6)
    assert nucleus[:len(ctx[0]) + steps] == greedy[:len(ctx[0]) + steps]
    assert any(d.graph is not None and d.top_p == 1e-6 for d in m._graph_decoders.values()), "graph path not taken"


@pytest.mark.parametrize("make,dtype", MODELS, ids=MODEL_IDS)
def test_graph_decode_seeded_stream_equals_non_stream(make, dtype):
    m = make(dtype)
    ctx = [[7, 3, 9]]
    for _ in range(2):  # 1st: the stream captures the graph; 2nd: both reuse it
        torch.manual_seed(42)
        streamed = list(m.generate_tokens_stream(ctx, 16, 40, temperature=1.0, top_p=0.9))
        torch.manual_seed(42)
        full = m.generate_tokens(ctx, 16, 40, temperature=1.0, top_p=0.9)
        assert len(streamed) == 40
        assert full == ctx[0] + streamed
    decs = list(m._graph_decoders.values())
    assert len(decs) == 1 and decs[0].graph is not None and decs[0].top_p == 0.9
    # another top_p: another decoder (the captured sampler call carries the value)
    m.generate_tokens(ctx, 16, 4, temperature=1.0, top_p=0.5)
    assert len(m._graph_decoders) == 2 and sorted(d.top_p for d in m._graph_decoders.values()) == [0.5, 0.9]
    # values that mean "no filter", and any value at temperature 0, share the plain decoder
    m._graph_decoders.clear()
    m.generate_tokens(ctx, 16, 4, temperature=0.0, top_p=0.5, min_p=0.5)
    m.generate_tokens(ctx, 16, 4, temperature=0.0)
    assert len(m._graph_decoders) == 1
