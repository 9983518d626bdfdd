"""Beam search on MI355X: csrc/kernels/beam_search.hip (``beam_step``, ``beam_reorder``) against the fp64 definition
(ops/beam_search.py) and ``index_select``, a device loop over a logit table, and ``generate_tokens(num_beams=...)``
end to end on the shared-prefix step.

The bound on a selected score: the kernel's lse sums V terms in fp32 — 17 serial additions per thread, then a tree of
log2(256 P) levels, each rounding <= 2^-24 of the sum, and expf / logf good to 2 ulp — so lse is off by at most
(log2 V + 20) 2^-24 absolutely; (x - lse) + c rounds twice more, each within an ulp of a magnitude <= 2 |s|:
``tol(s) = 4 |s| 2^-23 + (log2 V + 20) 2^-24``. Ranks whose fp64 neighbours are further than 2 tol apart must agree in
(beam, token); the seeds are chosen so that at least 90 % of the ranks are such and the rest are exact ties."""
import math
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import beam_search as bs


def tol(s: float, V: int) -> float:
    return 4 * abs(s) * 2.0 ** -23 + (math.log2(V) + 20) * 2.0 ** -24


def _check_ranks(got, ranked, V):
    """``got`` / ``ranked``: (s, b, v) best first. Scores rank by rank; (b, v) where the reference's neighbours are apart."""
    apart = 0
    for r, ((s, b, v), (rs, rb, rv)) in enumerate(zip(got, ranked)):
        assert abs(s - rs) <= tol(rs, V), (r, s, rs)
        near = [abs(ranked[j][0] - rs) for j in (r - 1, r + 1) if 0 <= j < len(ranked)]
        if min(near) > 2 * tol(rs, V):
            apart += 1
            assert (b, v) == (rb, rv), (r, (b, v), (rb, rv))
    assert apart >= 0.9 * len(ranked), (apart, len(ranked))


@pytest.mark.parametrize("R, W, V, stop, seed", [(1, 2, 4099, 17, 4100), (2, 2, 4099, None, 4101), (4, 4, 50257, 50256, 50261),
                                                 (8, 8, 262144, 4096, 1)])  # (seeds: see the module docstring)
def test_beam_step_matches_the_fp64_step(R, W, V, stop, seed):
    g = torch.Generator().manual_seed(seed)
    wide = (torch.randn(R, V + 24, generator=g) * 3).bfloat16()
    if stop is not None:
        wide[:2, stop] = 14.0  # the stop token among the best of (up to) two beams
    cum = (-5 * torch.rand(R, generator=g)).tolist() if R > 1 else [0.0]
    logits = wide.cuda()[:, :V]  # rows carry a stride larger than V
    T, t = 4, (1 if R == 1 else 2)
    st = bs.BeamState(W, T, V, "cuda")
    st.begin(T, stop, 1.5, rows=R, cum=cum, step=t - 1)
    idx = torch.zeros(W, dtype=torch.long, device="cuda")
    st.step(logits, idx)
    fin = []
    tokens, parents, new_cum, ranked = bs.reference_step(wide[:, :V], cum, W, t, stop, st._inv_host, fin)
    got = st.read()
    assert got["step"] == t and idx.tolist() == tokens and got["parent"][:W] == parents
    assert got["hist"][t - 1] == [list(e) for e in zip(tokens, parents)]
    walked = sorted(list(zip(got["cum"], parents, tokens)) + [(f[1], f[3], f[5]) for f in got["finished"]], key=lambda e: -e[0])
    ref_walked = sorted(list(zip(new_cum, parents, tokens)) + [(f[1], f[3], f[5]) for f in fin], key=lambda e: -e[0])
    _check_ranks(walked, ref_walked, V)
    assert [f[2:] for f in got["finished"]] == [f[2:] for f in fin] and (stop is None) == (not fin)
    for f, rf in zip(got["finished"], fin):
        assert abs(f[0] - rf[0]) <= tol(rf[1], V) * float(st._inv_host[t]) + abs(rf[0]) * 2.0 ** -23
    st.begin(T, stop, 1.5, rows=R, cum=cum, step=T)  # a step behind the last writes nothing
    before = st.buf.clone()
    st.step(logits, idx)
    assert torch.equal(st.buf, before) and idx.tolist() == tokens


def test_exact_ties_order_by_beam_then_token():
    W, V, lo, hi = 4, 4099, 7, 4098  # the two equal maxima lie in different parts
    row = torch.zeros(V).bfloat16()
    row[lo] = row[hi] = 5.0
    st = bs.BeamState(W, 2, V, "cuda")
    st.begin(2, None, 1.0, rows=W, cum=[-1.0] * W, step=1)
    idx = torch.zeros(W, dtype=torch.long, device="cuda")
    st.step(row.repeat(W, 1).cuda(), idx)
    got = st.read()
    assert idx.tolist() == [lo, hi, lo, hi] and got["parent"][:W] == [0, 0, 1, 1]
    assert len({torch.tensor(c).view(torch.int32).item() for c in got["cum"][:W]}) == 1  # bit-equal


LAYERS = [(1, 256), (12, 64)]  # (Hkv, D): two layers of different shapes in one launch
CAP = 70


@pytest.mark.parametrize("kind", ["identity", "cycle", "from_one"])
@pytest.mark.parametrize("n", [0, 1, 37])  # 37 ends inside a 4-KiB piece at both head dims
@pytest.mark.parametrize("W", [2, 8])
def test_beam_reorder_is_index_select(W, n, kind):
    g = torch.Generator("cuda").manual_seed(W + n)
    ks = [torch.randn(W, h, CAP, d, device="cuda", generator=g).bfloat16() for h, d in LAYERS]
    vs = [torch.randn(W, h, CAP, d, device="cuda", generator=g).bfloat16() for h, d in LAYERS]
    parent = {"identity": list(range(W)), "cycle": [(r + 1) % W for r in range(W)], "from_one": [W - 1] * W}[kind]
    sel = torch.tensor(parent, device="cuda")
    want = [c.clone() for c in ks + vs]
    for c in want:
        c[:, :, :n] = c[:, :, :n].index_select(0, sel)
    table = bs.ReorderTable(ks, vs)
    table.apply(sel.int(), torch.tensor([n], dtype=torch.int32, device="cuda"))
    for c, w in zip(ks + vs, want):  # slots from n on are untouched
        assert torch.equal(c.view(torch.int16), w.view(torch.int16))


@lru_cache(maxsize=None)
def _table(V=4099):
    g = torch.Generator().manual_seed(5)
    t = (torch.randn(V, V, generator=g) * 3).bfloat16()
    t[::3, 11] = 12.0  # token 11, the stop token of one case, is likely behind every third token
    return t, t.cuda()


@pytest.mark.parametrize("stop", [None, 11])
def test_device_loop_over_a_logit_table(stop):
    """Twelve steps with no host read in between: a beam's logits are the table row of its last token."""
    W, T, V, first = 4, 12, 4099, 1
    host, dev = _table()
    st = bs.BeamState(W, T, V, "cuda")
    st.begin(T, stop, 0.8)
    idx = torch.zeros(W, dtype=torch.long, device="cuda")
    st.step(dev[first:first + 1], idx)
    for _ in range(T - 1):
        st.step(dev[idx], idx)
    beams = st.beams()
    ref = bs.reference_generate(lambda seqs, parents: host[[s[-1] if s else first for s in seqs]], W, T, stop, 0.8)
    assert [(b["tokens"], b["finished"]) for b in beams] == [(b["tokens"], b["finished"]) for b in ref]
    for b, r in zip(beams, ref):
        assert abs(b["cum_logprob"] - r["cum_logprob"]) <= T * tol(r["cum_logprob"], V), (b, r)
    assert stop is None or any(b["finished"] for b in beams)


V, BLOCK, NEW, PROMPT = 256, 64, 16, [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]


@lru_cache(maxsize=None)
def _model(kind):
    if kind == "gpt":  # MHA, head_dim 64
        torch.manual_seed(11)
        m = NeuralNetworkModel("bmg", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    else:  # Gemma style: RoPE, head_dim 256, 4:1 GQA
        tc = SimpleNamespace(vocab_size=V, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=256,
                             num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                             attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
        torch.manual_seed(5)
        m = NeuralNetworkModel("bmgg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}}))
    return m.to("cuda").to(dtype=torch.bfloat16).eval()


@lru_cache(maxsize=None)
def _d0(kind):
    """The largest per-token gap between the ``logprobs`` option and ``score_tokens`` on a plain greedy call."""
    m = _model(kind)
    tokens, info = m.generate_tokens([PROMPT], BLOCK, NEW, temperature=0.0, logprobs=0)
    scored = m.score_tokens([tokens], BLOCK)[0]["token_logprobs"][len(PROMPT):]
    return max(abs(a - b) for a, b in zip(info["token_logprobs"], scored))


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_generate_tokens_beams_carry_their_own_scores(kind, W, monkeypatch):
    m, d0 = _model(kind), _d0(kind)
    tokens, info = m.generate_tokens([PROMPT], BLOCK, NEW, num_beams=W, length_penalty=1.0)
    beams = info["beams"]
    assert m.last_beam_search["path"] == "device" and len(beams) == W and tokens == PROMPT + beams[0]["tokens"]
    assert len({tuple(b["tokens"]) for b in beams}) == W
    assert all(a["score"] >= b["score"] for a, b in zip(beams, beams[1:]))
    for b in beams:  # a wrong parent or a wrong reorder misses this by O(1)
        scored = m.score_tokens([PROMPT + b["tokens"]], BLOCK)[0]["token_logprobs"][len(PROMPT):]
        print(f"beam {kind} W={W}: cum {b['cum_logprob']:.5f} scored {sum(scored):.5f} d0 {d0:.3e}")
        assert len(b["tokens"]) == NEW and abs(b["cum_logprob"] - sum(scored)) <= NEW * 2 * d0, (b, sum(scored), d0)
    monkeypatch.setenv("PENROZ_SHARED_PREFIX", "0")
    _, again = m.generate_tokens([PROMPT], BLOCK, NEW, num_beams=W, length_penalty=1.0)
    assert m.last_beam_search["path"] == "reference" and len(again["beams"]) == W
    assert all(set(b) == set(beams[0]) and len(b["tokens"]) == NEW for b in again["beams"])
