"""Ragged batches through the captured decode step (models/graph_decode.py, ``GraphDecoder(ragged=True)``)
on MI355X: every row at its own position and cache length.

Teacher-forced ragged program steps against a one-row, cache-free module forward over each row's true
sequence, with the uniform decoder on a rectangular control as the yardstick of what bf16 rounding does at
these shapes; equal lengths through the ragged decoder against the uniform one; generate_batch end to end
(graph replay vs the eager stand-in, the chosen tokens against cache-free reference logits, seeded
sampling); everything else of a request composed in one ragged call; int8 decode weights."""
import math
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode as gd
from penroz.models import kv_cache as kvc
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import ragged
from penroz.ops.stopping import reference_stop

V, CAP, STEPS = 256, 32, 3


@lru_cache(maxsize=None)
def _model(kind):
    if kind in ("gpt", "gpt-lossless"):
        torch.manual_seed(11)
        m = NeuralNetworkModel("rg", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    else:  # Gemma style: RoPE, head_dim 256, 4:1 GQA, RMSNorm, gated MLP
        tc = SimpleNamespace(vocab_size=V, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=256,
                             num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                             attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
        torch.manual_seed(5)
        m = NeuralNetworkModel("rgg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}}))
    m = m.to("cuda").to(dtype=torch.bfloat16).eval()
    return _make_lossless(m) if kind == "gpt-lossless" else m


def _make_lossless(model):
    """Every nn.Linear weight becomes k · 2^-e (integer |k| <= 127, ±127 in every row, e by row) at about its
    initial magnitude — the int8 weight tests' construction: quantised without loss, so an int8 step and the
    bf16 module forward compute one function and the bf16 bounds apply to it."""
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for mod in model.modules():
            if type(mod) is not torch.nn.Linear:
                continue
            N, K = mod.weight.shape
            k = torch.randint(-127, 128, (N, K), generator=g)
            k[:, 0], k[:, K - 1] = 127, -127
            e = round(math.log2(73.0 * math.sqrt(K))) + torch.arange(N) % 3
            w = k.float() * torch.exp2(-e.float()).unsqueeze(1)
            mod.weight.copy_(w.to(mod.weight.dtype))
            assert torch.equal(mod.weight.float().cpu(), w)
    return model


def _lens(rows):
    """Distinct within the batch, 1 and the longest included: 1 + (5·b mod 9) up to 9 rows, a permutation of
    1..rows above (5 and 24 are coprime)."""
    return [1 + (5 * b) % max(rows, 9) for b in range(rows)]


def _tokens(rows, n, seed):
    return torch.randint(0, V, (rows, n), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


@lru_cache(maxsize=None)
def _reference_logits(kind, rows, which):
    """(lens, sequences [rows, Lmax + STEPS], ref [rows, STEPS, V] fp32): row b's true sequence is its first
    lens[b] + STEPS tokens; ref[b, i] are the logits of a one-row, cache-free module forward over it at
    position lens[b] + i, where teacher-forced step i runs. ``which``: "ragged" or "rect" (every row 6 long).
    Computed once per (model, rows) and shared."""
    m = _model(kind)
    lens = _lens(rows) if which == "ragged" else [6] * rows
    seq = _tokens(rows, max(lens) + STEPS, 3)
    ref = torch.empty(rows, STEPS, V, device="cuda")
    with torch.inference_mode():
        for b, n in enumerate(lens):
            acts, _ = m._forward_nocache(seq[b:b + 1, :n + STEPS])
            ref[b] = acts[-1][0, n:n + STEPS].float()
    return lens, seq, ref


def _forced_steps(kind, rows, which, steps=STEPS, weight_quant=None):
    """Teacher-forced program steps -> (got [rows, steps, V] fp32, ref, decoder). Prefill padded through the
    modules with the decoder's cache attached; step i feeds row b its token at position lens[b] + i."""
    m = _model(kind)
    lens, seq, ref = _reference_logits(kind, rows, which)
    is_ragged = which == "ragged"
    dec = gd.GraphDecoder(m, rows, CAP, 0.0, None, weight_quant=weight_quant, ragged=is_ragged)
    assert dec.program is not None
    lmax = max(lens)
    prompts = [seq[b, :n].tolist() for b, n in enumerate(lens)]
    padded = torch.tensor(ragged.pad_prompts(prompts), device="cuda")
    lens_t = torch.tensor(lens, device="cuda")
    got = torch.empty(rows, steps, V, device="cuda")
    with torch.inference_mode():
        dec.attach()
        try:
            m(padded, skip_softmax=True)  # prefill through the modules
            assert dec.cache.seq_len() == lmax
            for i in range(steps):
                tok = seq.gather(1, (lens_t + i).unsqueeze(1))
                dec._set_state(tok, lens_t + i if is_ragged else lmax + i)
                dec.cache.graph_mode = True
                dec.cache.begin_step()
                try:
                    got[:, i] = dec.program.forward(tok, dec.cache).float()
                finally:
                    dec.cache.graph_mode = False
        finally:
            dec.detach()
    return got, ref[:, :steps], dec


def _row_errors(got, ref):
    """Per row and step: ||got - ref|| / ||ref||."""
    return ((got - ref).norm(dim=-1) / ref.norm(dim=-1))


@pytest.mark.parametrize("kind,rows", [("gpt", 3), ("gpt", 6), ("gpt", 24), ("gemma", 3), ("gemma", 24)])
def test_teacher_forced_ragged_steps_match_the_one_row_forward(kind, rows):
    """GPT rows 3 / 6 / 24: the GEMV, fused and batched regimes; Gemma 3 / 24: decode GEMVs and decode_gemm,
    both with the plain QKV linear and the RoPE pass over a [rows, D/2] table. Rows hold different data, so
    bf16 rounding scatters between them: ragged's worst row may be at most twice the uniform decoder's worst
    on a rectangular control, where a wrong position or a stale pad key gives errors of order 1."""
    got, ref, _ = _forced_steps(kind, rows, "ragged")
    ctl_got, ctl_ref, _ = _forced_steps(kind, rows, "rect")
    for i in range(STEPS):
        rel = ((got[:, i] - ref[:, i]).norm() / ref[:, i].norm()).item()
        ctl = ((ctl_got[:, i] - ctl_ref[:, i]).norm() / ctl_ref[:, i].norm()).item()
        worst, ctl_worst = _row_errors(got, ref)[:, i].max().item(), _row_errors(ctl_got, ctl_ref)[:, i].max().item()
        print(f"{kind} rows {rows} step {i}: ragged rel {rel:.3e} worst row {worst:.3e}; "
              f"control rel {ctl:.3e} worst row {ctl_worst:.3e}")
        assert rel < 2e-2, (i, rel)
        assert ctl < 2e-2, (i, ctl)
    worst, ctl_worst = _row_errors(got, ref).max().item(), _row_errors(ctl_got, ctl_ref).max().item()
    assert worst <= 2 * ctl_worst, (worst, ctl_worst)


def _prefill_step_and_run(m, dec, prompt, tok, n):
    """Prefill ``prompt`` [rows, T], one program step on ``tok`` -> its logits, then ``n`` greedy graph steps
    from the same state -> their tokens (the first of them rewrites the step's cache slot)."""
    T = prompt.shape[1]
    if dec.ragged:
        dec.set_lengths([T] * prompt.shape[0])
    with torch.inference_mode():
        dec.attach()
        try:
            dec.cache.clear()
            m(prompt, skip_softmax=True)
            dec._set_state(tok, dec._row_lengths(T))
            dec.cache.graph_mode = True
            dec.cache.begin_step()
            try:
                logits = dec.program.forward(tok, dec.cache).clone()
            finally:
                dec.cache.graph_mode = False
            toks = dec.run(tok, n).clone()
        finally:
            dec.detach()
    return logits, toks


@pytest.mark.parametrize("kind,rows", [("gpt", 3), ("gpt", 24), ("gemma", 3), ("gemma", 24)])
def test_equal_lengths_through_the_ragged_decoder(kind, rows):
    """GPT: the ragged step runs the uniform step's kernels, so with equal lengths the logits are bitwise the
    uniform decoder's and 20 greedy tokens the same. Gemma's ragged step rotates in a separate pass where the
    uniform one rotates in the QKV epilogue, and no switch of the uniform decoder selects exactly the ragged
    step's kernels (DECODE_EPILOGUES also changes the gate|up kernel and, at 1-4 rows, the QKV GEMV), so its
    logits are held to the project's 2e-2 bound."""
    m = _model(kind)
    prompt, tok = _tokens(rows, 6, 7), _tokens(rows, 1, 8)
    uni = gd.GraphDecoder(m, rows, CAP, 0.0, None)
    rag = gd.GraphDecoder(m, rows, CAP, 0.0, None, ragged=True)
    assert rag.cache.pos_t.shape == rag.cache.len_t.shape == (rows,) and uni.cache.pos_t.shape == (1,)
    lu, tu = _prefill_step_and_run(m, uni, prompt, tok, 20)
    lr, tr = _prefill_step_and_run(m, rag, prompt, tok, 20)
    assert isinstance(rag.graph, torch.cuda.CUDAGraph)
    if kind == "gpt":
        assert torch.equal(lr, lu)
        assert torch.equal(tr, tu)
    else:
        rel = ((lr.float() - lu.float()).norm() / lu.float().norm()).item()
        assert rel < 2e-2, rel
    assert rag.cache.pos_t.tolist() == [26] * rows and rag.cache.len_t.tolist() == [27] * rows


# ------------------------------------------------------------------ end to end
class _EagerGraph:
    """Stands in for a captured graph: replay() runs the decode step eagerly."""

    def __init__(self, dec):
        self.dec = dec

    def replay(self):
        self.dec._step()


def _eager_capture(self, last_tok, cache_len, start=0):
    self._set_state(last_tok, cache_len, start)
    self.graph = _EagerGraph(self)


def _prompts(rows, ragged_lens=True):
    lens = [1 + (5 * b) % 9 for b in range(rows)] if ragged_lens else [6] * rows
    toks = _tokens(rows, 9, 21).tolist()
    return [toks[b][:n] for b, n in enumerate(lens)]


def _shortfalls(m, prompts, contexts):
    """For every generated token: how far the reference logit of the chosen token lies below the row maximum
    (one cache-free forward per row over prompt + generated tokens) -> (worst shortfall, largest row maximum)."""
    worst, top = 0.0, 0.0
    with torch.inference_mode():
        for p, ctx in zip(prompts, contexts):
            acts, _ = m._forward_nocache(torch.tensor([ctx[:-1]], device="cuda"))
            logits = acts[-1][0, len(p) - 1:].float()  # position len - 1 + i decides generated token i
            chosen = torch.tensor(ctx[len(p):], device="cuda")
            mx = logits.amax(-1)
            worst = max(worst, (mx - logits.gather(1, chosen.unsqueeze(1)).squeeze(1)).max().item())
            top = max(top, mx.abs().max().item())
    return worst, top


@pytest.mark.parametrize("kind,rows", [("gpt", 3), ("gpt", 24), ("gemma", 3)])
def test_generate_batch_ragged_end_to_end(monkeypatch, kind, rows):
    m = _model(kind)
    m.__dict__.pop("_graph_decoders", None)
    prompts, block, new = _prompts(rows), 32, 20
    graphed = m.generate_batch(prompts, block, new, temperature=0.0)
    assert [r[:len(p)] for r, p in zip(graphed, prompts)] == prompts and all(len(r) == len(p) + new for r, p in zip(graphed, prompts))
    decs = list(m._graph_decoders.values())
    assert any(d.ragged and d.program is not None and isinstance(d.graph, torch.cuda.CUDAGraph) for d in decs), \
        "no graph captured by a ragged decoder"
    # (b) the chosen tokens against cache-free reference logits; the yardstick is the rectangular call
    rect = _prompts(rows, ragged_lens=False)
    ctl, _ = _shortfalls(m, rect, m.generate_batch(rect, block, new, temperature=0.0))
    got, top = _shortfalls(m, prompts, graphed)
    bf16_step = 2.0 ** (math.floor(math.log2(max(top, 1e-30))) - 7)
    delta = max(2 * ctl, bf16_step)
    print(f"{kind} rows {rows}: ragged shortfall {got:.4g}, rectangular {ctl:.4g}, bf16 step {bf16_step:.4g}")
    assert got <= delta, (got, ctl, bf16_step)
    # (c) seeded sampling
    torch.manual_seed(42)
    s1 = m.generate_batch(prompts, block, new, temperature=1.0, top_k=5)
    torch.manual_seed(42)
    assert m.generate_batch(prompts, block, new, temperature=1.0, top_k=5) == s1
    # (a) graph replay, state reset and the per-row advance: the same call on the eager stand-in
    m.__dict__.pop("_graph_decoders")
    monkeypatch.setattr(gd.GraphDecoder, "_capture", _eager_capture)
    assert m.generate_batch(prompts, block, new, temperature=0.0) == graphed


def test_ragged_falls_back_without_a_decode_program(monkeypatch):
    """PENROZ_DECODE_PROGRAM=0: the rows run one at a time through the one-row path, and no ragged decoder exists."""
    m = _model("gpt")
    m.__dict__.pop("_graph_decoders", None)
    prompts = _prompts(3)
    monkeypatch.setattr(gd, "DECODE_PROGRAM", False)
    out = m.generate_batch(prompts, 32, 6, temperature=0.0)
    assert not any(d.ragged for d in m.__dict__.get("_graph_decoders", {}).values())
    assert out == [m.generate_tokens([p], 32, 6, temperature=0.0) for p in prompts]


def test_the_fallback_is_decided_as_the_decoder_lookup_decides(monkeypatch):
    """``_ragged_fallback`` gives a reason exactly where ``get_decoder`` gives no ragged decoder: with a
    decode program neither does, without the program or without the captured step both do."""
    m = _model("gpt")
    assert m._ragged_fallback() is None and gd.get_decoder(m, 3, 32, 0.0, None, ragged=True) is not None
    monkeypatch.setattr(gd, "DECODE_PROGRAM", False)
    assert "no decode program" in m._ragged_fallback() and gd.get_decoder(m, 3, 32, 0.0, None, ragged=True) is None
    monkeypatch.setattr(gd, "GRAPH_DECODE", False)
    assert "no captured decode step" in m._ragged_fallback() and gd.get_decoder(m, 3, 32, 0.0, None, ragged=True) is None


def test_everything_composed_in_one_ragged_call(monkeypatch):
    monkeypatch.setattr(kvc, "TURBO_QUANT_ENABLED", True)  # the int8 KV cache
    m = _model("gpt")
    m.__dict__.pop("_graph_decoders", None)
    prompts, block, new = _prompts(3), 32, 16
    plain = m.generate_batch(prompts, block, new, temperature=0.0)
    banned = plain[0][len(prompts[0]) + 1]  # a token the unconstrained run does produce
    kw = dict(temperature=0.0, repetition_penalty=1.3, logprobs=2, banned_token_ids=[banned])
    full, infos = m.generate_batch(prompts, block, new, **kw)
    gen = [c[len(p):] for c, p in zip(full, prompts)]
    assert all(len(g) == new and banned not in g for g in gen)
    assert all(len(i["token_logprobs"]) == len(i["top_logprobs"]) == new for i in infos)
    stop = [gen[1][4:6]]
    contexts, infos = m.generate_batch(prompts, block, new, stop=stop, **kw)
    finish_at, which = reference_stop(gen, stop)
    assert finish_at[1] and finish_at[1] <= 6
    assert len(contexts) == len(infos) == 3
    for b, (ctx, info) in enumerate(zip(contexts, infos)):
        keep = finish_at[b] or new
        assert ctx == prompts[b] + gen[b][:keep]  # cut at its own finish, the tokens before it unchanged
        assert info["finish_reason"] == ("stop" if finish_at[b] else "length")
        assert info["stop_sequence"] == (which[b] if finish_at[b] else None)
        assert len(info["token_logprobs"]) == len(info["top_logprobs"]) == keep
        assert all(len(t) == 2 for t in info["top_logprobs"]) and banned not in ctx[len(prompts[b]):]
    dec = next(d for d in m._graph_decoders.values() if d.ragged)
    assert isinstance(dec.cache, gd.StaticTurboKVCache) and isinstance(dec.graph, torch.cuda.CUDAGraph)
    in_prompt = dec.penalties.dense()[0]
    for b, p in enumerate(prompts):  # exactly the row's true prompt tokens: pads add nothing
        assert sorted(in_prompt[b].nonzero().view(-1).tolist()) == sorted(set(p))


def test_ragged_with_int8_weights():
    """One teacher-forced ragged step on the int8 weight copies, on weights the quantiser represents exactly
    (the reference is the bf16 module forward), then a ragged call that asks for them."""
    got, ref, dec = _forced_steps("gpt-lossless", 3, "ragged", steps=1, weight_quant="int8")
    assert dec.weight_quant == "int8"
    rel = ((got - ref).norm() / ref.norm()).item()
    ctl_got, ctl_ref, ctl = _forced_steps("gpt-lossless", 3, "rect", steps=1, weight_quant="int8")
    assert ctl.weight_quant == "int8"
    worst, ctl_worst = _row_errors(got, ref).max().item(), _row_errors(ctl_got, ctl_ref).max().item()
    print(f"int8 weights, 3 rows: ragged rel {rel:.3e} worst row {worst:.3e}; control worst row {ctl_worst:.3e}")
    assert rel < 2e-2, rel
    assert worst <= 2 * ctl_worst, (worst, ctl_worst)
    m = _model("gpt-lossless")
    m.__dict__.pop("_graph_decoders", None)
    prompts = _prompts(3)
    out = m.generate_batch(prompts, 32, 8, temperature=0.0, weight_quant="int8")
    assert any(d.ragged and d.weight_quant == "int8" for d in m._graph_decoders.values())
    assert all(len(r) == len(p) + 8 for r, p in zip(out, prompts))
