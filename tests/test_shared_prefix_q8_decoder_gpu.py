"""``n``, ``share_prefix`` and ``num_beams`` under ``TURBO_QUANT_KV_CACHE=1`` on MI355X: the calls run the shared-prefix
step over int8 caches (``SharedPrefixTurboKVCache``, csrc/kernels/shared_prefix_attn_q8.hip) instead of falling back.
Their decoders' logits, with the tokens forced, stay as close to a cache-free pass as the replicated int8 decoder's on
the same tokens, and the beams are those of the reference search over such logits."""
import math
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode, kv_cache as kvc
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import beam_search as bs

V, BLOCK, NEW, PROMPT = 256, 64, 6, [3, 1, 4, 1, 5, 9, 2, 6, 5]
PROMPTS = [PROMPT + r for r in ([7], [8, 2, 1, 2], [3, 9, 9, 9, 4, 5, 6])]  # a 9-token prefix, remainders 1, 4, 7


@lru_cache(maxsize=None)
def _model(kind):
    if kind == "gpt":  # MHA, head_dim 64
        torch.manual_seed(11)
        m = NeuralNetworkModel("sq8g", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    else:  # Gemma style: RoPE, head_dim 64, 4:1 GQA
        tc = SimpleNamespace(vocab_size=V, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=64,
                             num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                             attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
        torch.manual_seed(5)
        m = NeuralNetworkModel("sq8gg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}}))
    return m.to("cuda").to(dtype=torch.bfloat16).eval()


@pytest.fixture
def served(monkeypatch):
    """The int8 KV cache switched on; -> the decoders that served the test's calls, in order."""
    monkeypatch.setattr(kvc, "TURBO_QUANT_ENABLED", True)
    got, real = [], graph_decode.get_decoder
    monkeypatch.setattr(graph_decode, "get_decoder", lambda *a, **k: got.append(real(*a, **k)) or got[-1])
    return got


def _prompt_logits(m, call):
    """-> (what ``call()`` returned, the logits [rows, T, V] of every pass of the model's modules it made: prompt passes)."""
    got = []
    hook = m.register_forward_hook(lambda mod, args, out: got.append(out[0][-1].float()))
    try:
        return call(), got
    finally:
        hook.remove()


def _forced(dec, toks, lens):
    """The decoder's step logits [rows, T, V] with ``toks`` [rows, T] forced: step t runs eagerly over the decoder's own
    cache, which holds the rows' prompts, at the lengths ``lens`` + t (an int, or [rows]); its own choice is dropped."""
    got, forward = [], dec.program.forward

    def recording(idx, cache):
        last = forward(idx, cache)
        got.append(last.float().reshape(toks.shape[0], -1))
        return last

    dec.program.forward = recording
    try:
        with torch.inference_mode():
            for t in range(toks.shape[1]):
                dec._set_state(toks[:, t:t + 1], lens + t)
                dec._step()
    finally:
        del dec.program.forward
    return torch.stack(got, dim=1)


@pytest.mark.parametrize("share", [False, True], ids=["n", "share_prefix"])
@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_forced_logits_are_as_close_as_the_replicated_int8_decoders(kind, share, served):
    """Row b's logits behind its last prompt token (``share_prefix``: the remainder pass) and behind each of the tokens
    the call sampled, forced through the shared-prefix decoder and through the replicated (``share_prefix``: plain
    ragged) ``StaticTurboKVCache`` decoder. Bound, the bf16 tests' relative one, on whole logit rows: at most twice
    the replicated decoder's deviation from a cache-free pass — both read the same quantised keys."""
    m = _model(kind)
    prompts, extra = (PROMPTS, {"share_prefix": True}) if share else ([PROMPT] * 3, {"n": 3})
    lens, P = [len(p) for p in prompts], len(PROMPT)
    lens_t = torch.tensor(lens, device="cuda") if share else P
    torch.manual_seed(3)
    contexts, first = _prompt_logits(m, lambda: m.generate_batch(PROMPTS if share else PROMPT, BLOCK, NEW, temperature=1.0, top_k=20, **extra))
    dec = served[-1]
    assert type(dec.cache) is graph_decode.SharedPrefixTurboKVCache and dec.graph is not None
    assert m.last_shared_prefix is not None and m.last_shared_prefix["rows"] == 3 and m.last_shared_prefix["prefix_len"] == P
    assert all(c[:n] == p and len(c) == n + NEW for c, p, n in zip(contexts, prompts, lens))
    toks = torch.tensor([c[n:] for c, n in zip(contexts, lens)], device="cuda")
    got = _forced(dec, toks, lens_t)
    _, rep_first = _prompt_logits(m, lambda: m.generate_batch(prompts, BLOCK, NEW, temperature=1.0, top_k=20))
    rep = served[-1]
    assert type(rep.cache) is graph_decode.StaticTurboKVCache and m.last_shared_prefix is None
    got_rep = _forced(rep, toks, lens_t)
    with torch.inference_mode():  # a pass without a cache, from row b's last prompt position on
        want = torch.stack([m._forward_nocache(torch.tensor([c], device="cuda"))[0][-1][0].float()[n - 1:] for c, n in zip(contexts, lens)])
    if share:  # the first tokens' logits: the remainder pass at row b's last position, the padded prompt pass likewise
        got = torch.cat([torch.stack([first[-1][b, n - P - 1] for b, n in enumerate(lens)]).unsqueeze(1), got], dim=1)
        got_rep = torch.cat([torch.stack([rep_first[0][b, n - 1] for b, n in enumerate(lens)]).unsqueeze(1), got_rep], dim=1)
    else:  # (one prompt pass serves every row in both calls)
        want = want[:, 1:]
    dev, dev_rep = (got - want).abs().max().item(), (got_rep - want).abs().max().item()
    print(f"shared_prefix q8 {kind} share={share}: logit deviation {dev:.3e}, replicated int8 decoder {dev_rep:.3e}")
    assert torch.isfinite(got).all() and dev <= 2 * dev_rep, (dev, dev_rep)


@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_beams_are_the_reference_search_over_the_decoders_forced_logits(kind, served):
    """``reference_generate`` fed, for every live hypothesis, the logits of the ``n = W`` int8 shared-prefix decoder
    with that hypothesis forced from the prompt on: a wrong parent, or a scale plane not re-parented with its int8
    plane, gives other logits and another search. Scores: ``tests/test_beam_search_gpu.py``'s bound per step."""
    m, W, new, P = _model(kind), 2, 16, len(PROMPT)
    assert graph_decode.shared_prefix_fallback(m, W, BLOCK) is None
    tokens, info = m.generate_tokens([PROMPT], BLOCK, new, num_beams=W, length_penalty=1.0)
    beams = info["beams"]
    assert m.last_beam_search["path"] == "device" and len(beams) == W and tokens == PROMPT + beams[0]["tokens"]
    assert served[-1].beam == W and type(served[-1].cache) is graph_decode.SharedPrefixTurboKVCache
    _, first = _prompt_logits(m, lambda: m.generate_batch(PROMPT, BLOCK, 2, temperature=1.0, n=W))
    dec = served[-1]  # its prefix cache holds the prompt
    assert not dec.beam and type(dec.cache) is graph_decode.SharedPrefixTurboKVCache

    def next_logits(seqs, parents):
        if not seqs[0]:
            return first[0][:, -1].cpu()
        return _forced(dec, torch.tensor(seqs, device="cuda"), P)[:, -1].cpu()

    ref = bs.reference_generate(next_logits, W, new, None, 1.0)
    assert [(b["tokens"], b["finished"]) for b in beams] == [(b["tokens"], b["finished"]) for b in ref]
    for b, r in zip(beams, ref):
        tol = 4 * abs(r["cum_logprob"]) * 2.0 ** -23 + (math.log2(V) + 20) * 2.0 ** -24
        print(f"beam q8 {kind}: cum {b['cum_logprob']:.6f} reference {r['cum_logprob']:.6f} tol {new * tol:.2e}")
        assert len(b["tokens"]) == new and abs(b["cum_logprob"] - r["cum_logprob"]) <= new * tol, (b, r)
