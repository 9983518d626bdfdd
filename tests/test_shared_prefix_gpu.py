"""``n`` samples of one prompt on MI355X: csrc/kernels/shared_prefix_attn.hip against the fp64 definition
(ops/shared_prefix.py) with ``decode_attention`` on the replicated cache as the yardstick of bf16 rounding, its
reproducibility and row independence, and ``generate_batch(n=...)`` end to end on the shared-prefix step."""
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
from penroz.ops import attention as attn_ops
from penroz.ops import shared_prefix as sp

#        D    H  Hkv  R   P  suffix S
CASES = [(64, 2, 2, 2, 1, 1, 1),        # the smallest case
         (64, 2, 2, 33, 65, 1, 2),      # the 32-row MFMA tile, the 64-key tile, an empty-tail range
         (64, 12, 12, 64, 300, 257, 4),  # the 256-key suffix chunk, several splits
         (256, 4, 1, 5, 97, 3, 3),      # G = 4 packing with pad rows, the 32-key tile
         (128, 4, 2, 9, 64, 2, 8),      # more ranges than 64-key tiles: weight-0 partials
         (256, 4, 1, 40, 97, 70, 3),    # 128-row tiles, two per KV head, four Q waves at D = 256; a second suffix chunk
         (128, 8, 1, 3, 70, 130, 2)]    # G = 8; a second suffix chunk with two threads per key


@lru_cache(maxsize=None)
def _inputs(D, H, Hkv, R, P, suffix):
    """Random bf16 with a few large-magnitude keys (the running maximum moves); unused cache slots hold NaN.
    -> (qkv rows, prefix K / V, suffix K / V before the step, the fp64 reference [R, H·D]); made once, shared."""
    g = torch.Generator("cuda").manual_seed(D + R + P)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    qkv = rnd(R, (H + 2 * Hkv) * D)
    kp, vp = rnd(1, Hkv, P + 5, D), rnd(1, Hkv, P + 5, D)
    ks, vs = rnd(R, Hkv, suffix + 3, D), rnd(R, Hkv, suffix + 3, D)
    kp[:, :, ::37] *= 6
    ks[:, :, ::5] *= 6
    for t, n in ((kp, P), (vp, P), (ks, suffix - 1), (vs, suffix - 1)):
        t[:, :, n:] = float("nan")
    q, k, v = _views(qkv, H, Hkv, D)
    ks_ref, vs_ref = ks.clone(), vs.clone()
    ks_ref[:, :, suffix - 1], vs_ref[:, :, suffix - 1] = k, v
    ref = sp.reference_attention(q, kp, vp, ks_ref, vs_ref, P, suffix).reshape(R, H * D)
    return qkv, kp, vp, ks, vs, ref


def _views(qkv, H, Hkv, D):
    R = qkv.shape[0]
    q, k, v = qkv.split([H * D, Hkv * D, Hkv * D], dim=1)
    return q.view(R, H, D), k.view(R, Hkv, D), v.view(R, Hkv, D)


def _run(case, rows=None):
    D, H, Hkv, R, P, suffix, S = case
    qkv, kp, vp, ks, vs, _ = _inputs(D, H, Hkv, R, P, suffix)
    rows = slice(None) if rows is None else rows
    ks, vs = ks[rows].clone(), vs[rows].clone()
    q, k, v = _views(qkv[rows], H, Hkv, D)
    dev = dict(device="cuda", dtype=torch.long)
    out = attn_ops.shared_prefix_attention(q, k, v, kp, vp, ks, vs, torch.tensor([P], **dev),
                                           torch.tensor([P + suffix], **dev), splits=S)
    return out, ks, vs, k, v


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_kernel_matches_the_fp64_definition(case):
    """Bound: twice ``decode_attention``'s own error on the replicated cache of the same content, plus one bf16
    ulp of the output magnitude (another summation order may round the final bf16 the other way once)."""
    D, H, Hkv, R, P, suffix, S = case
    qkv, kp, vp, ks0, vs0, ref = _inputs(D, H, Hkv, R, P, suffix)
    out, ks, vs, k, v = _run(case)
    assert torch.equal(ks[:, :, suffix - 1].view(torch.int16), k.view(torch.int16))
    assert torch.equal(vs[:, :, suffix - 1].view(torch.int16), v.view(torch.int16))
    assert torch.equal(ks[:, :, :suffix - 1].view(torch.int16), ks0[:, :, :suffix - 1].view(torch.int16))
    rep_k = torch.cat([kp[:, :, :P].expand(R, -1, -1, -1), ks[:, :, :suffix]], dim=2).contiguous()
    rep_v = torch.cat([vp[:, :, :P].expand(R, -1, -1, -1), vs[:, :, :suffix]], dim=2).contiguous()
    q = _views(qkv, H, Hkv, D)[0]
    dec = attn_ops.decode_attention(q.unsqueeze(1), rep_k, rep_v, P + suffix).view(R, H * D)
    err_dec = (dec.double() - ref).abs().max().item()
    err = (out.double() - ref).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 7)
    print(f"shared_prefix {case}: err {err:.3e} decode_attention {err_dec:.3e} ulp {ulp:.3e}")
    assert torch.isfinite(out).all() and err <= 2 * err_dec + ulp, (err, err_dec, ulp)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=lambda c: "-".join(map(str, c)))
def test_bits_are_reproducible_and_independent_of_the_other_rows(case):
    a, b = _run(case)[0], _run(case)[0]
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    two = _run(case, rows=slice(0, 2))[0]  # the same row 0 in a 2-row call
    assert torch.equal(two[0].view(torch.int16), a[0].view(torch.int16))


# ------------------------------------------------------------------ end to end
V, BLOCK, NEW, PROMPT = 256, 64, 6, [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]


@lru_cache(maxsize=None)
def _model(kind):
    if kind == "gpt":  # MHA, head_dim 64
        torch.manual_seed(11)
        m = NeuralNetworkModel("spg", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    else:  # Gemma style: RoPE, head_dim 256, 4:1 GQA
        tc = SimpleNamespace(vocab_size=V, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=256,
                             num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                             attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
        torch.manual_seed(5)
        m = NeuralNetworkModel("spgg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}}))
    return m.to("cuda").to(dtype=torch.bfloat16).eval()


def _deviation(m, contexts, infos):
    """The largest |reported token log-probability − teacher-forced one| over the rows: a cache-free pass of the
    model's modules over each row's full sequence, fp32 log_softmax, gather."""
    worst = 0.0
    with torch.inference_mode():
        for seq, info in zip(contexts, infos):
            x = torch.tensor([seq], device="cuda")
            logp = torch.log_softmax(m._forward_nocache(x)[0][-1][0].float(), dim=-1)
            want = logp[torch.arange(len(PROMPT) - 1, len(seq) - 1), x[0, len(PROMPT):]]
            worst = max(worst, (want.cpu() - torch.tensor(info["token_logprobs"])).abs().max().item())
    return worst


@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_sampled_rows_report_their_own_logprobs(kind):
    m = _model(kind)
    torch.manual_seed(3)
    contexts, infos = m.generate_batch(PROMPT, BLOCK, NEW, temperature=1.0, top_k=20, n=5, logprobs=0)
    assert m.last_shared_prefix is not None and m.last_shared_prefix["rows"] == 5
    assert m.last_shared_prefix["prefix_len"] == len(PROMPT)
    assert len(contexts) == 5 and all(c[:len(PROMPT)] == PROMPT and len(c) == len(PROMPT) + NEW for c in contexts)
    assert len({tuple(c) for c in contexts}) > 1
    torch.manual_seed(3)
    rep_contexts, rep_infos = m.generate_batch([PROMPT] * 5, BLOCK, NEW, temperature=1.0, top_k=20, logprobs=0)
    assert m.last_shared_prefix is None
    dev, dev_rep = _deviation(m, contexts, infos), _deviation(m, rep_contexts, rep_infos)
    print(f"shared_prefix {kind}: logprob deviation {dev:.3e}, replicated call {dev_rep:.3e}")
    assert dev <= 2 * dev_rep, (dev, dev_rep)


@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_greedy_rows_are_the_one_row_call(kind):
    m = _model(kind)
    one = m.generate_tokens([PROMPT], BLOCK, NEW, temperature=0.0)
    assert m.generate_batch([PROMPT] * 4, BLOCK, NEW, temperature=0.0) == [one] * 4  # (the seed's precondition)
    assert m.generate_batch([PROMPT], BLOCK, NEW, temperature=0.0, n=4) == [one] * 4
    assert m.last_shared_prefix["rows"] == 4
