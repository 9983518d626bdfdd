"""The int8 shared-prefix references (ops/shared_prefix.py) against dequantise-then-the-existing-reference, and the
fallback functions' reasons when the kernels' plans refuse."""
import pytest
import torch

from penroz.models import graph_decode, kv_cache as kvc
from penroz.ops import attention as attn_ops
from penroz.ops import shared_prefix as sp
from penroz.ops.sampling import reference_quantize


def _cache(g, rows, Hkv, cap, D):
    return torch.randint(-127, 128, (rows, Hkv, cap, D), generator=g, dtype=torch.int8), torch.rand(rows, Hkv, cap, generator=g) / 64


def _deq(x, s):
    return x.double() * s.double()[..., None]


def test_q8_references_are_the_existing_ones_on_dequantised_caches():
    g = torch.Generator().manual_seed(0)
    R, H, Hkv, D, P, n, Tq = 3, 4, 2, 16, 5, 4, 3
    (kp, kps), (vp, vps) = _cache(g, 1, Hkv, P + 2, D), _cache(g, 1, Hkv, P + 2, D)
    (ks, kss), (vs, vss) = _cache(g, R, Hkv, n + 2, D), _cache(g, R, Hkv, n + 2, D)
    q, k, v = (torch.randn(R, h, D, generator=g).bfloat16() for h in (H, Hkv, Hkv))
    out, (qk, sk, qv, sv) = sp.reference_attention_q8(q, k, v, (kp, vp, kps, vps), (ks, vs, kss, vss), P, n)
    wq, ws = reference_quantize(k.float())
    assert torch.equal(qk, wq) and torch.equal(sk, ws.squeeze(-1))
    ksd, vsd = _deq(ks, kss), _deq(vs, vss)
    ksd[:, :, n - 1], vsd[:, :, n - 1] = _deq(qk, sk), _deq(qv, sv)
    assert torch.equal(out, sp.reference_attention(q, _deq(kp, kps), _deq(vp, vps), ksd, vsd, P, n))
    q, k, v = (torch.randn(R, Tq, h, D, generator=g).bfloat16() for h in (H, Hkv, Hkv))
    out, (qk, sk, qv, sv) = sp.reference_prefill_attention_q8(q, k, v, (kp, vp, kps, vps), (ks, vs, kss, vss), P)
    wq, ws = reference_quantize(v.float().transpose(1, 2))
    assert torch.equal(qv, wq) and torch.equal(sv, ws.squeeze(-1))
    assert torch.equal(out, sp.reference_prefill_attention(q, _deq(kp, kps), _deq(vp, vps), _deq(qk, sk), _deq(qv, sv), P))
    # the CPU form of the op writes the slots the reference names
    suffix = (ks.clone(), vs.clone(), kss.clone(), vss.clone())
    got = attn_ops.shared_prefix_prefill_attention_q8(q, k, v, (kp, vp, kps, vps), suffix, torch.tensor([P]))
    assert got.shape == (R, Tq, H * D) and torch.equal(suffix[0][:, :, :Tq], qk) and torch.equal(suffix[3][:, :, :Tq], sv)


@pytest.mark.parametrize("turbo", [False, True])
def test_fallbacks_still_name_a_refusing_plan(turbo, monkeypatch):
    monkeypatch.setattr(kvc, "TURBO_QUANT_ENABLED", turbo)
    monkeypatch.setattr(graph_decode, "applicable", lambda model: True)
    monkeypatch.setattr(graph_decode, "ragged_program_ok", lambda model: True)
    monkeypatch.setattr(graph_decode, "_attention_shapes", lambda model: [(4, 2, 64)])
    asked = []
    decode, prefill = ("shared_prefix_q8_applies", "shared_prefix_prefill_q8_applies") if turbo else \
        ("shared_prefix_applies", "shared_prefix_prefill_applies")
    monkeypatch.setattr(attn_ops, decode, lambda *a: asked.append(decode) or False)
    assert "refuses 3 rows" in graph_decode.shared_prefix_fallback(None, 3, 64)
    monkeypatch.setattr(attn_ops, decode, lambda *a: True)
    monkeypatch.setattr(attn_ops, prefill, lambda *a: asked.append(prefill) or False)
    assert graph_decode.shared_prefix_fallback(None, 3, 64) is None
    assert "refuses 3 rows of 5 positions" in graph_decode.share_prefix_fallback(None, 3, 64, 5, 64)
    assert asked == [decode, prefill]
