"""Shared-prefix attention over the int8 KV cache on MI355X: csrc/kernels/shared_prefix_attn_q8.hip against the fp64
definition on the same quantised operands (ops/shared_prefix.py), with ``decode_attention`` / ``prefill_attention``
on the replicated int8 cache as the yardstick of rounding — the bound ``tests/test_shared_prefix_gpu.py`` holds the
bf16 kernel to — and the appended slots against ``kv_quantize``."""
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

from penroz.ops import _ext
from penroz.ops import attention as attn_ops
from penroz.ops import sampling as samp_ops
from penroz.ops import shared_prefix as sp

HEADS = [(64, 1), (128, 4), (256, 8)]  # (D, G); two KV heads each
HKV = 2
_i32 = lambda t: t.contiguous().view(torch.int32)
_i16 = lambda t: t.contiguous().view(torch.int16)
_dev = dict(device="cuda", dtype=torch.long)


def _ulp(ref):
    return 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 7)


def _cache(g, rows, cap, D, used):
    """A random int8 cache [rows, HKV, cap, D] whose scales vary by token (x 2^(t mod 5)): a misapplied or misindexed
    scale cannot cancel. Slots from ``used`` on hold NaN scales: reading one poisons the output."""
    x = torch.randint(-127, 128, (rows, HKV, cap, D), device="cuda", generator=g, dtype=torch.int8)
    s = (0.5 + torch.rand(rows, HKV, cap, device="cuda", generator=g)) / 508 * 2.0 ** (torch.arange(cap, device="cuda") % 5)
    s[:, :, used:] = float("nan")
    return x, s.float()


def _kv_quantize(x):
    """x [R, T, HKV, D] bf16 -> (int8 [R, HKV, T, D], fp32 [R, HKV, T]) by the cache's own kernel."""
    R, T, _, D = x.shape
    q, s = torch.empty(R, HKV, T, D, device="cuda", dtype=torch.int8), torch.empty(R, HKV, T, device="cuda")
    samp_ops.kv_quantize_into(x, q, s, 0)
    return q, s


# (R, P, suffix chunks beyond one key, S, per-row lengths): R 3 = a pad wave, 33 crosses the 32-row wave; P at the
# 64-key tile's edges; 130 with S = 4 leaves the last range empty (checked below); suffix 1 and one past the chunk
DECODE = [(3, 1, 0, 1, False), (33, 63, 1, 2, False), (3, 65, 0, 2, False), (33, 130, 0, 4, False), (33, 65, 1, 2, True)]


@lru_cache(maxsize=None)
def _decode_inputs(D, G, R, P, suffix):
    g = torch.Generator("cuda").manual_seed(D + R + P + suffix)
    qkv = torch.randn(R, (G + 2) * HKV * D, device="cuda", generator=g).bfloat16()
    return (qkv, *(_cache(g, 1, P + 5, D, P) for _ in "kv"), *(_cache(g, R, suffix + 3, D, suffix - 1) for _ in "kv"))


def _decode(D, G, R, P, suffix, S, lens, rows=slice(None)):
    """-> (out, q, k, v, prefix, suffix caches after the launch, suffix caches before it) for ``rows`` of the case."""
    qkv, (kp, kps), (vp, vps), (ks0, kss0), (vs0, vss0) = _decode_inputs(D, G, R, P, suffix)
    qkv = qkv[rows]
    q, k, v = (t.view(qkv.shape[0], -1, D) for t in qkv.split([G * HKV * D, HKV * D, HKV * D], dim=1))
    before = tuple(t[rows].clone() for t in (ks0, vs0, kss0, vss0))
    after = tuple(t.clone() for t in before)
    pre = (kp, vp, kps, vps)
    out = attn_ops.shared_prefix_attention_q8(q, k, v, pre, after, torch.tensor([P], **_dev),
                                              P + torch.tensor(lens, **_dev)[rows], splits=S)
    return out, q, k, v, pre, after, before


@pytest.mark.parametrize("case", DECODE, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("D,G", HEADS)
def test_decode_form_matches_the_fp64_definition(D, G, case):
    """Bound: twice ``decode_attention``'s own error on the replicated int8 cache of the same content, plus one bf16
    ulp of the output magnitude — the bf16 kernel's bound. The appended slot is ``kv_quantize``'s bits; every other
    slot is untouched."""
    R, P, chunks, S, per_row = case
    suffix = 1 + chunks * 16384 // D
    lens = [1 + b * (suffix - 1) // (R - 1) for b in range(R)] if per_row else [suffix] * R
    if P == 130:
        assert _ext.kernels().shared_prefix_q8_plan(R, G * HKV, HKV, D, P + 5, S)[3] == S
        assert _ext.kernels().shared_prefix_ranges(P, S)[-1][0] > P  # the last range starts beyond P: a weight-0 partial
    out, q, k, v, pre, (ks, vs, kss, vss), before = _decode(D, G, R, P, suffix, S, lens)
    (qk, sk), (qv, sv) = _kv_quantize(k.unsqueeze(1)), _kv_quantize(v.unsqueeze(1))
    want = [t.clone() for t in before]
    for b, n in enumerate(lens):
        want[0][b, :, n - 1], want[1][b, :, n - 1], want[2][b, :, n - 1], want[3][b, :, n - 1] = qk[b, :, 0], qv[b, :, 0], sk[b, :, 0], sv[b, :, 0]
    assert torch.equal(ks, want[0]) and torch.equal(vs, want[1])
    assert torch.equal(_i32(kss), _i32(want[2])) and torch.equal(_i32(vss), _i32(want[3]))
    ref, dec = [], []
    for b, n in enumerate(lens):
        one = slice(b, b + 1)
        r = sp.reference_attention_q8(q[one], k[one], v[one], pre, tuple(t[one] for t in before), P, n)[0]
        ref.append(r.reshape(1, -1))
        rep = [torch.cat([p[:, :, :P], s[one, :, :n]], dim=2).contiguous() for p, s in zip(pre, (ks, vs, kss, vss))]
        dec.append(attn_ops.decode_attention(q[one].unsqueeze(1), rep[0], rep[1], P + n, rep[2], rep[3]).view(1, -1))
    ref, dec = torch.cat(ref), torch.cat(dec)
    err, err_dec = (out.double() - ref).abs().max().item(), (dec.double() - ref).abs().max().item()
    print(f"shared_prefix q8 D={D} G={G} {case}: err {err:.3e} decode_attention {err_dec:.3e} ulp {_ulp(ref):.3e}")
    assert torch.isfinite(out).all() and err <= 2 * err_dec + _ulp(ref), (err, err_dec, _ulp(ref))


@pytest.mark.parametrize("D,G", HEADS)
def test_a_row_has_the_same_bits_among_3_rows_and_among_33(D, G):
    R, P, chunks, S, _ = DECODE[1]
    suffix = 1 + chunks * 16384 // D
    many = _decode(D, G, R, P, suffix, S, [suffix] * R)[0]
    few = _decode(D, G, R, P, suffix, S, [suffix] * R, rows=slice(0, 3))[0]
    assert torch.equal(_i16(few), _i16(many[:3]))
    assert torch.equal(_i16(many), _i16(_decode(D, G, R, P, suffix, S, [suffix] * R)[0]))  # and reproducible


@lru_cache(maxsize=None)
def _prefill_inputs(D, G, Tq, P):
    """R = 3 rows of Tq positions: (qkv rows, prefix K and V caches, suffix K and V caches before the launch)."""
    g = torch.Generator("cuda").manual_seed(D + Tq + P)
    qkv = torch.randn(3, Tq, (G + 2) * HKV * D, device="cuda", generator=g).bfloat16()
    qkv[:, ::5, G * HKV * D:(G + 1) * HKV * D] *= 6  # a few large keys: the running maximum moves
    return (qkv, *(_cache(g, 1, P + 5, D, P) for _ in "kv"), *(_cache(g, 3, Tq + 3, D, 0) for _ in "kv"))


def _prefill(D, G, Tq, P, S, qkv=None):
    """-> (out, q, k, v, prefix caches, suffix caches after the launch, suffix K / V before it)."""
    base, (kp, kps), (vp, vps), (ks0, kss0), (vs0, vss0) = _prefill_inputs(D, G, Tq, P)
    qkv = base if qkv is None else qkv
    q, k, v = (t.view(3, Tq, -1, D) for t in qkv.split([G * HKV * D, HKV * D, HKV * D], dim=2))
    pre, suf = (kp, vp, kps, vps), tuple(t.clone() for t in (ks0, vs0, kss0, vss0))
    out = attn_ops.shared_prefix_prefill_attention_q8(q, k, v, pre, suf, torch.tensor([P], **_dev), splits=S)
    return out, q, k, v, pre, suf, (ks0, vs0)


@pytest.mark.parametrize("Tq,P,S", [(1, 1, 1), (33, 65, 2)])
@pytest.mark.parametrize("D,G", HEADS)
def test_prefill_form_matches_the_fp64_definition(D, G, Tq, P, S):
    """R = 3 rows of Tq positions. Bound: twice ``prefill_attention``'s own error on the replicated int8 cache of the
    same content plus one bf16 ulp (the bf16 prefill form's bound); suffix slots 0..Tq-1 are ``kv_quantize``'s bits."""
    R = 3
    out, q, k, v, pre, (ks, vs, kss, vss), before = _prefill(D, G, Tq, P, S)
    (qk, sk), (qv, sv) = _kv_quantize(k), _kv_quantize(v)
    assert torch.equal(ks[:, :, :Tq], qk) and torch.equal(vs[:, :, :Tq], qv)
    assert torch.equal(_i32(kss[:, :, :Tq]), _i32(sk)) and torch.equal(_i32(vss[:, :, :Tq]), _i32(sv))
    assert torch.equal(ks[:, :, Tq:], before[0][:, :, Tq:]) and torch.equal(vs[:, :, Tq:], before[1][:, :, Tq:])
    assert torch.isnan(kss[:, :, Tq:]).all() and torch.isnan(vss[:, :, Tq:]).all()
    ref = sp.reference_prefill_attention_q8(q, k, v, pre, (ks, vs, kss, vss), P)[0].reshape(R, Tq, -1)
    rep = [torch.cat([p[:, :, :P].expand(R, *p.shape[1:2], P, *p.shape[3:]), s[:, :, :Tq]], dim=2).contiguous()
           for p, s in zip(pre, (ks, vs, kss, vss))]
    yard = attn_ops.prefill_attention(q, rep[0], rep[1], P + Tq, rep[2], rep[3])
    err, err_yard = (out.double() - ref).abs().max().item(), (yard.double() - ref).abs().max().item()
    print(f"shared_prefix q8 prefill D={D} G={G} Tq={Tq} P={P}: err {err:.3e} prefill_attention {err_yard:.3e} ulp {_ulp(ref):.3e}")
    assert torch.isfinite(out).all() and err <= 2 * err_yard + _ulp(ref), (err, err_yard, _ulp(ref))


@pytest.mark.parametrize("P,S", [(1, 1), (65, 2)])
@pytest.mark.parametrize("D,G", HEADS)
def test_prefill_pads_change_no_real_position(D, G, P, S):
    """Ragged remainders: row r holds 32 - r real positions of Tq = 33, the rest are pads. Refilled with other values
    of three times the magnitude (other absmax, other scales), the pads change neither the real positions' output bits
    nor their suffix slots, which stay ``kv_quantize``'s bits of the rows' own K/V (the test above)."""
    Tq = 33
    a, _, _, _, _, suf_a, _ = _prefill(D, G, Tq, P, S)
    qkv = _prefill_inputs(D, G, Tq, P)[0].clone()
    for r in range(3):
        qkv[r, Tq - 1 - r:] = torch.randn_like(qkv[r, Tq - 1 - r:]) * 3
    c, _, _, _, _, suf_c, _ = _prefill(D, G, Tq, P, S, qkv=qkv)
    for r in range(3):
        n = Tq - 1 - r
        assert torch.equal(_i16(c[r, :n]), _i16(a[r, :n])) and not torch.equal(_i16(c[r, n:]), _i16(a[r, n:]))
        assert all(torch.equal(x[r, :, :n], y[r, :, :n]) for x, y in zip(suf_c[:2], suf_a[:2]))
        assert all(torch.equal(_i32(x[r, :, :n]), _i32(y[r, :, :n])) for x, y in zip(suf_c[2:], suf_a[2:]))
