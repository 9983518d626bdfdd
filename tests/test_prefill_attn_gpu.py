"""Prefill attention over the KV cache (csrc/kernels/prefill_attn.hip) against the fp64-input reference:
parity on the tile edges, the running-max paths, the int8 cache, bitwise row independence, routing."""
import math

import pytest
import torch

from penroz.models.kv_cache import KVCache
from penroz.ops import _ext, attention as A, sampling as Sa

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(a, b, atol, rtol=0.0, msg=""):
    err = (a.float() - b.float()).abs().max().item()
    lim = atol + rtol * b.float().abs().max().item()
    print(f"{msg} max err {err:.5g}, limit {lim:.5g}")
    assert err <= lim, f"{msg} max err {err} > {lim}"


def _inputs(B, Tq, off, H, Hkv, D, cap=None, seed=0, knorm=None):
    """q: a strided view into fused QKV rows; bf16 caches [B, Hkv, cap, D] with NaN from slot S on.
    knorm 'grow' / 'shrink': key norms rising / falling 16-fold over the positions."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    S = off + Tq
    cap = S + 37 if cap is None else cap
    qkv = torch.randn(B, Tq, (H + 2 * Hkv) * D, device=DEV, generator=g).bfloat16()
    q = qkv[:, :, :H * D].view(B, Tq, H, D)
    k = torch.randn(B, Hkv, S, D, device=DEV, generator=g)
    if knorm is not None:
        ramp = torch.logspace(-2, 2, S, base=2.0, device=DEV).view(1, 1, S, 1)
        k = k * (ramp if knorm == "grow" else ramp.flip(2))
    v = torch.randn(B, Hkv, S, D, device=DEV, generator=g)
    kc = torch.full((B, Hkv, cap, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, float("nan"))
    kc[:, :, :S], vc[:, :, :S] = k.bfloat16(), v.bfloat16()
    return q, kc, vc, S


def _ref(q, kc, vc, S, off):
    return A.reference_cache_attention(q.double(), kc[:, :, :S].double(), vc[:, :, :S].double(), off)


CASES = [  # B, Tq, off, H, Hkv, D, cap == S
    (1, 16, 0, 2, 2, 64, False), (2, 33, 1, 4, 2, 64, False), (1, 64, 63, 4, 1, 64, False),
    (2, 65, 200, 8, 1, 64, False), (1, 130, 0, 2, 2, 64, True), (2, 130, 77, 4, 1, 64, False),
    (1, 16, 0, 4, 2, 128, False), (2, 33, 1, 8, 1, 128, False), (1, 64, 63, 2, 2, 128, False),
    (1, 65, 200, 4, 1, 128, False), (2, 130, 0, 4, 2, 128, False), (1, 130, 77, 8, 1, 128, False),
    (2, 16, 0, 4, 1, 256, False), (1, 33, 1, 2, 2, 256, False), (2, 64, 63, 8, 1, 256, False),
    (1, 65, 200, 4, 2, 256, False), (1, 130, 0, 4, 1, 256, False), (2, 130, 77, 2, 2, 256, False),
    (1, 130, 77, 8, 1, 256, True), (8, 130, 77, 4, 2, 64, False),  # the last: 128-row tiles
]


@pytest.mark.parametrize("B,Tq,off,H,Hkv,D,full", CASES)
def test_parity(B, Tq, off, H, Hkv, D, full):
    q, kc, vc, S = _inputs(B, Tq, off, H, Hkv, D, cap=off + Tq if full else None)
    out = A.prefill_attention(q, kc, vc, S)
    assert out.shape == (B, Tq, H * D) and out.dtype == torch.bfloat16
    _close(out, _ref(q, kc, vc, S, off), 0.02, 0.01, f"D={D} G={H // Hkv} Tq={Tq}+{off}")


@pytest.mark.parametrize("D,knorm", [(64, "grow"), (256, "grow"), (64, "shrink"), (256, "shrink")])
def test_running_max_paths(D, knorm):
    q, kc, vc, S = _inputs(1, 130, 77, 4, 2, D, knorm=knorm)
    _close(A.prefill_attention(q, kc, vc, S), _ref(q, kc, vc, S, 77), 0.02, 0.01, knorm)


@pytest.mark.parametrize("H,Hkv,D", [(2, 2, 64), (4, 1, 64), (2, 2, 256), (4, 1, 256)])
def test_int8_cache(H, Hkv, D):
    B, Tq, off = 2, 65, 77
    q, kc, vc, S = _inputs(B, Tq, off, H, Hkv, D)
    cap = kc.shape[2]
    kq, vq = (torch.randint(-127, 128, kc.shape, device=DEV, dtype=torch.int8) for _ in range(2))
    ks, vs = (torch.full((B, Hkv, cap), float("nan"), device=DEV) for _ in range(2))
    Sa.kv_quantize_into(kc[:, :, :S].transpose(1, 2), kq, ks, 0)
    Sa.kv_quantize_into(vc[:, :, :S].transpose(1, 2), vq, vs, 0)
    out = A.prefill_attention(q, kq, vq, S, ks, vs)
    ref = A.reference_cache_attention(q.double(), kq[:, :, :S].double() * ks[:, :, :S, None].double(),
                                      vq[:, :, :S].double() * vs[:, :, :S, None].double(), off)
    _close(out, ref, 0.02, 0.01, f"int8 D={D} G={H // Hkv}")


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (4, 1, 256)])
def test_rows_independent_bitwise(H, Hkv, D):
    q, kc, vc, S = _inputs(2, 130, 77, H, Hkv, D)
    out = A.prefill_attention(q, kc, vc, S)
    assert torch.equal(out, A.prefill_attention(q, kc, vc, S))
    assert torch.equal(out[:, :33], A.prefill_attention(q[:, :33], kc, vc, 77 + 33))
    assert torch.equal(out[1:], A.prefill_attention(q[1:], kc[1:].contiguous(), vc[1:].contiguous(), S))


def test_routing():
    q, kc, vc, S = _inputs(1, 40, 8, 4, 4, 64)
    assert torch.equal(A.decode_attention(q, kc, vc, S), A.prefill_attention(q, kc, vc, S))
    q5 = q[:, :5].contiguous()
    dec = _ext.kernels().decode_attn(q5, kc, vc, None, None, 13, 8, 1.0 / math.sqrt(64), None, None, None,
                                     A.decode_counters(q.device), None, None)
    assert torch.equal(A.decode_attention(q5, kc, vc, 13), dec)


def test_kv_cache_attend_in_two_chunks():
    H, D, T0, T1 = 4, 64, 48, 40
    g = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(1, T0 + T1, 3 * H * D, device=DEV, generator=g).bfloat16()
    q, k, v = (t.view(1, T0 + T1, H, D) for t in qkv.split(H * D, dim=2))
    cache = KVCache(1, capacity=128)
    out = torch.cat([cache.attend(0, q[:, :T0], k[:, :T0], v[:, :T0]), cache.attend(0, q[:, T0:], k[:, T0:], v[:, T0:])], 1)
    ref = A.reference_cache_attention(q.double(), k.transpose(1, 2).double(), v.transpose(1, 2).double(), 0)
    _close(out, ref, 0.02, 0.01, "two chunks")
