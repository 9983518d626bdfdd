"""``share_prefix`` on MI355X: the prefill form of csrc/kernels/shared_prefix_attn.hip and the per-row decode form
against the fp64 definitions (ops/shared_prefix.py), with ``prefill_attention`` / ``decode_attention`` on the replicated
cache as the yardstick of bf16 rounding; and ``generate_batch(share_prefix=True)`` end to end."""
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

from test_shared_prefix_gpu import BLOCK, CASES as DECODE_CASES, NEW, PROMPT, _inputs as _decode_inputs, _model, _views as _decode_views

from penroz.ops import attention as attn_ops
from penroz.ops import shared_prefix as sp

#        D    H  Hkv  R  Tq   P   S
CASES = [(64, 2, 2, 2, 1, 1, 1),        # the smallest shape
         (64, 2, 2, 3, 33, 65, 2),      # Tq crosses the 32-row wave tile, P the 64-key tile; an empty tail range
         (64, 12, 12, 4, 70, 300, 4),   # the causal suffix crosses a 64-key tile, the diagonal in the second; several splits
         (256, 4, 1, 2, 40, 97, 3),     # G = 4 packing with pad rows; 32-key tiles; the diagonal across tiles at D = 256
         (128, 8, 1, 2, 17, 70, 2),     # G = 8: 136 packed rows exceed a 128-row tile
         (128, 4, 2, 5, 130, 64, 8)]    # more ranges than key tiles: weight-0 partials; more than 128 query rows per sequence
IDS = lambda c: "-".join(map(str, c))
_bits = lambda t: t.contiguous().view(torch.int16)


def _ulp(ref):
    return 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 7)


@lru_cache(maxsize=None)
def _inputs(D, H, Hkv, R, Tq, P):
    """Random bf16 with a few large-magnitude keys (the running maximum moves); unused cache slots hold NaN.
    -> (qkv rows [R, Tq, ·], prefix K / V, the fp64 reference [R, Tq, H·D]); made once, shared, never written."""
    g = torch.Generator("cuda").manual_seed(D + R + P + Tq)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    qkv = rnd(R, Tq, (H + 2 * Hkv) * D)
    kp, vp = rnd(1, Hkv, P + 5, D), rnd(1, Hkv, P + 5, D)
    kp[:, :, ::37] *= 6
    qkv[:, ::5, H * D:(H + Hkv) * D] *= 6
    kp[:, :, P:], vp[:, :, P:] = float("nan"), float("nan")
    q, k, v = _views(qkv, H, Hkv, D)
    ref = sp.reference_prefill_attention(q, kp, vp, k.transpose(1, 2), v.transpose(1, 2), P).reshape(R, Tq, H * D)
    return qkv, kp, vp, ref


def _views(qkv, H, Hkv, D):
    R, Tq = qkv.shape[:2]
    q, k, v = qkv.split([H * D, Hkv * D, Hkv * D], dim=2)
    return q.view(R, Tq, H, D), k.view(R, Tq, Hkv, D), v.view(R, Tq, Hkv, D)


def _run(case, qkv=None, rows=slice(None)):
    D, H, Hkv, R, Tq, P, S = case
    base, kp, vp, _ = _inputs(*case[:6])
    q, k, v = _views((base if qkv is None else qkv)[rows], H, Hkv, D)
    ks = torch.full((q.shape[0], Hkv, Tq + 3, D), float("nan"), device="cuda", dtype=torch.bfloat16)
    vs = ks.clone()
    out = attn_ops.shared_prefix_prefill_attention(q, k, v, kp, vp, ks, vs, torch.tensor([P], device="cuda"), splits=S)
    return out, ks, vs, k, v


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_prefill_form_matches_the_fp64_definition(case):
    """Bound: twice ``prefill_attention``'s own error on the replicated cache of the same content (P + Tq keys, query
    offset P), plus one bf16 ulp of the output magnitude."""
    D, H, Hkv, R, Tq, P, S = case
    qkv, kp, vp, ref = _inputs(*case[:6])
    out, ks, vs, k, v = _run(case)
    assert torch.equal(_bits(ks[:, :, :Tq]), _bits(k.transpose(1, 2))) and torch.equal(_bits(vs[:, :, :Tq]), _bits(v.transpose(1, 2)))
    assert torch.isnan(ks[:, :, Tq:]).all() and torch.isnan(vs[:, :, Tq:]).all()
    rep_k = torch.cat([kp[:, :, :P].expand(R, -1, -1, -1), ks[:, :, :Tq]], dim=2).contiguous()
    rep_v = torch.cat([vp[:, :, :P].expand(R, -1, -1, -1), vs[:, :, :Tq]], dim=2).contiguous()
    yard = attn_ops.prefill_attention(_views(qkv, H, Hkv, D)[0], rep_k, rep_v, P + Tq)
    err_yard, err = (yard.double() - ref).abs().max().item(), (out.double() - ref).abs().max().item()
    print(f"shared_prefix prefill {case}: err {err:.3e} prefill_attention {err_yard:.3e} ulp {_ulp(ref):.3e}")
    assert torch.isfinite(out).all() and err <= 2 * err_yard + _ulp(ref), (err, err_yard, _ulp(ref))


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=IDS)
def test_prefill_bits_depend_on_the_row_alone(case):
    D, H, Hkv, R, Tq = case[:5]
    a, b = _run(case)[0], _run(case)[0]
    assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(_run(case, rows=slice(0, 2))[0][0]), _bits(a[0]))  # the same row 0 in a 2-row call
    qkv = _inputs(*case[:6])[0].clone()  # row r's last r + 1 positions are pads: refill them
    for r in range(R):
        qkv[r, Tq - 1 - r:] = torch.randn_like(qkv[r, Tq - 1 - r:]) * 3
    c = _run(case, qkv=qkv)[0]
    assert all(torch.equal(_bits(c[r, :Tq - 1 - r]), _bits(a[r, :Tq - 1 - r])) for r in range(R))


@pytest.mark.parametrize("case", [DECODE_CASES[2], DECODE_CASES[3], DECODE_CASES[6]], ids=IDS)
def test_decode_form_with_per_row_lengths(case):
    """Row b holds ``lens[b]`` suffix keys, from 1 (row 0) to the case's own count (the last row); the same bound,
    against ``decode_attention`` on each row's replicated cache."""
    D, H, Hkv, R, P, suffix, S = case
    qkv, kp, vp, ks0, vs0, _ = _decode_inputs(D, H, Hkv, R, P, suffix)
    q, k, v = _decode_views(qkv, H, Hkv, D)
    lens = [1 + b * (suffix - 1) // (R - 1) for b in range(R)]
    ks, vs = ks0.clone(), vs0.clone()
    dev = dict(device="cuda", dtype=torch.long)
    out = attn_ops.shared_prefix_attention(q, k, v, kp, vp, ks, vs, torch.tensor([P], **dev),
                                           P + torch.tensor(lens, **dev), splits=S)
    want_k, want_v = ks0.clone(), vs0.clone()
    for b, n in enumerate(lens):
        want_k[b, :, n - 1], want_v[b, :, n - 1] = k[b], v[b]
    assert torch.equal(_bits(ks), _bits(want_k)) and torch.equal(_bits(vs), _bits(want_v))  # each append in its own slot
    err = err_dec = 0.0
    over = -math.inf  # the largest err_b − ulp_b: what the yardstick's 2·err has to cover
    for b, n in enumerate(lens):
        ref = sp.reference_attention(q[b:b + 1], kp, vp, ks[b:b + 1], vs[b:b + 1], P, n).reshape(1, H * D)
        rep_k = torch.cat([kp[:, :, :P], ks[b:b + 1, :, :n]], dim=2).contiguous()
        rep_v = torch.cat([vp[:, :, :P], vs[b:b + 1, :, :n]], dim=2).contiguous()
        dec = attn_ops.decode_attention(q[b:b + 1].unsqueeze(1), rep_k, rep_v, P + n).view(1, H * D)
        err_b = (out[b:b + 1].double() - ref).abs().max().item()
        err, over = max(err, err_b), max(over, err_b - _ulp(ref))
        err_dec = max(err_dec, (dec.double() - ref).abs().max().item())
    print(f"shared_prefix per-row {case}: err {err:.3e} decode_attention {err_dec:.3e} err - ulp {over:.3e}")
    assert torch.isfinite(out).all() and over <= 2 * err_dec, (err, over, err_dec)
    one, each = (attn_ops.shared_prefix_attention(q, k, v, kp, vp, ks0.clone(), vs0.clone(), torch.tensor([P], **dev), n_t, splits=S)
                 for n_t in (torch.tensor([P + suffix], **dev), torch.full((R,), P + suffix, **dev)))
    assert torch.equal(_bits(one), _bits(each))


# ------------------------------------------------------------------ end to end
PROMPTS = [PROMPT + r for r in ([7], [8, 2], [1, 2, 3], [9, 9, 9, 4], [5, 6])]


def _deviation(m, contexts, infos):
    """The largest |reported token log-probability − teacher-forced one| over the rows (a cache-free pass)."""
    worst = 0.0
    with torch.inference_mode():
        for seq, info, p in zip(contexts, infos, PROMPTS):
            x = torch.tensor([seq], device="cuda")
            logp = torch.log_softmax(m._forward_nocache(x)[0][-1][0].float(), dim=-1)
            want = logp[torch.arange(len(p) - 1, len(seq) - 1), x[0, len(p):]]
            worst = max(worst, (want.cpu() - torch.tensor(info["token_logprobs"])).abs().max().item())
    return worst


@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_rows_report_their_own_logprobs(kind):
    m = _model(kind)
    torch.manual_seed(3)
    contexts, infos = m.generate_batch(PROMPTS, BLOCK, NEW, temperature=1.0, top_k=20, logprobs=0, share_prefix=True)
    assert m.last_shared_prefix is not None and m.last_shared_prefix["rows"] == 5
    assert m.last_shared_prefix["prefix_len"] == len(PROMPT) and m.last_shared_prefix["remainders"] == [1, 2, 3, 4, 2]
    assert all(c[:len(p)] == p and len(c) == len(p) + NEW for c, p in zip(contexts, PROMPTS))
    torch.manual_seed(3)
    plain_contexts, plain_infos = m.generate_batch(PROMPTS, BLOCK, NEW, temperature=1.0, top_k=20, logprobs=0)
    assert m.last_shared_prefix is None
    dev, dev_plain = _deviation(m, contexts, infos), _deviation(m, plain_contexts, plain_infos)
    print(f"share_prefix {kind}: logprob deviation {dev:.3e}, plain ragged call {dev_plain:.3e}")
    assert dev <= 2 * dev_plain, (dev, dev_plain)
