"""The per-row forms a ragged decode step is made of (ops/ragged.py), kernel by kernel on MI355X: decode
attention with one cache length per batch row (``seq_len_dev`` [B]) — split counts that differ between the
rows of one launch, the in-launch merge, the combine launch, the small kernel, the int8 cache, the fused
append — and per-row positions in the embedding kernels and the RoPE table. The caches hold NaN at and
beyond each row's own length: a key read from there shows in the output."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

from penroz.ops import _ext, attention as A, fused as Fu, gemm as G, rope as Ro, sampling as Sa

DEV = "cuda"


def _close(a, b, atol, rtol=0.0, msg=""):
    err = (a.float() - b.float()).abs().max().item()
    lim = atol + rtol * b.float().abs().max().item()
    assert err <= lim, f"{msg} max err {err} > {lim}"


def _lens64():
    return [1 + (37 * b) % 600 for b in range(64)]


def _caches(B, Hkv, cap, D, lens, dtype=torch.bfloat16):
    kc = torch.randn(B, Hkv, cap, D, device=DEV).to(dtype)
    vc = torch.randn(B, Hkv, cap, D, device=DEV).to(dtype)
    for b, n in enumerate(lens):
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("nan")
    return kc, vc


def _per_row_reference(q, kc, vc, lens):
    return torch.cat([A.reference_cache_attention(q[b:b + 1].float(), kc[b:b + 1, :, :n].float(),
                                                  vc[b:b + 1, :, :n].float(), n - 1) for b, n in enumerate(lens)])


# (B, H, Hkv, D, lens, cap, merge, small): rows of one launch on both sides of every boundary — one key, the
# 256-key chunk and split size (255 / 256 / 257), several splits; ``merge`` False: no arrival counters
CASES = [
    pytest.param(3, 4, 4, 64, [1, 257, 1000], 1100, True, False, id="merge-different-split-counts"),
    pytest.param(3, 4, 4, 64, [1, 257, 1000], 1100, False, False, id="combine-launch"),
    pytest.param(5, 8, 2, 128, [1, 40, 255, 256, 300], 1100, True, False, id="gqa4-general"),
    pytest.param(5, 8, 2, 128, [1, 40, 255, 256, 300], 320, True, True, id="gqa4-small"),
    pytest.param(2, 4, 1, 256, [3, 700], 1024, True, True, id="small-kernel-d256"),
    pytest.param(64, 12, 12, 64, _lens64(), 640, True, False, id="64-rows"),
]


@pytest.mark.parametrize("B,H,Hkv,D,lens,cap,merge,small", CASES)
def test_decode_attention_with_per_row_lengths(monkeypatch, B, H, Hkv, D, lens, cap, merge, small):
    torch.manual_seed(B + D)
    if not merge:
        monkeypatch.setenv("PENROZ_DECODE_MERGE", "0")
    cnt = A.decode_counters(torch.device(DEV))
    assert (cnt is not None) == merge
    plan = _ext.kernels().decode_attn_plan(B, 1, H, Hkv, D, cap, True, cnt.numel() if merge else 0)
    assert plan[0] == small, plan
    if len(lens) == 3:
        assert plan[1] > 1 and plan[3] == merge, plan  # several splits; merged in the launch, or by the combine launch
    q = torch.randn(B, 1, H, D, device=DEV).to(torch.bfloat16)
    kc, vc = _caches(B, Hkv, cap, D, lens)
    sl = torch.tensor(lens, device=DEV)
    out = A.decode_attention(q, kc, vc, cap, seq_len_dev=sl)
    assert torch.isfinite(out.float()).all(), "a key at or beyond a row's own length was read"
    _close(out, _per_row_reference(q, kc, vc, lens), 0.02, 0.01)
    if merge and not small:
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0


def test_decode_attention_with_per_row_lengths_int8():
    torch.manual_seed(5)
    B, H, D, cap, lens = 3, 4, 64, 1100, [1, 257, 1000]
    q = torch.randn(B, 1, H, D, device=DEV).to(torch.bfloat16)
    k = torch.randn(B, cap, H, D, device=DEV).to(torch.bfloat16)
    v = torch.randn(B, cap, H, D, device=DEV).to(torch.bfloat16)
    kq, vq = (torch.empty(B, H, cap, D, dtype=torch.int8, device=DEV) for _ in range(2))
    ks, vs = torch.ones(B, H, cap, device=DEV), torch.ones(B, H, cap, device=DEV)
    Sa.kv_quantize_into(k, kq, ks, 0)
    Sa.kv_quantize_into(v, vq, vs, 0)
    for b, n in enumerate(lens):  # a scale read from beyond a row's length shows
        ks[b, :, n:] = float("nan")
        vs[b, :, n:] = float("nan")
    out = A.decode_attention(q, kq, vq, cap, ks, vs, seq_len_dev=torch.tensor(lens, device=DEV))
    ref = _per_row_reference(q, k.transpose(1, 2), v.transpose(1, 2), lens)
    _close(out, ref, 0.05, 0.02)  # (test_decode_attention_int8's tolerance: the cache is quantised)


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("B,H,Hkv,D,lens,cap", [(3, 4, 4, 64, [1, 257, 1000], 1100), (5, 8, 2, 128, [1, 40, 255, 256, 300], 320),
                                                (2, 4, 1, 256, [3, 700], 1024)])
def test_fused_append_with_per_row_lengths(int8, B, H, Hkv, D, lens, cap):
    """Output and cache contents equal per-row kv_append (``pos_dev`` [B]) followed by attention, and
    nothing outside slot ``len_b - 1`` of each row is written."""
    torch.manual_seed(D + cap)
    rows = torch.randn(B, 1, (H + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    q = rows[:, :, :H * D].view(B, 1, H, D)
    k = rows[:, :, H * D:(H + Hkv) * D].view(B, 1, Hkv, D)
    v = rows[:, :, (H + Hkv) * D:].view(B, 1, Hkv, D)
    sl = torch.tensor(lens, device=DEV)
    pos = sl - 1
    if int8:
        kc = torch.randint(-128, 127, (B, Hkv, cap, D), device=DEV, dtype=torch.int8)
        vc = torch.randint(-128, 127, (B, Hkv, cap, D), device=DEV, dtype=torch.int8)
        ks, vs = torch.rand(B, Hkv, cap, device=DEV) * 0.02, torch.rand(B, Hkv, cap, device=DEV) * 0.02
    else:
        kc = torch.randn(B, Hkv, cap, D, device=DEV).to(torch.bfloat16)
        vc = torch.randn(B, Hkv, cap, D, device=DEV).to(torch.bfloat16)
        ks = vs = None
    before = [t.clone() if t is not None else None for t in (kc, vc, ks, vs)]
    c1 = [t.clone() if t is not None else None for t in before]
    c2 = [t.clone() if t is not None else None for t in before]
    _ext.kernels().kv_append(k, v, c1[0], c1[1], c1[2], c1[3], pos, 0)
    ref = A.decode_attention(q, c1[0], c1[1], cap, c1[2], c1[3], seq_len_dev=sl)
    out = A.decode_attention(q, c2[0], c2[1], cap, c2[2], c2[3], seq_len_dev=sl, k_new=k, v_new=v)
    _close(out, ref, 1e-6)
    for was, a, b_ in zip(before, c1, c2):
        if was is None:
            continue
        assert torch.equal(a, b_), "cache contents differ from kv_append's"
        for b, n in enumerate(lens):  # bitwise untouched outside the row's own slot
            assert torch.equal(b_[b, :, :n - 1], was[b, :, :n - 1]) and torch.equal(b_[b, :, n:], was[b, :, n:])
    if not int8:
        for b, n in enumerate(lens):
            assert torch.equal(c2[0][b, :, n - 1], k[b, 0]) and torch.equal(c2[1][b, :, n - 1], v[b, 0])


@pytest.mark.parametrize("B,H,Hkv,D,S,cap", [(3, 4, 4, 64, 700, 1100), (5, 8, 2, 128, 300, 320), (64, 12, 12, 64, 300, 640)])
def test_equal_lengths_are_bitwise_the_one_length_form(B, H, Hkv, D, S, cap):
    torch.manual_seed(S)
    q = torch.randn(B, 1, H, D, device=DEV).to(torch.bfloat16)
    kc, vc = _caches(B, Hkv, cap, D, [S] * B)
    one = A.decode_attention(q, kc, vc, cap, seq_len_dev=torch.tensor([S], device=DEV))
    cnt = A.decode_counters(torch.device(DEV))
    for _ in range(3):  # (a replayed graph reuses the counters)
        per_row = A.decode_attention(q, kc, vc, cap, seq_len_dev=torch.full((B,), S, device=DEV))
        assert torch.equal(per_row, one)
    torch.cuda.synchronize()
    assert cnt is None or int(cnt.abs().sum()) == 0


def test_in_kernel_rope_refuses_per_row_lengths():
    B, H, Hkv, D, cap = 2, 4, 1, 256, 64
    rows = torch.randn(B, 1, (H + 2 * Hkv) * D, device=DEV).to(torch.bfloat16)
    q, k, v = (t.reshape(B, 1, -1, D) for t in rows.split([H * D, Hkv * D, Hkv * D], dim=2))
    kc, vc = _caches(B, Hkv, cap, D, [cap] * B)
    rope = (torch.ones(D // 2, device=DEV), torch.zeros(D // 2, device=DEV))
    with pytest.raises(RuntimeError, match="RoPE"):
        A.decode_attention(q, kc, vc, cap, seq_len_dev=torch.tensor([5, 9], device=DEV), k_new=k, v_new=v, rope=rope)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embedding_with_per_row_positions(dtype):
    torch.manual_seed(0)
    V, P, C, B = 1000, 64, 768, 7
    wte, wpe = torch.randn(V, C, device=DEV).to(dtype), torch.randn(P, C, device=DEV).to(dtype)
    idx = torch.randint(0, V, (B, 1), device=DEV)
    pos = torch.tensor([0, 5, 63, 17, 17, 1, 100], device=DEV)  # (the last one is clamped to the table, as now)
    out = Fu.embedding_fwd(idx, wte, wpe, 0, pos_dev=pos)
    ref = wte[idx.view(-1)].float() + wpe[pos.clamp(max=P - 1)].float()
    _close(out, ref, 1e-6)  # (test_embedding's tolerance)
    one = Fu.embedding_fwd(idx, wte, wpe, 0, pos_dev=torch.tensor([17], device=DEV))
    assert torch.equal(one, Fu.embedding_fwd(idx, wte, wpe, 0, pos_dev=torch.full((B,), 17, device=DEV)))


@pytest.mark.parametrize("rows", [1, 3, 4])
def test_decode_gemv_emb_with_per_row_positions(rows):
    """The embedding rows it writes are exact sums of two bf16 values (1e-6, as the embedding kernel's test);
    its output — LayerNorm and a K = 128 dot product in fp32, rounded to bf16 once — is held to the bf16
    tolerance of the attention tests, 0.02 + 0.01·max|ref|."""
    torch.manual_seed(rows)
    V, P, C, N = 256, 64, 128, 384
    wte = torch.randn(V, C, device=DEV).to(torch.bfloat16)
    wpe = torch.randn(P, C, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, C, device=DEV) / math.sqrt(C)).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV).to(torch.bfloat16)
    gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.1
    idx = torch.randint(0, V, (rows,), device=DEV)
    pos = torch.tensor([9, 0, 63, 31][:rows], device=DEV)
    resid = torch.empty(rows, C, device=DEV)
    out = G.decode_gemv_emb(idx, pos, wte, wpe, resid, (gamma, beta, 1e-5), w, bias)
    x = wte[idx].float() + wpe[pos].float()
    _close(resid, x, 1e-6)
    ref = torch.nn.functional.layer_norm(x, (C,), gamma, beta, 1e-5) @ w.float().t() + bias.float()
    _close(out, ref, 0.02, 0.01)
    same = torch.empty_like(resid)
    a = G.decode_gemv_emb(idx, torch.tensor([31], device=DEV), wte, wpe, same, (gamma, beta, 1e-5), w, bias)
    b = G.decode_gemv_emb(idx, torch.full((rows,), 31, device=DEV), wte, wpe, resid, (gamma, beta, 1e-5), w, bias)
    assert torch.equal(a, b) and torch.equal(same, resid)


def test_rope_table_with_per_row_offsets():
    inv = 1.0 / (10000.0 ** (torch.arange(0, 256, 2, device=DEV).float() / 256))
    pos = torch.tensor([0, 7, 1023, 7, 300], device=DEV)
    cos, sin = Ro.rope_table(inv, 0, 1, DEV, offset_dev=pos)
    assert cos.shape == sin.shape == (5, 128)
    for r, p in enumerate(pos.tolist()):
        c1, s1 = Ro.rope_table(inv, 0, 1, DEV, offset_dev=torch.tensor([p], device=DEV))
        assert torch.equal(cos[r:r + 1], c1) and torch.equal(sin[r:r + 1], s1)
    with pytest.raises(ValueError):
        Ro.rope_table(inv, 0, 2, DEV, offset_dev=pos)


def test_counter_advance_per_row():
    """sample_step's fused advance and decode_advance add 1 to every row's position and length."""
    torch.manual_seed(0)
    k = _ext.kernels()
    B, V = 5, 256
    logits = torch.randn(B, V, device=DEV).to(torch.bfloat16)
    seed, step = torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV)
    idx = torch.zeros(B, 1, dtype=torch.long, device=DEV)
    out = torch.zeros(B, 8, dtype=torch.long, device=DEV)
    pos = torch.tensor([0, 4, 8, 2, 6], device=DEV)
    ln = pos + 1
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i in range(3):
        k.sample_step(logits, 0.0, 0, seed, step, idx, out, pos, ln, done)
    assert pos.tolist() == [3, 7, 11, 5, 9] and ln.tolist() == [4, 8, 12, 6, 10] and step.item() == 3 and done.item() == 0
    assert torch.equal(logits.float().gather(1, out[:, :3]), logits.float().amax(-1, keepdim=True).expand(B, 3))
    k.decode_advance(pos, ln, step)
    assert pos.tolist() == [4, 8, 12, 6, 10] and ln.tolist() == [5, 9, 13, 7, 11] and step.item() == 4
    one_a, one_b = torch.tensor([3], device=DEV), torch.tensor([4], device=DEV)
    k.sample_step(logits, 0.0, 0, seed, step, idx, out, one_a, one_b, done)  # the [1] form, as before
    k.decode_advance(one_a, one_b, step)
    assert one_a.item() == 5 and one_b.item() == 6 and step.item() == 6
    with pytest.raises(RuntimeError):
        k.sample_step(logits, 0.0, 0, seed, step, idx, out, pos, one_b, done)
