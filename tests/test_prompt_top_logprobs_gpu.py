"""The top-n form of csrc/kernels/lmhead_lse.hip against ``reference_top_n`` (fp64), on the MI355X. Measured there:
largest logit shortfall 0, largest log-probability deviation 4.5e-6, against the existing check's bound 2.32e-4."""
import functools

import pytest
import torch
from test_prompt_logprobs_gpu import BF, BOUND, DEV, K, _gemma, _gpt  # (skips this module too where there is no GPU)

from penroz.ops.prompt_logprobs import reference_top_n

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(N, V, C, bias, lossless):
    """(h, W, bias, targets) on the device and the fp64 (ids, logprobs, logits) for n = 20. Lossless: small integers, equal
    logits everywhere; rows 0 and N - 1 reach the largest possible logit at 21 or 25 (V = 17: 4) columns on both sides of the
    half-wave (3 | 4), tile (127 | 128), range (1791 | 1792, 3583 | 3584) and ragged-tile boundaries; row 1 is all zeros."""
    g = torch.Generator().manual_seed(N + V + C)
    if lossless:
        h, W = (torch.randint(-2, 3, (s, C), generator=g).float() for s in (N, V))
        b = torch.randint(-3, 4, (V,), generator=g).float() if bias else None
        ties = [c for c in (3, 4, 127, 128, 1791, 1792, 3583, 3584, V - 2, V - 1, *range(200, 215)) if c < V]
        h[0] = h[N - 1] = W[ties] = torch.randint(0, 2, (C,), generator=g).float() * 4 - 2
        h[1 % N] = h[1 % N] * (N == 1)
        if bias:
            b[ties] = 3
    else:
        h, W = torch.randn(N, C, generator=g), torch.randn(V, C, generator=g) / C ** 0.5
        b = torch.randn(V, generator=g) if bias else None
    h, W, b = h.to(DEV, BF), W.to(DEV, BF), None if b is None else b.to(DEV)
    x = h.double() @ W.double().T + (0 if b is None else b.double())
    return (h, W, b, torch.randint(0, V, (N,), generator=g).to(DEV)), (*reference_top_n(h, W, b, 20), x)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n", [1, 5, 20])
@pytest.mark.parametrize("V, splits", [(17, 0), (1001, 0), (5000, 3)])  # S = 1; 8; 3 ranges of 14 tiles
@pytest.mark.parametrize("N", [1, 129, 514])  # 514: the 256-row form without n
@pytest.mark.parametrize("C, lossless", [(64, True), (32, False), (768, False)])
def test_against_the_reference(C, lossless, N, V, splits, n, bias):
    args, (r_ids, r_lps, x) = case(N, V, C, bias, lossless)
    assert K.lmhead_lse_plan(N, V, C, splits, n)[:2] == (128, {17: 1, 1001: 8, 5000: 3}[V])
    lp, top, top_lp, ids, lps = K.lmhead_lse(*args, splits, top_n=n)
    k = min(n, V)
    assert ids.shape == lps.shape == (N, n) and (ids[:, k:] == -1).all() and (lps[:, k:] == float("-inf")).all()
    assert torch.equal(ids[:, 0], top) and torch.equal(lps[:, 0].view(torch.int32), top_lp.view(torch.int32))
    if lossless:  # ids and order exactly; the logsumexp's own rounding at logits up to 256 (the existing test's 1e-4)
        assert torch.equal(ids, r_ids[:, :n]) and (lps[:, :k].double() - r_lps[:, :k]).abs().max() < 1e-4
        return
    got = x.gather(1, ids[:, :k])  # the fp64 logits of the returned ids: none below the fp64 k-th best by more than the bound
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    print(f"shortfall {(x.gather(1, r_ids[:, k - 1:k]) - got).max().item():.3e}, deviation {(lps[:, :k].double() - (got - lse)).abs().max().item():.3e}")
    assert (ids[:, :k].sort(dim=-1).values.diff(dim=-1) > 0).all() and (got >= x.gather(1, r_ids[:, k - 1:k]) - BOUND).all()
    assert (lps[:, :k].double() - (got - lse)).abs().max() <= BOUND and (lps[:, :k].diff(dim=-1) <= 0).all()


@pytest.mark.parametrize("bias", [False, True])
def test_consistency_with_the_plain_launch(bias):
    (h, W, b, t), _ = case(129, 1001, 768, bias, False)
    bits = lambda r: [y.view(torch.int32) if y.dtype == torch.float32 else y for y in r]  # noqa: E731
    plain, big = bits(K.lmhead_lse_raw(h, W, b, t, 8)), bits(K.lmhead_lse_raw(h, W, b, t, 8, top_n=5))
    again = bits(K.lmhead_lse_raw(h, W, b, t, 8, top_n=5))  # the same row tile and S: the plain launch's bits; a second run's
    assert all(torch.equal(a, c) for a, c in zip(plain, big[:5])) and all(torch.equal(a, c) for a, c in zip(big, again))
    for r in (0, 77, 128):  # a row scored alone, at the same S
        one = bits(K.lmhead_lse_raw(h[r:r + 1].clone(), W, b, t[r:r + 1].clone(), 8, top_n=5))
        assert all(torch.equal(a, c[r:r + 1]) for a, c in zip(one, big))


@pytest.mark.parametrize("make", [_gpt, _gemma])
def test_through_the_model(make):
    m = make()
    seqs = [torch.randint(0, 256, (s,), generator=torch.Generator().manual_seed(s)).tolist() for s in (13, 6)]
    got, plain = m.score_tokens(seqs, 16, top_n=5), m.score_tokens(seqs, 16)
    assert [m.score_tokens([s], 16, top_n=5)[0] for s in seqs] == got  # row by row: the batched call exactly
    assert [{k: v for k, v in d.items() if k != "top_n"} for d in got] == plain and all("top_n" in d for d in got)
    assert all(len(p) == 5 and p[0] == [i, x] for d in got for p, i, x in zip(d["top_n"][1:], d["top_tokens"][1:], d["top_logprobs"][1:]))
    tokens, info = m.generate_tokens([seqs[1]], 16, 6, temperature=0.0, prompt_logprobs=True, prompt_top_logprobs=5)
    assert tokens == m.generate_tokens([seqs[1]], 16, 6, temperature=0.0) and info == {"prompt_logprobs": got[1]}
    assert m.generate_tokens([seqs[1]], 16, 6, temperature=0.0, prompt_logprobs=True)[1] == {"prompt_logprobs": plain[1]}
