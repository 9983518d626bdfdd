"""Prompt scoring on the device (csrc/kernels/lmhead_lse.hip) against ``reference_score`` (fp64), and
``score_tokens`` / ``generate_tokens(prompt_logprobs=True)`` through tiny bf16 GPT and Gemma models.

Tolerance. ``FP32_TORCH_DEV`` is the largest deviation of plain fp32 torch (``h.float() @ W.float().T``,
``logsumexp``, ``gather``) from the fp64 reference over every case of ``test_normal_operands`` below,
measured on the CPU from the same inputs (``make_case``): 2.9e-5, at the rows whose logits reach ±80 to ±110
(one unit of fp32 there is 7.6e-6). The kernel is allowed ``BOUND = 8 × FP32_TORCH_DEV``: it sums over C and
over the vocabulary splits in another order and uses the hardware exp2. With these seeds the fp64 gap
between a row's two best logits is below ``BOUND`` in at most 2 % of a case's rows (measured: at most one
row per case); ``top_token`` must match in all others."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext
from penroz.ops import prompt_logprobs as plp_ops
from penroz.ops.prompt_logprobs import reference_score

DEV, BF = "cuda", torch.bfloat16
FP32_TORCH_DEV = 2.9e-5
BOUND = 8 * FP32_TORCH_DEV
K = _ext.kernels()
TILE = K.lmhead_lse_plan(1, 1001, 768)[0]  # the row tile of small N


def make_case(N, V, C, bias, seed=0):
    """CPU operands: logits ~ N(0, 1); every third row scaled until its logits reach about ±80, every third
    dominated by one logit (the target's in half of those)."""
    g = torch.Generator().manual_seed(seed + 7 * N + V + C)
    h = torch.randn(N, C, generator=g)
    W = torch.randn(V, C, generator=g) / C ** 0.5
    t = torch.randint(0, V, (N,), generator=g)
    for i in range(N):
        kind = (i + V) % 3
        if kind == 1:
            h[i] *= 20.0
        elif kind == 2:
            k = int(t[i]) if i % 2 else (int(t[i]) + 1) % V
            h[i] = 40.0 * W[k] / W[k].norm() ** 2
    b = torch.randn(V, generator=g) if bias else None
    return h.to(BF), W.to(BF), b, t


def check(got, h, W, b, t):
    lp, top, top_lp = (x.cpu() for x in got[:3])
    r_lp, r_top, r_top_lp = (x.cpu() for x in reference_score(h.to(DEV), W.to(DEV), None if b is None else b.to(DEV), t))
    d_lp, d_top = (lp.double() - r_lp).abs().max().item(), (top_lp.double() - r_top_lp).abs().max().item()
    print(f"token_logprob deviation {d_lp:.3e}, top_logprob deviation {d_top:.3e}, bound {BOUND:.3e}")
    assert lp.dtype == top_lp.dtype == torch.float32 and top.dtype == torch.int64 and torch.isfinite(lp).all()
    assert d_lp <= BOUND and d_top <= BOUND
    x = h.to(DEV).double() @ W.to(DEV).double().T + (0 if b is None else b.to(DEV).double())
    best2 = x.topk(min(2, x.shape[1]), dim=-1).values.cpu()
    clear = (best2[:, 0] - best2[:, -1] > BOUND) | (x.shape[1] == 1)
    assert (~clear).sum().item() <= 0.02 * len(t) + (len(t) < 50)  # at most 2 % of rows are too close to call
    assert torch.equal(top[clear], r_top[clear])
    if h.shape[1] >= 768:  # (32 dimensions leave 5000 random directions too close for one logit to dominate)
        i = torch.arange(len(t))
        dominated = (i + W.shape[0]) % 3 == 2
        assert (lp[dominated & (i % 2 == 1)] > -1e-3).all() and (lp[dominated & (i % 2 == 0)] < -20).all()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("C", [32, 768])
@pytest.mark.parametrize("V, splits", [(100, 0), (1001, 0), (5000, 3)])  # one ragged tile; S = 8; S = 3 of 14 tiles
@pytest.mark.parametrize("N", [1, TILE - 1, TILE + 1, 511, 513])  # 513: the 256-row form, its last tile one row
def test_normal_operands(N, V, splits, C, bias):
    h, W, b, t = make_case(N, V, C, bias)
    assert K.lmhead_lse_plan(N, V, C)[0] == (256 if N == 513 else TILE)
    assert K.lmhead_lse_plan(N, V, C, splits)[1] == {100: 1, 1001: 8, 5000: 3}[V]
    dev = [x.to(DEV) for x in (h, W)] + [None if b is None else b.to(DEV), t.to(DEV)]
    check(K.lmhead_lse(*dev, splits), h, W, b, t)
    if splits == 0:
        check(plp_ops.score_rows(*dev), h, W, b, t)  # the public entry takes the kernel for these


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N", [TILE + 2, 514])  # the 128-row and the 256-row form
def test_lossless_operands_are_exact(N, bias):
    """Small integers: every logit is exact in fp32 in any summation order."""
    V, C = 1001, 64
    g = torch.Generator().manual_seed(1)
    h = torch.randint(-2, 3, (N, C), generator=g).float()
    W = torch.randint(-2, 3, (V, C), generator=g).float()
    t = torch.randint(0, V, (N,), generator=g)
    pa, pb = (torch.randint(0, 2, (C,), generator=g).float() * 4 - 2 for _ in range(2))
    h[3], h[TILE] = pa, pb
    W[900], W[5] = pa, pa      # row 3: equal maxima in the first and the last (ragged) split
    W[405], W[400] = pb, pb    # row TILE: equal maxima inside one tile
    h[7] = 0                   # every logit equal (without the bias)
    t[:6] = torch.tensor([0, V - 1, 897, 5, 900, 400])  # column 0, the last, inside the ragged last tile
    b = torch.randint(-3, 4, (V,), generator=g).float() if bias else None
    args = [h.to(DEV, BF), W.to(DEV, BF), None if b is None else b.to(DEV), t.to(DEV)]
    lp, top, top_lp, x_t, _ = (x.cpu() for x in K.lmhead_lse_raw(*args, 3))
    x = h.double() @ W.double().T + (0 if b is None else b.double())
    r_lp, r_top, r_top_lp = reference_score(h, W, b, t)
    assert torch.equal(x_t.double(), x.gather(1, t.view(-1, 1)).squeeze(1)) and torch.equal(top, r_top)
    # (logits up to 256, where one unit of fp32 is 3e-5: the logsumexp's own rounding)
    assert (lp.double() - r_lp).abs().max() < 1e-4 and (top_lp.double() - r_top_lp).abs().max() < 1e-4
    if not bias:
        assert top[3] == 5 and top[TILE] == 400 and top[7] == 0
        assert abs(lp[7].item() + torch.tensor(float(V)).log().item()) < 1e-5


@pytest.mark.parametrize("N, bias", [(TILE + 1, False), (513, False), (513, True)])  # 513: N = 1 against the 256-row form
def test_a_row_does_not_depend_on_its_neighbours(N, bias):
    h, W, b, t = (None if x is None else x.to(DEV) for x in make_case(N, 1001, 768, bias, seed=5))
    S = K.lmhead_lse_plan(1, 1001, 768)[1]
    big = K.lmhead_lse_raw(h, W, b, t, S)
    for r in (77, 200 % N, N - 1):  # lanes of different waves and blocks of the first tile; the last tile's only row
        one = K.lmhead_lse_raw(h[r:r + 1].clone(), W, b, t[r:r + 1].clone(), S)
        for x, y in zip(one, big):
            assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else x.dtype),
                               y[r:r + 1].view(torch.int32 if y.dtype == torch.float32 else y.dtype))


# ------------------------------------------------------------------ through the models
def _gpt():
    torch.manual_seed(11)
    m = NeuralNetworkModel("gd", Mapper(bench.gpt2_layers(V=256, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=BF)


def _gemma():
    from types import SimpleNamespace
    tc = SimpleNamespace(vocab_size=256, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=64,
                         num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                         attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
    torch.manual_seed(5)
    m = NeuralNetworkModel("gg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}})).to(DEV)
    return m.to(dtype=BF)


@pytest.mark.parametrize("make", [_gpt, _gemma])
def test_score_tokens_and_the_option(make):
    m = make()
    seqs = [torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(n)).tolist() for n in (13, 6)]
    got = m.score_tokens(seqs, 16)
    assert [m.score_tokens([s], 16)[0] for s in seqs] == got  # row by row: the batched call exactly
    head = m.layers[m._head_index()]
    seen = []
    hook = head.register_forward_hook(lambda mod, args, out: seen.append(args[0]))
    x = torch.tensor([seqs[0], seqs[1] + [seqs[1][-1]] * 7], device=DEV)
    with torch.inference_mode(), m._autocast(torch.device(DEV)):
        m(x, skip_softmax=True)
    hook.remove()
    hidden = seen[0].to(BF)  # as the bf16 projection reads them (a LayerNorm under autocast hands it fp32 rows)
    assert head.weight.dtype == BF and plp_ops.kernel_takes(hidden[0], head.weight)  # the kernel's operands
    for b, s in enumerate(seqs):
        lp, top, top_lp = reference_score(hidden[b, :len(s) - 1], head.weight, head.bias, torch.tensor(s[1:]))
        assert (torch.tensor(got[b]["token_logprobs"][1:]) - lp.cpu()).abs().max() <= BOUND
        assert (torch.tensor(got[b]["top_logprobs"][1:]) - top_lp.cpu()).abs().max() <= BOUND
    plain = m.generate_tokens([seqs[1]], 16, 6, temperature=0.0)
    tokens, info = m.generate_tokens([seqs[1]], 16, 6, temperature=0.0, prompt_logprobs=True)
    assert tokens == plain and info == {"prompt_logprobs": got[1]}
