"""``n`` samples of one prompt (ops/shared_prefix.py) without a GPU: ``check_n``'s refusals, the neutral values,
the replicated fallback, the op's CPU form against the fp64 definition, the kernel's launch plan, ``/generate``."""
from unittest.mock import patch

import pytest
import torch
from fastapi.testclient import TestClient

import bench
import main
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import _ext
from penroz.ops import attention as attn_ops
from penroz.ops import shared_prefix as sp
from penroz.ops.decode_options import check_options
from penroz.serve import app as A

V, BLOCK, NEW = 256, 32, 6
PROMPT = [3, 1, 4, 1, 5]


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return NeuralNetworkModel("sp", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 3e-3}}))


def _shape(**kw):
    return {"rows": 1, "prompt_len": 5, "block_size": BLOCK, "stream": False, **kw}


@pytest.mark.parametrize("n, shape, extra", [
    (0, _shape(), {}), (65, _shape(), {}), (2.0, _shape(), {}), (True, _shape(), {}),  # the value
    (2, _shape(rows=2), {}),                                                           # several prompt rows
    (2, _shape(stream=True), {}),                                                      # stream
    (2, _shape(), {"speculate": 2, "temperature": 0.0}),                               # speculate
    (2, _shape(prompt_len=BLOCK - NEW + 1), {}),                                       # the window would slide
    (2, _shape(single=True), {}),                                                      # generate_tokens*
])
def test_check_n_refuses(n, shape, extra):
    with pytest.raises(ValueError):
        check_options(V, NEW, extra.pop("temperature", 1.0), None, n=n, call_shape=shape, **extra)


def test_generate_tokens_refuses_n_before_any_forward(monkeypatch, tiny):
    monkeypatch.setattr(NeuralNetworkModel, "forward", lambda *a, **k: pytest.fail("forward ran before validation"))
    with pytest.raises(ValueError, match="generate_batch"):
        tiny.generate_tokens([PROMPT], BLOCK, NEW, n=2)
    with pytest.raises(ValueError, match="generate_batch"):
        list(tiny.generate_tokens_stream([PROMPT], BLOCK, NEW, n=2))
    with pytest.raises(ValueError, match="window"):
        tiny.generate_batch([PROMPT], BLOCK, BLOCK, n=2)
    for empty in ([], [[]]):
        with pytest.raises(ValueError, match="one prompt"):
            tiny.generate_batch(empty, BLOCK, NEW, n=2)


@pytest.mark.parametrize("n", [None, 1])
def test_neutral_values_are_the_plain_call(n):
    assert check_options(V, NEW, 1.0, 5, n=n, call_shape=_shape()) == check_options(V, NEW, 1.0, 5)
    assert check_options(V, NEW, 1.0, 5, n=3, call_shape=_shape()).n == 3


def test_cpu_fallback_is_the_replicated_call(tiny):
    torch.manual_seed(7)
    got = tiny.generate_batch(PROMPT, BLOCK, NEW, temperature=1.0, top_k=20, n=3, logprobs=0)
    torch.manual_seed(7)
    want = tiny.generate_batch([PROMPT] * 3, BLOCK, NEW, temperature=1.0, top_k=20, logprobs=0)
    assert got == want and len(got[0]) == 3 and tiny.last_shared_prefix is None


@pytest.mark.parametrize("D, H, Hkv, R, P, suffix", [(64, 2, 2, 2, 1, 1), (64, 2, 2, 33, 65, 1)])
def test_cpu_op_is_the_definition(D, H, Hkv, R, P, suffix):
    g = torch.Generator().manual_seed(1)
    q, kn, vn = (torch.randn(R, h, D, generator=g) for h in (H, Hkv, Hkv))
    kp, vp = torch.randn(1, Hkv, P + 3, D, generator=g), torch.randn(1, Hkv, P + 3, D, generator=g)
    ks, vs = torch.randn(R, Hkv, suffix + 2, D, generator=g), torch.randn(R, Hkv, suffix + 2, D, generator=g)
    out = attn_ops.shared_prefix_attention(q, kn, vn, kp, vp, ks, vs, torch.tensor([P]), torch.tensor([P + suffix]))
    assert torch.equal(ks[:, :, suffix - 1], kn) and torch.equal(vs[:, :, suffix - 1], vn)
    # the definition, written out per row and head
    ref = torch.empty(R, H, D, dtype=torch.float64)
    for r in range(R):
        for h in range(H):
            hk = h // (H // Hkv)
            k = torch.cat([kp[0, hk, :P], ks[r, hk, :suffix]]).double()
            v = torch.cat([vp[0, hk, :P], vs[r, hk, :suffix]]).double()
            ref[r, h] = torch.softmax(k @ q[r, h].double() / D ** 0.5, 0) @ v
    assert torch.allclose(out.double(), ref.reshape(R, H * D), atol=1e-5)


needs_ext = pytest.mark.skipif(not _ext.available(), reason="the extension is not built")


@needs_ext
@pytest.mark.parametrize("R, H, Hkv, D, capP", [(4, 12, 12, 64, 1024), (64, 12, 12, 64, 1024), (16, 4, 1, 256, 4096),
                                                (64, 4, 1, 256, 4096), (2, 2, 2, 64, 1)])
def test_plan_ranges_tile_the_prefix(R, H, Hkv, D, capP):
    K = _ext.kernels()
    ok, tile_rows, tiles, S, grid, lds, ws = K.shared_prefix_plan(R, H, Hkv, D, capP)
    G = H // Hkv
    assert ok and S >= 1 and tile_rows * tiles >= R * G and grid == Hkv * tiles * S + R * Hkv and lds <= 160 * 1024
    assert ws == (S + 1) * R * H * (D + 2)
    for P in {1, min(64, capP), min(65, capP), capP}:
        ranges = [r for r in K.shared_prefix_ranges(P, S) if r[0] < r[1]]
        assert ranges[0][0] == 0 and ranges[-1][1] == P
        assert all(a[1] == b[0] and a[1] % 64 == 0 for a, b in zip(ranges, ranges[1:]))


@needs_ext
@pytest.mark.parametrize("R, H, Hkv, D", [(1, 2, 2, 64), (65, 2, 2, 64), (4, 2, 2, 32), (4, 6, 2, 64)])
def test_plan_refuses(R, H, Hkv, D):
    assert not _ext.kernels().shared_prefix_plan(R, H, Hkv, D, 128)[0]


client = TestClient(main.app, raise_server_exceptions=False)
BODY = {"model_id": "t", "input": PROMPT, "block_size": BLOCK, "max_new_tokens": NEW, "temperature": 1.0, "n": 3}


def test_api_n_returns_n_sequences_and_refuses_stream(tiny):
    with patch.object(A, "load_for_serving", return_value=tiny):
        r = client.post("/generate/", json=BODY)
        assert r.status_code == 200
        seqs = r.json()["sequences"]
        assert len(seqs) == 3 and all(s[:len(PROMPT)] == PROMPT and len(s) == len(PROMPT) + NEW for s in seqs)
    with patch.object(A, "load_for_serving", side_effect=AssertionError("loaded before the check")):
        assert client.post("/generate/", json={**BODY, "stream": True}).status_code == 400
