"""prefill_attn's launch plan (host_plan.h plan_prefill_attn, no GPU needed): what it admits, that its grid
covers every (batch, KV head, query tile) once, its LDS, and that ops.attention.prefill_applies reads it."""
import pytest
import torch

from penroz.ops import _ext, attention as A

pytestmark = pytest.mark.skipif(not _ext.available(), reason="HIP extension not built")

BF16, I8, F16, F32 = torch.bfloat16, torch.int8, torch.float16, torch.float32
SHAPES = [(B, Tq, H, Hkv, D) for D in (64, 128, 256) for H, Hkv in ((2, 2), (4, 2), (4, 1), (8, 1))
          for B, Tq in ((1, 16), (2, 33), (1, 130), (8, 1024), (1, 4096))]


def _plan(B, Tq, H, Hkv, D, qdt=BF16, cdt=BF16):
    return _ext.kernels().prefill_attn_plan(B, Tq, H, Hkv, D, qdt == BF16, {BF16: "bf16", I8: "int8"}.get(cdt, "other"))


@pytest.mark.parametrize("cdt", [BF16, I8])
@pytest.mark.parametrize("B,Tq,H,Hkv,D", SHAPES)
def test_admitted_plan_covers_every_tile_once(B, Tq, H, Hkv, D, cdt):
    ok, rows, pos, grid, lds = _plan(B, Tq, H, Hkv, D, cdt=cdt)
    G = H // Hkv
    assert ok and rows in (32, 64, 128) and pos * G == rows
    tiles = -(-Tq // pos)
    assert grid == B * Hkv * tiles and (tiles - 1) * pos < Tq <= tiles * pos
    # the widest tile that still gives a workgroup per CU, else the narrowest
    assert rows == 32 or grid >= 256
    assert rows == 128 or B * Hkv * -(-Tq * G // (2 * rows)) < 256
    assert 0 < lds <= 160 * 1024
    assert A.prefill_applies(B, Tq, H, Hkv, D, BF16, cdt)


@pytest.mark.parametrize("B,Tq,H,Hkv,D,qdt,cdt", [
    (1, 64, 4, 4, 32, BF16, BF16), (1, 64, 4, 4, 512, BF16, BF16), (1, 64, 6, 2, 64, BF16, BF16),
    (1, 64, 16, 1, 64, BF16, BF16), (1, 64, 4, 4, 64, F16, F16), (1, 64, 4, 4, 64, F32, F32),
    (1, 64, 4, 4, 64, F16, I8), (1, 64, 4, 3, 64, BF16, BF16)])
def test_refused_shapes_stay_on_the_decode_kernel(B, Tq, H, Hkv, D, qdt, cdt):
    assert _plan(B, Tq, H, Hkv, D, qdt, cdt) == (False, 0, 0, 0, 0)
    assert not A.prefill_applies(B, Tq, H, Hkv, D, qdt, cdt)
