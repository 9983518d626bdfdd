"""Host-side launch plans of the HIP extension (no GPU needed: the built extension imports on the
CPU runner): the fused decode QKV + RoPE kernel's split-K plan is exported by the kernel's own
source and the Python admission check reads it instead of re-deriving the rule."""
import pytest

from penroz.ops import _ext, gemm as G

pytestmark = pytest.mark.skipif(not _ext.available(), reason="HIP extension not built")


@pytest.mark.parametrize("M,N,K", [(1, 1536, 1152), (64, 1536, 1152), (16, 6144, 5376), (1, 2304, 768),
                                   (64, 8192, 2048), (32, 4096 + 512, 4096)])
def test_qkv_rope_plan_matches_launch_rule(M, N, K):
    split, ws, counters = _ext.kernels().skinny_qkv_rope_plan(M, N, K)
    ntiles, steps = N // 32, K // 32
    assert 1 <= split <= max(1, min(16, steps))
    assert split == 1 or ntiles < 128  # wide outputs never split
    assert split == 1 or ntiles * split >= 192 or split == min(steps // 4, 16)  # ~192 workgroups
    mb = 1 if M <= 16 else 2 if M <= 32 else 4
    assert ws == (split * ntiles * mb * 512 if split > 1 else 0)
    assert counters == (ntiles if split > 1 else 0)
    assert G.qkv_rope_plan_fits(M, N, K) == (ws <= 1 << 19 and counters <= 1 << 12)


def test_qkv_rope_plan_admission_over_every_split():
    """Every split the launcher would pick is admitted exactly when its slabs fit the shared
    workspace; at 64 rows some narrow outputs do not (95 tiles split 3 ways: 583 680 floats), and
    those fall back before any graph capture instead of throwing inside it."""
    refused = []
    for tiles in range(1, 128):
        split, ws, counters = _ext.kernels().skinny_qkv_rope_plan(64, 32 * tiles, 32 * 4096)
        assert G.qkv_rope_plan_fits(64, 32 * tiles, 32 * 4096) == (ws <= 1 << 19)
        if ws > 1 << 19:
            refused.append(tiles)
    assert 95 in refused
    split, ws, _ = _ext.kernels().skinny_qkv_rope_plan(64, 32 * 16, 32 * 64)
    assert split == 12 and ws == 12 * 16 * 4 * 512


def test_decode_gemv_limits_are_the_launchers_own():
    """(rows, K, LN-mode K, paired-row K) of decode_gemv / decode_gemv_pair: the decode programs'
    admission checks (models/graph_decode.py) read the constants the launch checks use."""
    from penroz.models import graph_decode as gd

    assert _ext.kernels().decode_gemv_limits() == (4, 8192, 1024, 1792)
    assert gd._gemv_limits() == (4, 8192, 1024, 1792)


def _tiles(qb, BM, BN, T):
    return (min(T, (qb + 1) * BM) + BN - 1) // BN


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("nblk,nvh,slots,BM,T", [(8, 32, 256, 128, 1024), (16, 32, 512, 64, 1024), (8, 64, 256, 128, 1024),
                                                 (3, 2, 256, 128, 300), (40, 8, 512, 64, 2560), (1, 4, 256, 128, 100)])
def test_attn_work_plan_covers_every_tile_once(monkeypatch, mode, nblk, nvh, slots, BM, T):
    """flash_attn_gen.hip's causal work list: every query block's key tiles are covered exactly
    once (whole, or as the two halves [0, n/2) and [n/2, n)), split blocks are exactly those at or
    above split0, and items come heaviest first (the dispatch order the balance relies on)."""
    monkeypatch.setenv("PENROZ_ATTN_KV_SPLIT", mode)
    r = _ext.kernels().attn_work_plan(nblk, nvh, slots, BM, 32, T, 256, 2.7)
    n, split0, items = r[0], r[1], r[2:]
    if split0 >= nblk:  # nothing split: the kernel walks the blocks heaviest first by formula
        assert n == nblk and items == []
        return
    if mode == "2":
        assert split0 == 1
    assert n == len(items) == nblk + (nblk - split0)
    covered = {}
    sizes = []
    for e in items:
        qb, part = e & 0xFFFF, e >> 16
        nt = _tiles(qb, BM, 32, T)
        lo, hi = {0: (0, nt), 1: (0, nt // 2), 2: (nt // 2, nt)}[part]
        assert (part == 0) == (qb < split0)
        covered.setdefault(qb, []).append((lo, hi))
        sizes.append(hi - lo)
    for qb in range(nblk):
        spans = sorted(covered[qb])
        assert spans[0][0] == 0 and spans[-1][1] == _tiles(qb, BM, 32, T)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert sizes == sorted(sizes, reverse=True)


def test_attn_work_plan_off_and_many_rounds(monkeypatch):
    """PENROZ_ATTN_KV_SPLIT=0 never splits; grids of several rounds are not split either."""
    monkeypatch.setenv("PENROZ_ATTN_KV_SPLIT", "0")
    assert _ext.kernels().attn_work_plan(8, 32, 256, 128, 32, 1024, 256, 2.7)[:2] == [8, 8]
    monkeypatch.setenv("PENROZ_ATTN_KV_SPLIT", "1")
    assert _ext.kernels().attn_work_plan(8, 768, 256, 128, 32, 1024, 256, 2.7)[:2] == [8, 8]
    r = _ext.kernels().attn_work_plan(8, 32, 256, 128, 32, 1024, 256, 2.7)
    assert r[1] < 8  # the Gemma-3 1B B=8 forward grid (one round) is split


# sampler paths of sample_plan's first field
TWO_STAGE, REGISTER, STREAM = 0, 1, 2


def _sample_plan(dtype, V, temperature, top_k, filtered, B=1, min_rows=None):
    import torch
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}[dtype]
    return _ext.kernels().sample_plan(dt, B, V, temperature, top_k, filtered, min_rows)


@pytest.mark.parametrize("dtype,V,temperature,top_k,filtered,plan", [
    ("bf16", 50304, 0.8, 50, False, (TWO_STAGE, 0, 13, 50)),
    ("bf16", 50304, 0.8, 0, False, (REGISTER, 13, 0, 0)),
    ("bf16", 50304, 0.8, 0, True, (STREAM, 0, 0, 0)),  # 13 chunks: not built with the nucleus code
    ("bf16", 40960, 0.8, 0, True, (REGISTER, 10, 0, 0)),
    ("bf16", 40960, 0.8, 100, False, (REGISTER, 10, 0, 0)),  # top_k above the two-stage pair's 64
    ("fp32", 8192, 0.8, 50, False, (TWO_STAGE, 0, 2, 50)),
    ("bf16", 262144, 0.8, 50, False, (TWO_STAGE, 0, 64, 50)),
    ("bf16", 262152, 0.8, 50, False, (STREAM, 0, 0, 0)),  # one chunk past 64 parts
    ("fp32", 96000, 0.8, 0, False, (STREAM, 0, 0, 0)),
    ("fp32", 96000, 0.0, 0, False, (TWO_STAGE, 0, 24, 0)),  # greedy
    ("fp32", 1024, 0.8, 0, False, (REGISTER, 1, 0, 0)),
    ("fp16", 4096, 0.8, 50, False, (STREAM, 0, 0, 0)),
    ("fp16", 4096, 0.0, 0, False, (STREAM, 0, 0, 0)),
    ("bf16", 50257, 0.8, 50, True, (STREAM, 0, 0, 0)),
    ("bf16", 50257, 0.0, 0, False, (STREAM, 0, 0, 0)),
])
def test_sample_plan_table(dtype, V, temperature, top_k, filtered, plan):
    """Which sampler kernel serves a row (host_plan.h plan_sample), worked out by hand from the
    launch rule; PENROZ_SAMPLE_TWO_STAGE_MIN_ROWS at its default of 1."""
    assert _sample_plan(dtype, V, temperature, top_k, filtered, min_rows=1) == plan
    assert _sample_plan(dtype, V, temperature, top_k, filtered) == plan  # None: the process's own value (unset: 1)


def test_sample_plan_min_rows_and_filter_at_temperature_zero():
    """With the switch at 2 rows a single bf16 row of 50 304 logits stays in registers; two rows
    take the two-stage pair. Temperature 0 ignores the filters."""
    assert _sample_plan("bf16", 50304, 0.8, 50, False, B=1, min_rows=2) == (REGISTER, 13, 0, 0)
    assert _sample_plan("bf16", 50304, 0.8, 50, False, B=2, min_rows=2) == (TWO_STAGE, 0, 13, 50)
    assert _sample_plan("bf16", 50304, 0.0, 0, True, min_rows=1) == _sample_plan("bf16", 50304, 0.0, 0, False, min_rows=1)


# (B, H, Hkv, D, S, bf16_plain, counters) -> (small, splits, keys per split, merge); None: not asserted
_DECODE_PLANS = [
    ((1, 12, 12, 64, 1024, True, 4096), (False, 4, 256, True)),
    ((1, 12, 12, 64, 1024, True, 0), (False, 1, 1024, False)),
    ((64, 12, 12, 64, 1024, True, 4096), (False, 1, None, None)),
    ((64, 12, 12, 64, 1024, True, 0), (False, 1, None, None)),
    ((1, 4, 1, 256, 1024, True, 4096), (True, 1, None, False)),
    ((1, 4, 1, 256, 1024, True, 0), (True, 1, None, False)),
    ((1, 4, 1, 256, 1024, False, 4096), (False, 4, 256, True)),  # fp32 / fp16 q or an int8 cache
    ((1, 4, 1, 256, 1025, True, 4096), (False, None, None, None)),
    ((1, 4, 1, 256, 1025, True, 0), (False, None, None, None)),
    ((65, 4, 1, 256, 1024, True, 0), (False, None, None, None)),
    ((1, 16, 1, 512, 1024, True, 0), (False, None, None, None)),
    ((1, 8, 1, 512, 1024, True, 0), (True, 1, None, False)),
    ((1, 4, 1, 256, 16384, True, 8192), (False, 16, 1024, False)),
    ((1, 4, 1, 256, 8192, True, 8192), (False, 16, 256, True)),
]


@pytest.mark.parametrize("shape,plan", _DECODE_PLANS)
def test_decode_attn_plan_table(shape, plan):
    """decode_attn's launch plan (host_plan.h plan_decode_attn), worked out by hand from the launch
    rule with the environment switches unset, and decode_small_applies (what ops/attention.py asks)
    agreeing with it."""
    B, H, Hkv, D, S, plain, counters = shape
    K = _ext.kernels()
    got = K.decode_attn_plan(B, 1, H, Hkv, D, S, plain, counters)
    assert all(w is None or g == w for g, w in zip(got, plan)), got
    assert got[1] >= 1 and (not got[3] or (got[1] <= 16 and S <= 8192))
    assert K.decode_small_applies(B, 1, H, Hkv, D, S) == K.decode_attn_plan(B, 1, H, Hkv, D, S, True, counters)[0]
    assert not K.decode_attn_plan(B, 2, H, Hkv, D, S, plain, counters)[0]  # two query rows: never the small kernel
