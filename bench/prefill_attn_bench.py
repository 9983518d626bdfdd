"""Prefill attention over the KV cache (csrc/kernels/prefill_attn.hip): three arms alternating in one
process — the MFMA prefill kernel, the decode-kernel route (PENROZ_PREFILL_ATTN=0, the previous code
path) and, at q_offset 0, flash_fwd on the same fused QKV (the same FLOPs without the cache: what the
hardware allows). Every arm is warmed up; a round times `--iters` launches between two synchronises, and
the median and the min-max spread of `--rounds` rounds are reported, with TF from the causal FLOP count.
Then time-to-first-token: generate_tokens(a 1024-token prompt, max_new_tokens=1), both routes alternating.

    python bench/prefill_attn_bench.py [--rounds 7] [--iters 10] [--no-ttft] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench as B_  # noqa: E402
from penroz.ops import attention as A, sampling as Sa  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
GPT2, GEMMA, D128 = (12, 12, 64), (4, 1, 256), (8, 2, 128)
# (name, (H, Hkv, D), B, Tq, q_offset, int8 cache)
SHAPES = ([("gpt2", GPT2, 1, 1024, 0, False), ("gpt2", GPT2, 8, 1024, 0, False)]
          + [("gpt2", GPT2, 1, t, off, False) for t in (16, 32, 64, 256) for off in (0, 512)]
          + [("gemma3-1b", GEMMA, 1, t, off, i8) for i8 in (False, True) for t, off in ((1024, 0), (4096, 0), (512, 3584))]
          + [("d128", D128, 1, 2048, 0, False)])


def causal_flops(B, H, D, Tq, off):
    """QKᵀ and PV over the visible keys only: 4·D per (query, key) pair."""
    pairs = Tq * off + Tq * (Tq + 1) // 2
    return 4.0 * D * B * H * pairs


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def with_route(on, fn):
    def run():
        os.environ["PENROZ_PREFILL_ATTN"] = "1" if on else "0"
        try:
            return fn()
        finally:
            os.environ.pop("PENROZ_PREFILL_ATTN", None)
    return run


def stats(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def attention_rows(rounds, iters, emit):
    os.environ["PENROZ_PREFILL_MIN_TQ"] = "1"  # the crossover rows time the new kernel below the default too
    for name, (H, Hkv, D), B, Tq, off, i8 in SHAPES:
        torch.manual_seed(0)
        S = off + Tq
        qkv = torch.randn(B, Tq, (H + 2 * Hkv) * D, device=DEV, dtype=BF)
        q = qkv[:, :, :H * D].view(B, Tq, H, D)
        kc, vc = (torch.randn(B, Hkv, S, D, device=DEV, dtype=BF) for _ in range(2))
        kc[:, :, off:] = qkv[:, :, H * D:(H + Hkv) * D].view(B, Tq, Hkv, D).transpose(1, 2)
        vc[:, :, off:] = qkv[:, :, (H + Hkv) * D:].view(B, Tq, Hkv, D).transpose(1, 2)
        sc = (None, None)
        if i8:
            kq, vq = (torch.empty(B, Hkv, S, D, device=DEV, dtype=torch.int8) for _ in range(2))
            sc = tuple(torch.empty(B, Hkv, S, device=DEV) for _ in range(2))
            Sa.kv_quantize_into(kc.transpose(1, 2), kq, sc[0], 0)
            Sa.kv_quantize_into(vc.transpose(1, 2), vq, sc[1], 0)
            kc, vc = kq, vq
        arms = {"prefill": with_route(True, lambda: A.decode_attention(q, kc, vc, S, *sc)),
                "decode": with_route(False, lambda: A.decode_attention(q, kc, vc, S, *sc))}
        if off == 0 and not i8:
            arms["flash"] = lambda: A.flash_fwd(qkv, H, Hkv, D)
        outs = {k: f() for k, f in arms.items()}  # first launches; also the outputs compared below
        diff = (outs["prefill"].float() - outs["decode"].float()).abs().max().item()
        for f in arms.values():
            timed(f, 3)
        us = {k: [] for k in arms}
        for _ in range(rounds):
            for k, f in arms.items():
                us[k].append(timed(f, iters))
        fl = causal_flops(B, H, D, Tq, off)
        row = {"shape": name, "H": H, "Hkv": Hkv, "D": D, "B": B, "Tq": Tq, "q_offset": off, "int8": i8,
               "max_abs_diff_vs_decode": round(diff, 5)}
        for k in arms:
            row[k + "_us"] = stats(us[k])
            row[k + "_TF"] = round(fl / statistics.median(us[k]) / 1e6, 2)
        emit(row)
    os.environ.pop("PENROZ_PREFILL_MIN_TQ", None)


def ttft_rows(rounds, emit):
    from penroz.models.mapper import Mapper
    from penroz.models.model import NeuralNetworkModel
    for name, layers, block in (("gpt2", B_.gpt2_layers(), 1024), ("gemma3-1b", B_.gemma3_1b_layers(), 2048)):
        torch.manual_seed(0)
        model = NeuralNetworkModel("ttft-" + name, Mapper(layers, {"adamw": {"lr": 1e-3}})).to(DEV)
        model.to(dtype=BF)
        n = min(1024, block - 1)  # GPT-2: the new token still fits its 1024-position window
        prompt = [torch.randint(0, 50000, (n,)).tolist()]
        arms = {k: with_route(on, lambda: model.generate_tokens(prompt, block, 1, temperature=0.0))
                for k, on in (("prefill", True), ("decode", False))}
        for f in arms.values():
            f(), f()
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, f in arms.items():
                ms[k].append(timed(f, 1) / 1e3)
        emit({"ttft": name, "prompt": n, **{k + "_ms": stats(v) for k, v in ms.items()}})
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-ttft", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    attention_rows(a.rounds, a.iters, emit)
    if not a.no_ttft:
        ttft_rows(a.rounds, emit)


if __name__ == "__main__":
    main()
