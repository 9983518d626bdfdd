"""n samples of one prompt (csrc/kernels/shared_prefix_attn.hip): the shared-prefix attention, both launches,
against decode_attention on the replicated cache of the same content — the arms alternate in one process,
every arm is warmed up, a round times `--iters` launches between two synchronises, and the median and the
min-max spread of `--rounds` rounds are reported. Then generate_batch(n = R) against the replicated call:
ms per decode step (from two call lengths) and the time to the first token, the arms alternating as well.

    python bench/shared_prefix_bench.py [--rounds 7] [--iters 200] [--no-e2e] [--int8] [--out FILE]

--int8: the same arms over the int8 KV cache (csrc/kernels/shared_prefix_attn_q8.hip against decode_attention's fused
int8 append on the replicated int8 cache; end to end with the TurboQuant cache switched on for the process).
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
from penroz.ops import attention as A  # noqa: E402
from penroz.ops._ext import kernels  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
GPT2, GEMMA = (12, 12, 64), (4, 1, 256)
# (name, (H, Hkv, D), prefix lengths)
SHAPES = [("gpt2", GPT2, (128, 1024)), ("gemma3-1b", GEMMA, (128, 1024, 4096))]
ROWS, SUFFIXES = (4, 16, 64), (1, 128)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def stats(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def _q8(shape):
    """A random int8 cache of this shape and its per-token scales."""
    return (torch.randint(-127, 128, shape, device=DEV, dtype=torch.int8),
            (0.5 + torch.rand(shape[:3], device=DEV)) / 127)


def attention_rows(rounds, iters, emit, int8=False):
    for name, (H, Hkv, D), prefixes in SHAPES:
        for P in prefixes:
            for R in ROWS:
                for suffix in SUFFIXES:
                    torch.manual_seed(0)
                    qkv = torch.randn(R, (H + 2 * Hkv) * D, device=DEV, dtype=BF)
                    q, k, v = qkv.split([H * D, Hkv * D, Hkv * D], dim=1)
                    q, k, v = q.view(R, H, D), k.view(R, Hkv, D), v.view(R, Hkv, D)
                    kp, vp = (torch.randn(1, Hkv, P, D, device=DEV, dtype=BF) for _ in range(2))
                    ks, vs = (torch.randn(R, Hkv, suffix, D, device=DEV, dtype=BF) for _ in range(2))
                    pt = torch.tensor([P], device=DEV)
                    lt = torch.tensor([P + suffix], device=DEV)
                    # the replicated cache of the same content; its arm appends the step's K/V itself as well
                    kc = torch.cat([kp.expand(R, -1, -1, -1), ks], dim=2).contiguous()
                    vc = torch.cat([vp.expand(R, -1, -1, -1), vs], dim=2).contiguous()
                    arms = {"shared": lambda: A.shared_prefix_attention(q, k, v, kp, vp, ks, vs, pt, lt),
                            "replicated": lambda: A.decode_attention(q.unsqueeze(1), kc, vc, P + suffix, seq_len_dev=lt,
                                                                     k_new=k.unsqueeze(1), v_new=v.unsqueeze(1))}
                    if int8:  # the same arms over int8 caches of the same shapes
                        (kp8, kps), (vp8, vps) = _q8(kp.shape), _q8(vp.shape)
                        (ks8, kss), (vs8, vss) = _q8(ks.shape), _q8(vs.shape)
                        kc8, vc8 = (torch.cat([p_.expand(R, -1, -1, -1), s_], dim=2).contiguous() for p_, s_ in ((kp8, ks8), (vp8, vs8)))
                        kcs, vcs = (torch.cat([p_.expand(R, -1, -1), s_], dim=2).contiguous() for p_, s_ in ((kps, kss), (vps, vss)))
                        arms = {"shared": lambda: A.shared_prefix_attention_q8(q, k, v, (kp8, vp8, kps, vps), (ks8, vs8, kss, vss), pt, lt),
                                "replicated": lambda: A.decode_attention(q.unsqueeze(1), kc8, vc8, P + suffix, kcs, vcs, seq_len_dev=lt,
                                                                         k_new=k.unsqueeze(1), v_new=v.unsqueeze(1))}
                    outs = {n_: f() for n_, f in arms.items()}
                    diff = (outs["shared"].float() - outs["replicated"].view(R, -1).float()).abs().max().item()
                    for f in arms.values():
                        timed(f, 3)
                    us = {n_: [] for n_ in arms}
                    for _ in range(rounds):
                        for n_, f in arms.items():
                            us[n_].append(timed(f, iters))
                    emit({"cache": "int8" if int8 else "bf16", "shape": name, "H": H, "Hkv": Hkv, "D": D, "R": R, "prefix": P, "suffix": suffix,
                          "splits": kernels().shared_prefix_plan(R, H, Hkv, D, P)[3], "max_abs_diff": round(diff, 5),
                          **{n_ + "_us": stats(x) for n_, x in us.items()}})


def e2e_rows(rounds, emit):
    from penroz.models import kv_cache as kvc
    from penroz.models.mapper import Mapper
    from penroz.models.model import NeuralNetworkModel
    for name, layers, block, plen in (("gpt2", B_.gpt2_layers(), 1024, 896), ("gemma3-1b", B_.gemma3_1b_layers(), 2048, 1024)):
        torch.manual_seed(0)
        model = NeuralNetworkModel("sp-" + name, Mapper(layers, {"adamw": {"lr": 1e-3}})).to(DEV)
        model.to(dtype=BF)
        prompt = torch.randint(0, 50000, (plen,)).tolist()
        for R in ROWS:
            def call(shared, new):
                if shared:
                    return lambda: model.generate_batch(prompt, block, new, temperature=1.0, top_k=50, n=R)
                return lambda: model.generate_batch([prompt] * R, block, new, temperature=1.0, top_k=50)
            arms = {(k_, new): call(k_ == "shared", new) for k_ in ("shared", "replicated") for new in (1, 2, 66)}
            for f in arms.values():
                f(), f()
            ms = {a_: [] for a_ in arms}
            for _ in range(rounds):
                for a_, f in arms.items():
                    ms[a_].append(timed(f, 1) / 1e3)
            row = {"e2e": name, "cache": "int8" if kvc.TURBO_QUANT_ENABLED else "bf16", "prompt": plen, "R": R}
            for k_ in ("shared", "replicated"):
                med = {new: statistics.median(ms[(k_, new)]) for new in (1, 2, 66)}
                row[k_ + "_ttft_ms"] = stats(ms[(k_, 1)])
                row[k_ + "_ms_per_step"] = round((med[66] - med[2]) / 64, 4)  # graph replays only
            emit(row)
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)  # a window of 2-8 ms at 10-40 µs a launch
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--int8", action="store_true")
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

    if a.int8:
        from penroz.models import kv_cache as kvc
        kvc.TURBO_QUANT_ENABLED = True
    attention_rows(a.rounds, a.iters, emit, a.int8)
    if not a.no_e2e:
        e2e_rows(a.rounds, emit)


if __name__ == "__main__":
    main()
