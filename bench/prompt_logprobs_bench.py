"""Prompt scoring (csrc/kernels/lmhead_lse.hip): six arms alternating in one process —
(a) the fused kernel through ``ops.prompt_logprobs.score_rows``; (b) the route it replaces: hipBLASLt
``h · Wᵀ`` to bf16 logits, fp32 ``log_softmax``, ``gather``, ``max``; (c) hipBLASLt's GEMM alone, the
floor for the matrix work; (d, e) the kernel's top-n form, ``score_rows(..., top_n=5 / 20)``; (f) the route
that replaces: (b)'s GEMM and ``log_softmax``, then ``topk(20)``. Every arm is warmed up; a round times ``--iters`` calls between two
synchronises; the median and the min-max spread of ``--rounds`` rounds are reported, with TF/s from
2·N·V·C and each arm's peak extra device memory (``torch.cuda.max_memory_allocated`` over one call,
above what the operands hold). The arms' outputs are compared once per shape.

    python bench/prompt_logprobs_bench.py [--rounds 7] [--iters 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from penroz.ops import prompt_logprobs as plp  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
# (name, C, V) x N
HEADS = [("gpt2-124m", 768, 50257), ("gpt2-124m-padded", 768, 50304), ("gemma3-1b", 1152, 262144)]
ROWS = [128, 1024, 4096]


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def stats(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = open(a.out, "w") if a.out else None
    for name, C, V in HEADS:
        torch.manual_seed(0)
        W = (torch.randn(V, C, device=DEV) / C ** 0.5).to(BF)
        for N in ROWS:
            h = torch.randn(N, C, device=DEV).to(BF)
            t = torch.randint(0, V, (N,), device=DEV)
            assert plp.kernel_takes(h, W), "the fused arm must run the kernel"

            def fused():
                return plp.score_rows(h, W, None, t)

            def unfused():
                lsm = torch.log_softmax((h @ W.T).float(), dim=-1)
                best = lsm.max(dim=-1)
                return lsm.gather(1, t.unsqueeze(1)).squeeze(1), best.indices, best.values

            def gemm():
                return h @ W.T

            def unfused_top20():
                lsm = torch.log_softmax((h @ W.T).float(), dim=-1)
                best = lsm.topk(20, dim=-1)
                return lsm.gather(1, t.unsqueeze(1)).squeeze(1), best.indices, best.values

            arms = {"fused": fused, "unfused": unfused, "gemm": gemm,
                    "fused_top5": lambda: plp.score_rows(h, W, None, t, 5),
                    "fused_top20": lambda: plp.score_rows(h, W, None, t, 20), "unfused_top20": unfused_top20}
            got, ref = fused(), unfused()
            diff = (got[0] - ref[0]).abs().max().item()  # (the unfused route rounds its logits to bf16)
            top20 = arms["fused_top20"]()
            assert torch.equal(top20[3][:, 0], top20[1]) and (top20[4][:, 1:] <= top20[4][:, :-1]).all()
            mem = {k: peak_extra_mib(f) for k, f in arms.items()}
            for f in arms.values():
                timed(f, 2)
            us = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, f in arms.items():
                    us[k].append(timed(f, a.iters))
            fl = 2.0 * N * V * C
            row = {"head": name, "C": C, "V": V, "N": N, "plan": list(plp.kernels().lmhead_lse_plan(N, V, C)),
                   "plan_top_n": list(plp.kernels().lmhead_lse_plan(N, V, C, 0, 20)),
                   "max_abs_diff_vs_unfused": round(diff, 5)}
            for k in arms:
                row[k + "_us"] = stats(us[k])
                row[k + "_TF"] = round(fl / statistics.median(us[k]) / 1e6, 1)
                row[k + "_extra_MiB"] = mem[k]
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del h, t
        del W
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
