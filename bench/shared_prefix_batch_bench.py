"""share_prefix (ops/shared_prefix.py): a batch of different prompts that begin with the same tokens, against the plain
ragged call on the same prompts — the arms alternate in one process, every arm is warmed up, a round times `--iters`
launches between two synchronises, and the median and the min-max spread of `--rounds` rounds are reported.

Attention alone, one layer, remainders padded to 64 positions:
  kernel:  the prefill form of shared_prefix_attn.hip against prefill_attention at offset P on the replicated cache of
           the same content (its arm stores the rows' K/V itself as well) — the same queries and keys;
  prompt:  all the attention of a prompt pass — plain: R rows of P + 64 positions; shared: the prefix once, then the kernel.
Then generate_batch(share_prefix=True) against the plain call: time to the first token and ms per decode step (from
two call lengths), remainders spread over [16, 64].

    python bench/shared_prefix_batch_bench.py [--rounds 7] [--iters 20] [--no-e2e] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench as B_  # noqa: E402
from shared_prefix_bench import BF, DEV, GEMMA, GPT2, stats, timed  # noqa: E402
from penroz.ops import attention as A  # noqa: E402
from penroz.ops import sampling as S_  # noqa: E402
from penroz.ops._ext import kernels  # noqa: E402

SHAPES = [("gpt2", GPT2, (128, 1024, 4096)), ("gemma3-1b", GEMMA, (128, 1024, 4096))]
ROWS, TQ = (16, 64), 64


def attention_rows(rounds, iters, emit):
    for name, (H, Hkv, D), prefixes in SHAPES:
        for P in prefixes:
            for R in ROWS:
                torch.manual_seed(0)
                W = (H + 2 * Hkv) * D
                full = torch.randn(R, P + TQ, W, device=DEV, dtype=BF)  # the plain call's QKV rows
                full[:, :P] = full[:1, :P]                              # (the rows agree on the prefix)
                views = lambda x: [t.view(*x.shape[:2], -1, D) for t in x.split([H * D, Hkv * D, Hkv * D], dim=2)]
                qf, kf, vf = views(full)
                q, k, v = views(full[:, P:].contiguous())    # the shared call's: the remainders' rows,
                q1, k1, v1 = views(full[:1, :P].contiguous())  # and the one prefix
                kp, vp = (torch.empty(1, Hkv, P, D, device=DEV, dtype=BF) for _ in range(2))
                ks, vs = (torch.empty(R, Hkv, 128, D, device=DEV, dtype=BF) for _ in range(2))
                kc, vc = (torch.empty(R, Hkv, P + TQ, D, device=DEV, dtype=BF) for _ in range(2))
                pt = torch.tensor([P], device=DEV)

                def store(kn, vn, kd, vd, pos):
                    S_.kv_store_into(kn, kd, pos)
                    S_.kv_store_into(vn, vd, pos)

                def plain_kernel():
                    store(k, v, kc, vc, P)
                    return A.prefill_attention(q, kc, vc, P + TQ)

                def plain_prompt():
                    store(kf, vf, kc, vc, 0)
                    return A.prefill_attention(qf, kc, vc, P + TQ)

                def shared_prompt():
                    store(k1, v1, kp, vp, 0)
                    A.prefill_attention(q1, kp, vp, P)
                    return A.shared_prefix_prefill_attention(q, k, v, kp, vp, ks, vs, pt)

                arms = {"plain_prompt": plain_prompt, "shared_prompt": shared_prompt, "plain_kernel": plain_kernel,
                        "shared_kernel": lambda: A.shared_prefix_prefill_attention(q, k, v, kp, vp, ks, vs, pt)}
                outs = {n_: f() for n_, f in arms.items()}
                diff = (outs["shared_kernel"].float() - outs["plain_kernel"].float()).abs().max().item()
                for f in arms.values():
                    timed(f, 2)
                us = {n_: [] for n_ in arms}
                for _ in range(rounds):
                    for n_, f in arms.items():
                        us[n_].append(timed(f, iters))
                plan = kernels().shared_prefix_prefill_plan(R, TQ, H, Hkv, D, P, 128)
                emit({"shape": name, "H": H, "Hkv": Hkv, "D": D, "R": R, "prefix": P, "Tq": TQ, "tile_rows": plan[1],
                      "splits": plan[4], "max_abs_diff": round(diff, 5), **{n_ + "_us": stats(x) for n_, x in us.items()}})
                del full, kc, vc
                torch.cuda.empty_cache()


def e2e_rows(rounds, emit):
    import statistics as st
    from penroz.models.mapper import Mapper
    from penroz.models.model import NeuralNetworkModel
    for name, layers, block, plen in (("gpt2", B_.gpt2_layers(), 1024, 880), ("gemma3-1b", B_.gemma3_1b_layers(), 2048, 1024)):
        torch.manual_seed(0)
        model = NeuralNetworkModel("spb-" + name, Mapper(layers, {"adamw": {"lr": 1e-3}})).to(DEV)
        model.to(dtype=BF)
        head = torch.randint(0, 50000, (plen,)).tolist()
        for R in ROWS:
            prompts = [head + torch.randint(0, 50000, (16 + (48 * b) // (R - 1),)).tolist() for b in range(R)]

            def call(shared, new):
                return lambda: model.generate_batch(prompts, block, new, temperature=1.0, top_k=50, share_prefix=shared or None)
            arms = {(k_, new): call(k_ == "shared", new) for k_ in ("shared", "plain") for new in (1, 2, 66)}
            for f in arms.values():
                f(), f()
            ms = {a_: [] for a_ in arms}
            for _ in range(rounds):
                for a_, f in arms.items():
                    ms[a_].append(timed(f, 1) / 1e3)
            call(True, 2)()
            row = {"e2e": name, "prefix": plen, "R": R, "ran_shared": model.last_shared_prefix is not None}
            for k_ in ("shared", "plain"):
                med = {new: st.median(ms[(k_, new)]) for new in (1, 2, 66)}
                row[k_ + "_ttft_ms"] = stats(ms[(k_, 1)])
                row[k_ + "_ms_per_step"] = round((med[66] - med[2]) / 64, 4)  # graph replays only
            emit(row)
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)  # a launch is 0.1-20 ms here
    ap.add_argument("--no-e2e", action="store_true")
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
    if not a.no_e2e:
        e2e_rows(a.rounds, emit)


if __name__ == "__main__":
    main()
