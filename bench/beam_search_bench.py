"""Beam search (csrc/kernels/beam_search.hip). The arms of every comparison alternate in one process, every arm is
warmed up, a round times its launches between two synchronises, and the median and the min-max spread of
`--rounds` rounds are reported.

  step     generate_tokens(num_beams = W) against generate_batch(n = W) — the same shared-prefix step with the
           sampler in beam_step's and beam_reorder's place — as ms per decode step, from two call lengths that
           share one suffix capacity (66 and 126 new tokens), GPT-2 124M shape, W = 4 and 8;
  select   beam_step's two launches against the sampler (sample_tokens) plus token_logprobs (n = 16) on the same
           [W, V] logits. Both comparison kernels are the eager entry points, which allocate their outputs;
  reorder  beam_reorder at W = 8 over the GPT-2 124M suffix caches (12 layers, 12 KV heads, D = 64) with 128 and
           1024 slots in use, a cyclic parent: µs and bytes moved (read + written) per second.

    python bench/beam_search_bench.py [--rounds 7] [--iters 200] [--no-e2e] [--out FILE]
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
from penroz.ops import beam_search as bs  # noqa: E402
from penroz.ops._ext import kernels  # noqa: E402

DEV, BF = "cuda", torch.bfloat16


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def stats(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def alternate(arms, rounds, iters):
    for f in arms.values():
        timed(f, 3)
    us = {n_: [] for n_ in arms}
    for _ in range(rounds):
        for n_, f in arms.items():
            us[n_].append(timed(f, iters))
    return us


def select_rows(rounds, iters, emit):
    K = kernels()
    for V in (50257, 262144):
        for W in (4, 8):
            torch.manual_seed(0)
            logits = (torch.randn(W, V, device=DEV) * 3).to(BF)
            st = bs.BeamState(W, 64, V, DEV)
            idx = torch.zeros(W, dtype=torch.long, device=DEV)
            u = torch.rand(W, device=DEV)

            def beam():
                st.step(logits, idx)

            def sampler():
                tok = K.sample_tokens(logits, u, 1.0, 0)
                K.token_logprobs(logits, tok, 16)

            def rearm(f):  # (the step index never reaches T: every launch does the whole step; one small copy in both arms)
                def g():
                    st.buf[:72].copy_(head)
                    f()
                return g
            st.begin(64, 7, 1.0, rows=W, cum=[-1.0] * W, step=1)
            head = st.buf[:72].clone()
            us = alternate({"beam_step": rearm(beam), "sampler_logprobs": rearm(sampler)}, rounds, iters)
            emit({"select": True, "V": V, "W": W, **{n_ + "_us": stats(x) for n_, x in us.items()}})


def reorder_rows(rounds, iters, emit):
    W, L, Hkv, D = 8, 12, 12, 64
    for n in (128, 1024):
        ks = [torch.randn(W, Hkv, n, D, device=DEV).to(BF) for _ in range(L)]
        vs = [torch.randn(W, Hkv, n, D, device=DEV).to(BF) for _ in range(L)]
        table = bs.ReorderTable(ks, vs)
        parent = torch.tensor([(r + 1) % W for r in range(W)], dtype=torch.int32, device=DEV)
        n_t = torch.tensor([n], dtype=torch.int32, device=DEV)
        us = alternate({"reorder": lambda: table.apply(parent, n_t)}, rounds, iters)["reorder"]
        moved = 2 * 2 * L * W * Hkv * n * D * 2  # read + written, K and V
        emit({"reorder": True, "W": W, "slots": n, "bytes_moved": moved, "us": stats(us),
              "GB_per_s": round(moved / statistics.median(us) / 1e3, 1)})


def step_rows(rounds, emit):
    from penroz.models.mapper import Mapper
    from penroz.models.model import NeuralNetworkModel
    torch.manual_seed(0)
    model = NeuralNetworkModel("beam-gpt2", Mapper(B_.gpt2_layers(), {"adamw": {"lr": 1e-3}})).to(DEV)
    model.to(dtype=BF)
    prompt, block = torch.randint(0, 50000, (512,)).tolist(), 1024
    for W in (4, 8):
        arms = {}
        for new in (66, 126):
            arms[("beam", new)] = lambda new=new: model.generate_tokens([prompt], block, new, num_beams=W)
            arms[("n", new)] = lambda new=new: model.generate_batch(prompt, block, new, temperature=1.0, n=W)
        ms = {a_: [t / 1e3 for t in x] for a_, x in alternate(arms, rounds, 1).items()}
        row = {"step": "gpt2", "prompt": len(prompt), "W": W, "path": model.last_beam_search["path"]}
        for k_ in ("beam", "n"):
            med = {new: statistics.median(ms[(k_, new)]) for new in (66, 126)}
            row[k_ + "_ms_per_step"] = round((med[126] - med[66]) / 60, 4)  # graph replays only
            row[k_ + "_call_ms_126"] = stats(ms[(k_, 126)])
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
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

    select_rows(a.rounds, a.iters, emit)
    reorder_rows(a.rounds, a.iters, emit)
    if not a.no_e2e:
        step_rows(a.rounds, emit)


if __name__ == "__main__":
    main()
