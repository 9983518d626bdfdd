"""Per-kernel time of the Gemma-3 1B / GPT-2 decode GEMVs, bf16 weights (decode_gemv /
decode_gemv_pair) vs int8 weights (decode_gemv_q8 / decode_gemv_q8_pair), over the rows-per-wave /
pairs-per-wave variants (0: the launch plan's choice). Each shape cycles through enough weight
copies to exceed the 256 MiB cache; the loop over the copies is captured in a graph and replayed.

python bench/decode_gemv_q8_bench.py [ROWS=1]
Prints one JSON line per shape: µs per launch (best of 5 replays) and weight TB/s per variant
(profiles/decode_int8_weights.md)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from penroz.ops import _ext

K_ = _ext.kernels()
DEV = "cuda"
M = int(sys.argv[1]) if len(sys.argv) > 1 else 1


def bench(fn_of_copy, ncopy, reps=5):
    for c in range(ncopy):
        fn_of_copy(c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in range(ncopy):
            fn_of_copy(c)
    g.replay()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / ncopy)
    return best * 1e6


def run(name, N, K, kind):
    ncopy = max(4, min(400, int(700e6 / (N * K * 2)) + 1))
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    wb = [(torch.randn(N, K, device=DEV) * 0.02).to(torch.bfloat16) for _ in range(ncopy)]
    wq = [(torch.randint(-127, 128, (N, K), device=DEV, dtype=torch.int8), torch.rand(N, device=DEV)) for _ in range(ncopy)]
    D = 256
    cos = torch.rand(1, D // 2, device=DEV); sin = torch.rand(1, D // 2, device=DEV)
    n_out = N // 2 if kind == "gated" else N
    out = torch.empty(M, n_out, device=DEV, dtype=torch.bfloat16)
    res = {}
    if kind == "plain":
        for rpw in (0, 2, 4, 8):
            res[f"bf16 rpw{rpw}"] = bench(lambda c: K_.decode_gemv(x, None, None, None, None, None, None, 0.0, wb[c], None, out, 0, rpw), ncopy)
            res[f"int8 rpw{rpw}"] = bench(lambda c: K_.decode_gemv_q8(x, None, None, None, None, None, None, 0.0, wq[c][0], wq[c][1], None, out, 0, rpw), ncopy)
    else:
        mode = 1 if kind == "gated" else 2
        for ppw in (0, 1, 2, 4):
            res[f"bf16 ppw{ppw}"] = bench(lambda c: K_.decode_gemv_pair(x, wb[c], out, mode, 1, D, 5, cos, sin, ppw), ncopy)
            res[f"int8 ppw{ppw}"] = bench(lambda c: K_.decode_gemv_q8_pair(x, wq[c][0], wq[c][1], out, mode, 1, D, 5, cos, sin, ppw), ncopy)
    line = {"shape": name, "M": M, "N": N, "K": K, "copies": ncopy,
            "us": {k: round(v, 2) for k, v in res.items()},
            "TBps": {k: round((N * K * (2 if k.startswith("bf16") else 1)) / v / 1e6, 2) for k, v in res.items()}}
    print(json.dumps(line), flush=True)


run("gemma gate|up", 13824, 1152, "gated")
run("gemma qkv", 1536, 1152, "rope")
run("gemma o", 1152, 1024, "plain")
run("gemma down", 1152, 6912, "plain")
run("gemma head", 262144, 1152, "plain")
run("gpt2 fc2", 768, 3072, "plain")
run("gpt2 proj", 768, 768, "plain")
