"""KV-cache decode throughput, random weights, one MI355X: GPT-2 124M (reference example layout)
or a Gemma-3 1B shaped model (RoPE, GQA 4:1, head_dim 256, 262k vocab; HF config builder).

python bench/bench_decode.py [--model gpt2|gemma3-1b] [--batch 64] [--prompt 64] [--new 128] [--turbo]
                             [--top-k 50] [--top-p P] [--min-p P]      (--top-k 0: no top-k)
                             [--weights bf16|int8] [--ab ROUNDS]
                             [--repetition-penalty R] [--presence-penalty P] [--frequency-penalty F]
                             [--ab-penalties ROUNDS]
                             [--logprobs N[,N...]] [--ab-logprobs ROUNDS]
                             [--stop IDS[/IDS...]] [--ab-stop ROUNDS]
                             [--logit-bias N] [--allowed N] [--ab-bias ROUNDS]
                             [--ragged ROUNDS]
                             [--speculate K[,K...]] [--rounds ROUNDS] [--copy-model]
Prints one JSON line: generated tokens/s over all rows (BASELINE config 4: batch 64 /generate).
--weights int8: the batch 1-4 decode steps read int8 weight copies (ops/weight_quant.py). --ab ROUNDS:
both weight formats on one model in this one process, alternating, ROUNDS timed runs each; the line
then holds both arms (ms/step of every run, median, min, the linears' weight bytes per token and the
rate they were read at) and the int8 / bf16 ratio of the medians.
--repetition-penalty / --presence-penalty / --frequency-penalty: logit penalties (ops/penalties.py) in the
decode step. --ab-penalties ROUNDS: the same process alternates between runs with those penalties and
runs without (one decoder, its two captured graphs), ROUNDS timed runs each; the line holds both arms
and the penalised / plain ratio of the medians.
--logprobs N: per-token log-probabilities with the N most likely tokens (ops/logprobs.py) in the decode
step. --ab-logprobs ROUNDS: the same process alternates between runs without them and runs with every
N listed (one decoder, two captured graphs, N read on the device), ROUNDS timed runs each; the line holds
every arm and its difference to the run without. A run's time includes reading the results back.
--stop IDS: stop sequences (ops/stopping.py), each a comma-separated list of token ids, several divided by
"/", checked on the device at the end of the decode step; the default of --ab-stop is one sequence of eight
ids, which random weights never complete, so every run generates all its tokens. --ab-stop ROUNDS: the same
process alternates between runs without and with the stop check (one decoder, two captured graphs, bursts of
PENROZ_STOP_BURST steps in the second), ROUNDS timed runs each; the line holds both arms, their difference
and how many rows finished early (0 is what the comparison needs).
--logit-bias N: N random logit-bias entries (ops/logit_bias.py; ids drawn without replacement, biases in
[-5, 5]); --allowed N: an allowed set of N random ids; both rewrite the logits in front of the sampler inside
the decode step. --ab-bias ROUNDS: the same process alternates between runs without, with the entries
(default 300) and with the allowed set (default 1000) — one decoder, its three captured graphs — ROUNDS timed
runs each; the line holds every arm, its difference to the run without, and the bytes the mask form stores.
--ragged ROUNDS: the same process alternates between the uniform batch (every prompt --prompt long) and a ragged
one (ops/ragged.py) of the same rows whose prompt lengths are spread evenly over [prompt / 4, prompt] — the same
longest row, so the same padded prefill and capacity — ROUNDS timed runs each; the line holds both arms, their
difference, and whether a ragged decoder's captured graph served the ragged arm. --block >= prompt + new.
--speculate K[,K...]: prompt-lookup speculative decoding (ops/speculative.py) of ONE greedy sequence (--batch is
ignored): the same process alternates between the plain greedy call and a speculative one per K, --rounds timed
pairs of runs each. A run's prefill and fixed costs are taken out by difference: every arm generates --new and
--new / 4 tokens, and ms/step is the time between the two over the steps between the two (greedy: the longer
run repeats the shorter one's steps). Per arm: ms/step, tokens/step and ms/token. --copy-model (gpt2): the
best case — position table, attention output projections and fc2 weights zeroed, vocabulary projection = the
token table, so the argmax is the token fed and every draft is accepted. --block >= prompt + new + K.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.models import kv_cache as KV
import penroz.models.model as M

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--prompt", type=int, default=64)
ap.add_argument("--new", type=int, default=128)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
ap.add_argument("--turbo", action="store_true")
ap.add_argument("--model", default="gpt2", choices=["gpt2", "gemma3-1b"])
# the generation window (block_size): a context longer than it is cropped and re-prefilled every
# token, so long-context rows need --block >= prompt + new
ap.add_argument("--block", type=int, default=1024)
ap.add_argument("--top-k", type=int, default=50, help="0: no top-k")
ap.add_argument("--top-p", type=float, default=None)
ap.add_argument("--min-p", type=float, default=None)
ap.add_argument("--weights", default="bf16", choices=["bf16", "int8"], help="decode weight format")
ap.add_argument("--ab", type=int, default=0, metavar="ROUNDS", help="alternate bf16 and int8 weights, ROUNDS runs each")
ap.add_argument("--repetition-penalty", type=float, default=None)
ap.add_argument("--presence-penalty", type=float, default=None)
ap.add_argument("--frequency-penalty", type=float, default=None)
ap.add_argument("--ab-penalties", type=int, default=0, metavar="ROUNDS",
                help="alternate runs with and without the penalties, ROUNDS runs each")
ap.add_argument("--logprobs", default=None, metavar="N[,N...]",
                help="log-probabilities with the N most likely tokens (0-20); a list for --ab-logprobs")
ap.add_argument("--ab-logprobs", type=int, default=0, metavar="ROUNDS",
                help="alternate runs without log-probabilities and with every N of --logprobs, ROUNDS runs each")
ap.add_argument("--stop", default=None, metavar="IDS[/IDS...]",
                help="stop sequences: comma-separated token ids, several divided by '/'")
ap.add_argument("--ab-stop", type=int, default=0, metavar="ROUNDS",
                help="alternate runs without and with the stop check, ROUNDS runs each")
ap.add_argument("--logit-bias", type=int, default=0, metavar="N", help="N random logit-bias entries (1-1024)")
ap.add_argument("--allowed", type=int, default=0, metavar="N", help="an allowed set of N random token ids")
ap.add_argument("--ab-bias", type=int, default=0, metavar="ROUNDS",
                help="alternate runs without, with the entries and with the allowed set, ROUNDS runs each")
ap.add_argument("--ragged", type=int, default=0, metavar="ROUNDS",
                help="alternate a uniform and a ragged batch (prompt lengths spread over [prompt / 4, prompt]), ROUNDS runs each")
ap.add_argument("--speculate", default=None, metavar="K[,K...]", help="speculative arms (1-3) beside the plain greedy call")
ap.add_argument("--rounds", type=int, default=5, help="--speculate: timed pairs of runs per arm")
ap.add_argument("--copy-model", action="store_true", help="--speculate, gpt2: a model whose argmax is the token it was fed")
a = ap.parse_args()
if a.ab_bias:
    a.logit_bias, a.allowed = a.logit_bias or 300, a.allowed or 1000
if a.ab_stop and not a.stop:
    a.stop = "1,2,3,4,5,6,7,8"
stop_seqs = [[int(t) for t in seq.split(",")] for seq in a.stop.split("/")] if a.stop else None
lp_ns = [int(v) for v in a.logprobs.split(",")] if a.logprobs else []
if a.turbo:
    M.create_kv_cache = lambda n, cap=None: KV.TurboQuantKVCache(n, cap)
torch.manual_seed(0)
if a.model == "gpt2":
    layers, V = bench.gpt2_layers(), 50304
else:  # google/gemma-3-1b-pt text config (shapes only; no checkpoint)
    from types import SimpleNamespace
    V = 262144
    layers = Mapper.from_hf_config(SimpleNamespace(
        model_type="gemma3_text", vocab_size=V, hidden_size=1152, intermediate_size=6912, num_hidden_layers=26,
        num_attention_heads=4, num_key_value_heads=1, head_dim=256, rms_norm_eps=1e-6, rope_theta=1e6,
        rope_local_base_freq=10000.0, attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh",
        query_pre_attn_scalar=256, sliding_window=512))
m = NeuralNetworkModel("dec", Mapper(layers, {"adamw": {"lr": 6e-4}})).to("cuda")
if a.dtype == "bf16":
    m.to(dtype=torch.bfloat16)
if a.copy_model:
    assert a.model == "gpt2", "--copy-model: gpt2 only"
    from penroz.models.executor import GPTExecutor
    sp = GPTExecutor.match(m)
    with torch.no_grad():
        sp.wpe.weight.zero_()
        for b in sp.blocks:
            b.proj.weight.zero_()
            b.fc2.weight.zero_()
        sp.head.weight.copy_(sp.wte.weight)
ctx = torch.randint(0, V, (a.batch, a.prompt)).tolist()
samp = dict(temperature=1.0, top_k=a.top_k or None, top_p=a.top_p, min_p=a.min_p)
pens = dict(repetition_penalty=a.repetition_penalty, presence_penalty=a.presence_penalty,
            frequency_penalty=a.frequency_penalty)
g_bias = torch.Generator().manual_seed(1)
bias_entries = ({int(i): float(b) for i, b in zip(torch.randperm(V, generator=g_bias)[:a.logit_bias].tolist(),
                                                  torch.empty(a.logit_bias).uniform_(-5, 5, generator=g_bias).tolist())}
                if a.logit_bias else None)
allowed_ids = torch.randperm(V, generator=g_bias)[:a.allowed].tolist() if a.allowed else None


early = 0  # rows of the last timed() run that a stop sequence finished


def timed(weights: str, new: int, penalised: bool = True, logprobs: int | None = None, stop=None,
          logit_bias=None, allowed=None, context=None) -> float:
    """Seconds of one generate_batch of ``new`` tokens with this weight format ("" selects bf16
    whatever PENROZ_DECODE_WEIGHTS says), with the command line's penalties or without any, with
    ``logprobs`` (None: without), with the stop sequences ``stop`` (None: without) and with the logit-bias
    entries ``logit_bias`` / the allowed ids ``allowed`` (None: without). ``context``: the prompts (None: the
    uniform batch)."""
    global early
    kw = {} if stop is None else {"stop": stop}
    if logit_bias is not None:
        kw["logit_bias"] = logit_bias
    if allowed is not None:
        kw["allowed_token_ids"] = allowed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.generate_batch(ctx if context is None else context, a.block, new, weight_quant="int8" if weights == "int8" else "", **samp,
                           **(pens if penalised else {}), logprobs=logprobs, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    early = sum(i["finish_reason"] == "stop" for i in out[1]) if stop is not None else 0
    return dt


def weight_bytes(weights: str) -> int:
    """Bytes of linear weights one decode step reads: every nn.Linear once (bf16: 2 per weight;
    int8: 1 per weight + one fp32 scale per row)."""
    lins = [mod.weight for mod in m.modules() if isinstance(mod, torch.nn.Linear)]
    if weights == "int8":
        return sum(w.numel() + 4 * w.shape[0] for w in lins)
    return sum(w.numel() * w.element_size() for w in lins)


def in_effect() -> list:
    return sorted({d.weight_quant or "bf16" for d in m.__dict__.get("_graph_decoders", {}).values()})


if a.speculate:
    ks = [int(v) for v in a.speculate.split(",")]
    assert a.block >= a.prompt + a.new + max(ks), "--speculate: --block >= prompt + new + K"
    short = max(1, a.new // 4)
    wq = "int8" if a.weights == "int8" else ""

    def spec_run(k: int, new: int):
        """(seconds, decode steps, tokens) of one greedy one-row call; k = 0: the plain call."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate_tokens(ctx[:1], a.block, new, temperature=0.0, weight_quant=wq, speculate=k or None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, (m.last_speculation["steps"] if k else new), out

    arms = {k: [] for k in [0] + ks}
    ref = None
    for k in arms:  # warmup: every arm's decoder and graph captured (the cache keeps two decoders: re-captured per switch)
        out = spec_run(k, a.new)[2]
        ref = out if ref is None else ref
        diff = next((i for i, (x, y) in enumerate(zip(out, ref)) if x != y), None)  # (a near-tie, flipped: random weights)
        arms[k] = {"same_tokens_as_plain": out == ref, "first_difference_at": diff, "ms_per_step": [], "tokens_per_step": [], "ms_per_token": [],
                   "run_ms": []}
    for _ in range(a.rounds):
        for k, res in arms.items():  # alternating: every arm sees the same drift of clocks and neighbours
            spec_run(k, short)  # (this arm's decoder is the cached one again: its capture is not timed below)
            t1, s1, _ = spec_run(k, short)
            t2, s2, _ = spec_run(k, a.new)
            res["ms_per_step"].append((t2 - t1) / (s2 - s1) * 1e3)
            res["tokens_per_step"].append((a.new - short) / (s2 - s1))
            res["ms_per_token"].append((t2 - t1) / (a.new - short) * 1e3)
            res["run_ms"].append(t2 * 1e3)
        stats = dict(m.last_speculation or {})
    out = {}
    for k, res in arms.items():
        o = {"same_tokens_as_plain": res["same_tokens_as_plain"], "first_difference_at": res["first_difference_at"]}
        for key in ("ms_per_step", "tokens_per_step", "ms_per_token", "run_ms"):
            v = sorted(res[key])
            o[key] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        out["plain" if k == 0 else f"k={k}"] = o
    base = out["plain"]["ms_per_step"]["median"]
    for name, o in out.items():
        # extra tokens per step at which the arm's step costs what that many plain steps cost
        o["break_even_extra_tokens_per_step"] = round(o["ms_per_step"]["median"] / base - 1, 4)
    print(json.dumps({"metric": "greedy one-row decode, plain vs speculative, alternating in one process; prefill and "
                                "fixed costs removed by differencing runs of --new and --new / 4 tokens",
                      "arms": out, "last_arm_speculation": stats, "copy_model": a.copy_model, "prompt": a.prompt,
                      "new_tokens": a.new, "short_run": short, "block": a.block, "rounds": a.rounds, "weights": a.weights,
                      "weights_in_effect": in_effect(), "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
if a.ab:
    arms = {"bf16": [], "int8": []}
    for w in arms:
        timed(w, 4)  # warmup: quantised copies, graph capture
    effect = in_effect()
    for _ in range(a.ab):
        for w in arms:  # alternating: both arms see the same drift of clocks and neighbours
            arms[w].append(timed(w, a.new) / a.new * 1e3)
    res = {}
    for w, ms in arms.items():
        med = sorted(ms)[len(ms) // 2]
        res[w] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(med, 4), "min": round(min(ms), 4),
                  "weight_bytes_per_token": weight_bytes(w),
                  "weight_tb_per_s_at_median": round(weight_bytes(w) / (med * 1e-3) / 1e12, 3)}
    print(json.dumps({"metric": "decode ms/step, bf16 vs int8 weights, alternating in one process", "arms": res,
                      "int8_over_bf16_median": round(res["int8"]["median"] / res["bf16"]["median"], 4),
                      "weights_in_effect": effect, "batch": a.batch, "prompt": a.prompt, "new_tokens": a.new,
                      "block": a.block, "rounds": a.ab, "top_k": a.top_k or None,
                      "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
if a.ab_penalties:
    from penroz.ops.penalties import check_penalties
    assert check_penalties(**pens) is not None, "--ab-penalties needs a penalty that is not neutral"
    arms = {"plain": [], "penalised": []}
    for arm in arms:
        timed(a.weights, 4, arm == "penalised")  # warmup: both graphs of the one decoder captured
    for _ in range(a.ab_penalties):
        for arm in arms:  # alternating: both arms see the same drift of clocks and neighbours
            arms[arm].append(timed(a.weights, a.new, arm == "penalised") / a.new * 1e3)
    res = {}
    for arm, ms in arms.items():
        med = sorted(ms)[len(ms) // 2]
        res[arm] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(med, 4), "min": round(min(ms), 4)}
    decs = list(m.__dict__.get("_graph_decoders", {}).values())
    print(json.dumps({"metric": "decode ms/step, with vs without logit penalties, alternating in one process",
                      "arms": res, "penalised_over_plain_median": round(res["penalised"]["median"] / res["plain"]["median"], 4),
                      "penalised_minus_plain_us": round((res["penalised"]["median"] - res["plain"]["median"]) * 1e3, 2),
                      **pens, "decoders": len(decs), "batch": a.batch, "prompt": a.prompt, "new_tokens": a.new,
                      "block": a.block, "rounds": a.ab_penalties, "top_k": a.top_k or None, "top_p": a.top_p,
                      "min_p": a.min_p, "weights": a.weights, "weights_in_effect": in_effect(),
                      "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
if a.ab_logprobs:
    assert lp_ns, "--ab-logprobs needs --logprobs N[,N...]"
    arms = {None: [], **{n: [] for n in lp_ns}}
    for arm in arms:
        timed(a.weights, 4, logprobs=arm)  # warmup: both graphs of the one decoder captured
    for _ in range(a.ab_logprobs):
        for arm in arms:  # alternating: every arm sees the same drift of clocks and neighbours
            arms[arm].append(timed(a.weights, a.new, logprobs=arm) / a.new * 1e3)
    res = {}
    for arm, ms in arms.items():
        med = sorted(ms)[len(ms) // 2]
        res["off" if arm is None else f"n={arm}"] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(med, 4),
                                                     "min": round(min(ms), 4)}
    for k, v in res.items():
        v["minus_off_us"] = round((v["median"] - res["off"]["median"]) * 1e3, 2)
    decs = list(m.__dict__.get("_graph_decoders", {}).values())
    print(json.dumps({"metric": "decode ms/step, without vs with log-probabilities, alternating in one process",
                      "arms": res, **pens, "decoders": len(decs), "batch": a.batch, "prompt": a.prompt,
                      "new_tokens": a.new, "block": a.block, "rounds": a.ab_logprobs, "top_k": a.top_k or None,
                      "top_p": a.top_p, "min_p": a.min_p, "weights": a.weights, "weights_in_effect": in_effect(),
                      "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
if a.ab_stop:
    arms = {"off": [], "on": []}
    finished = 0
    for arm in arms:
        timed(a.weights, 4, stop=stop_seqs if arm == "on" else None)  # warmup: both graphs of the one decoder captured
    for _ in range(a.ab_stop):
        for arm in arms:  # alternating: both arms see the same drift of clocks and neighbours
            arms[arm].append(timed(a.weights, a.new, stop=stop_seqs if arm == "on" else None) / a.new * 1e3)
            finished += early
    res = {}
    for arm, ms in arms.items():
        med = sorted(ms)[len(ms) // 2]
        res[arm] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(med, 4), "min": round(min(ms), 4)}
    decs = list(m.__dict__.get("_graph_decoders", {}).values())
    print(json.dumps({"metric": "decode ms/step, without vs with the stop check, alternating in one process",
                      "arms": res, "on_minus_off_us": round((res["on"]["median"] - res["off"]["median"]) * 1e3, 2),
                      "on_minus_off_min_us": round((res["on"]["min"] - res["off"]["min"]) * 1e3, 2),
                      "stop": stop_seqs, "rows_finished_early": finished, "stop_burst": M._stop_burst(), **pens,
                      "decoders": len(decs), "batch": a.batch, "prompt": a.prompt, "new_tokens": a.new,
                      "block": a.block, "rounds": a.ab_stop, "top_k": a.top_k or None, "top_p": a.top_p,
                      "min_p": a.min_p, "weights": a.weights, "weights_in_effect": in_effect(),
                      "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
if a.ab_bias:
    arms = {"off": {}, "entries": {"logit_bias": bias_entries}, "allowed": {"allowed": allowed_ids}}
    times = {arm: [] for arm in arms}
    for arm, kw in arms.items():
        timed(a.weights, 4, **kw)  # warmup: the three graphs of the one decoder captured
    for _ in range(a.ab_bias):
        for arm, kw in arms.items():  # alternating: every arm sees the same drift of clocks and neighbours
            times[arm].append(timed(a.weights, a.new, **kw) / a.new * 1e3)
    res = {}
    for arm, ms in times.items():
        med = sorted(ms)[len(ms) // 2]
        res[arm] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(med, 4), "min": round(min(ms), 4)}
    for v in res.values():
        v["minus_off_us"] = round((v["median"] - res["off"]["median"]) * 1e3, 2)
        v["minus_off_min_us"] = round((v["min"] - res["off"]["min"]) * 1e3, 2)
    decs = list(m.__dict__.get("_graph_decoders", {}).values())
    elem = 2 if a.dtype == "bf16" else 4
    print(json.dumps({"metric": "decode ms/step, without vs with the logit-bias rewrite, alternating in one process",
                      "arms": res, "entries": a.logit_bias, "allowed_ids": a.allowed,
                      "mask_bytes_stored_per_step": a.batch * (V - a.allowed) * elem, **pens, "decoders": len(decs),
                      "batch": a.batch, "prompt": a.prompt, "new_tokens": a.new, "block": a.block, "rounds": a.ab_bias,
                      "top_k": a.top_k or None, "top_p": a.top_p, "min_p": a.min_p, "weights": a.weights,
                      "weights_in_effect": in_effect(), "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
if a.ragged:
    assert a.block >= a.prompt + a.new, "--ragged: a ragged call never slides its window (--block >= prompt + new)"
    lo = max(1, a.prompt // 4)
    lens = [lo + round((a.prompt - lo) * b / max(1, a.batch - 1)) for b in range(a.batch)]
    arms = {"uniform": ctx, "ragged": [row[:n] for row, n in zip(ctx, lens)]}
    times = {arm: [] for arm in arms}
    for arm, rows in arms.items():
        timed(a.weights, 4, context=rows)  # warmup: each arm's decoder and graph captured
    for _ in range(a.ragged):
        for arm, rows in arms.items():  # alternating: both arms see the same drift of clocks and neighbours
            times[arm].append(timed(a.weights, a.new, context=rows) / a.new * 1e3)
    res = {}
    for arm, ms in times.items():
        med = sorted(ms)[len(ms) // 2]
        res[arm] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(med, 4), "min": round(min(ms), 4)}
    decs = list(m.__dict__.get("_graph_decoders", {}).values())
    print(json.dumps({"metric": "decode ms/step (prefill included), uniform vs ragged batch, alternating in one process",
                      "arms": res, "ragged_minus_uniform_us": round((res["ragged"]["median"] - res["uniform"]["median"]) * 1e3, 2),
                      "ragged_minus_uniform_min_us": round((res["ragged"]["min"] - res["uniform"]["min"]) * 1e3, 2),
                      "ragged_over_uniform_median": round(res["ragged"]["median"] / res["uniform"]["median"], 4),
                      "prompt_lengths": [min(lens), max(lens)],
                      "ragged_graph": any(getattr(d, "ragged", False) and d.graph is not None for d in decs), **pens,
                      "batch": a.batch, "prompt": a.prompt, "new_tokens": a.new, "block": a.block, "rounds": a.ragged,
                      "top_k": a.top_k or None, "top_p": a.top_p, "min_p": a.min_p, "weights": a.weights,
                      "weights_in_effect": in_effect(), "kv_cache": "int8-turboquant" if a.turbo else a.dtype,
                      "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
    sys.exit(0)
lp_n = lp_ns[0] if lp_ns else None
bias_kw = dict(logit_bias=bias_entries, allowed=allowed_ids)
timed(a.weights, 4, logprobs=lp_n, stop=stop_seqs, **bias_kw)  # warmup
dt = timed(a.weights, a.new, logprobs=lp_n, stop=stop_seqs, **bias_kw)
print(json.dumps({"metric": "decode tokens/sec (all rows)", "value": a.batch * a.new / dt, "batch": a.batch,
                  "prompt": a.prompt, "new_tokens": a.new, "block": a.block, "ms_per_step": dt / a.new * 1e3, "dtype": a.dtype,
                  "top_k": a.top_k or None, "top_p": a.top_p, "min_p": a.min_p, **pens, "logprobs": lp_n,
                  "stop": stop_seqs, "logit_bias_entries": a.logit_bias, "allowed_ids": a.allowed, "weights": a.weights, "weights_in_effect": in_effect(),
                  "kv_cache": "int8-turboquant" if a.turbo else a.dtype, "model": "gpt2-124m" if a.model == "gpt2" else "gemma3-1b-shape", "data": "random weights"}))
