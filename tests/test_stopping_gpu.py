"""Stop sequences on the device (csrc/kernels/stop_check.hip): the kernel against ``reference_stop``
on scripted streams — ``done``, ``finish_at`` and the rewritten tokens, exactly — and the decode path
(graph bursts, eager steps, streaming, log-probabilities, penalties, the routed ``stop_token``) through
a tiny bf16 GPT: every row must equal the same-seed run without ``stop``, cut at ``reference_stop``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode as gd
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel, _stop_burst
from penroz.ops.stopping import MAX_LEN, MAX_SEQS, StopState, reference_stop

DEV = "cuda"

# ------------------------------------------------------------------ the kernel
STOP_SETS = {
    "overlap": [[5, 5, 7]],
    "ties": [[9], [2, 3], [3], [1, 2, 3]],
    "lengths": [[1, 2, 3, 4], [3]],
    "long": [[0, 1, 2, 0, 1, 2, 0, 1]],
    "16x8": [[(i + j) % 4 for j in range(MAX_LEN)] for i in range(MAX_SEQS)],
}
NEVER = 15  # in none of the sets
T = 24


def streams(B, stop, seed):
    """int64 [B, T] with ids below 16: drawn, then row 0 made to complete ``stop[-1]`` (after a prefix
    of it that a restarting matcher would trip over) and the last row, if there is another, made to
    complete nothing."""
    g = torch.Generator().manual_seed(seed)
    gen = torch.randint(0, 15, (B, T), generator=g)
    s = stop[-1]
    gen[0, :3] = NEVER
    gen[0, 3:3 + len(s) - 1] = torch.tensor(s[:-1], dtype=torch.long)
    gen[0, 3 + len(s) - 1:3 + 2 * len(s) - 1] = torch.tensor(s)
    if B > 1:
        gen[B - 1] = NEVER
    return gen


def frozen(gen, finish_at):
    want = gen.clone()
    for b, at in enumerate(finish_at):
        if at:
            want[b, at:] = gen[b, at - 1]
    return want


def run_call(st, gen, stop, step_form):
    """One call on the state's buffers, a column per launch; checks everything against the reference."""
    finish_at, which = reference_stop(gen, stop)
    st.set_stop(stop)
    st.begin()
    seen = torch.empty_like(gen)
    out = torch.full((gen.shape[0], T), -7, dtype=torch.long, device=DEV)
    step_t = torch.zeros(1, dtype=torch.long, device=DEV)
    for t in range(T):
        col = gen[:, t].to(DEV).view(-1, 1).contiguous()
        if step_form:  # as the captured step: the sampler wrote idx and the column, the counter advanced
            out[:, t] = col.view(-1)
            step_t.fill_(t + 1)
            st.step(col, out, step_t)
        else:
            assert st.observe(col) is col
        seen[:, t] = col.view(-1).cpu()
    done, fin = st.read()
    assert fin == finish_at and done == [w + 1 for w in which]
    assert torch.equal(seen, frozen(gen, finish_at))
    if step_form:
        assert torch.equal(out.cpu(), seen)
    assert st.n_gen.tolist() == [at or T for at in finish_at]  # a finished row's state no longer changes
    return finish_at


@pytest.mark.parametrize("step_form", [False, True], ids=["observe", "step"])
@pytest.mark.parametrize("name", sorted(STOP_SETS))
@pytest.mark.parametrize("B", [1, 3, 65])
def test_kernel_equals_the_reference(B, name, step_form):
    """Two calls on the same buffers, the second with another set. In each call the reference alone
    finishes a row and, where there is more than one row, leaves one unfinished (checked on the CPU);
    the single row of B = 1 finishes in the first call and is left unfinished in a third."""
    names = sorted(STOP_SETS)
    stop, other = STOP_SETS[name], STOP_SETS[names[(names.index(name) + 1) % len(names)]]
    st = StopState(B, DEV)
    for i, s in enumerate((stop, other)):
        gen = streams(B, s, seed=B + i)
        finish_at, _ = reference_stop(gen, s)
        assert finish_at[0] and (B == 1 or not finish_at[-1])
        run_call(st, gen, s, step_form)
    if B == 1:
        gen = torch.full((1, T), NEVER)
        assert reference_stop(gen, stop) == ([0], [-1])
        run_call(st, gen, stop, step_form)


def test_kernel_refuses_operands_of_another_shape():
    st = StopState(3, DEV)
    st.set_stop([[1]])
    st.begin()
    with pytest.raises(RuntimeError):
        st.observe(torch.zeros(3, dtype=torch.long))  # a host tensor
    with pytest.raises((RuntimeError, AssertionError)):
        st.observe(torch.zeros(4, dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError):
        st.step(torch.zeros(3, 1, dtype=torch.long, device=DEV), torch.zeros(2, 8, dtype=torch.long, device=DEV),
                torch.ones(1, dtype=torch.long, device=DEV))
    # a step counter outside the burst buffer writes nothing outside it
    idx, out = torch.ones(3, 1, dtype=torch.long, device=DEV), torch.zeros(3, 2, dtype=torch.long, device=DEV)
    st.step(idx, out, torch.ones(1, dtype=torch.long, device=DEV))  # finishes all rows on [1]
    st.step(idx, out, torch.full((1,), 9, dtype=torch.long, device=DEV))
    assert out.tolist() == [[0, 0]] * 3 and st.read() == ([1] * 3, [1] * 3)


# ------------------------------------------------------------------ graph decode
BLOCK, NEW, P = 16, 40, 6  # 6 + 40 tokens through a window of 16: it re-prefills twice
KW = dict(temperature=1.0, top_k=5)
SEED = 7


def _ctx(nrows):
    return torch.randint(0, 256, (nrows, P), generator=torch.Generator().manual_seed(2)).tolist()


def _gpt():
    torch.manual_seed(11)
    m = NeuralNetworkModel("stop", Mapper(bench.gpt2_layers(V=256, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    return m.to(DEV).to(dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def gpt():
    return _gpt()


def _dec(m, rows, temperature=1.0):
    (dec,) = [d for d in m._graph_decoders.values() if d.rows == rows and d.temperature == temperature]
    return dec


@pytest.fixture(scope="module")
def plain(gpt):
    """The run without ``stop``, computed once and left unchanged."""
    torch.manual_seed(SEED)
    rows = gpt.generate_batch(_ctx(3), BLOCK, NEW, **KW)
    assert all(len(r) == P + NEW for r in rows)
    return rows


def stops_from(rows):
    """Row 0's generated tokens 9-11 and row 1's generated token 20; row 2 is left to run."""
    return [rows[0][P + 8:P + 11], [rows[1][P + 19]]]


def cut(rows, stop):
    finish_at, which = reference_stop([r[P:] for r in rows], stop)
    return [r[:P + at] if at else r for r, at in zip(rows, finish_at)], finish_at, which


def reasons(finish_at, which):
    return [{"finish_reason": "stop", "stop_sequence": w} if at else {"finish_reason": "length", "stop_sequence": None}
            for at, w in zip(finish_at, which)]


@pytest.mark.parametrize("burst", [None, "1", "4"], ids=["default", "burst1", "burst4"])
def test_rows_finish_on_their_own_in_graph_bursts(monkeypatch, gpt, plain, burst):
    if burst is not None:
        monkeypatch.setenv("PENROZ_STOP_BURST", burst)
    stop = stops_from(plain)
    want, finish_at, which = cut(plain, stop)
    assert finish_at[0] and finish_at[1]  # (row 2 runs to length unless it meets one of them)
    runs = []
    run = gd.GraphDecoder.run

    def counted(self, last_tok, n_steps, start=0):
        runs.append(n_steps)
        return run(self, last_tok, n_steps, start)

    monkeypatch.setattr(gd.GraphDecoder, "run", counted)
    torch.manual_seed(SEED)
    contexts, infos = gpt.generate_batch(_ctx(3), BLOCK, NEW, stop=stop, **KW)
    assert contexts == want and infos == reasons(finish_at, which)
    dec = _dec(gpt, 3)
    assert dec._stop_on and isinstance(dec.graph, torch.cuda.CUDAGraph), "graph path not taken"
    assert runs and max(runs) <= _stop_burst()


def test_stream_ends_at_the_finish(gpt, plain):
    stop = stops_from(plain)
    want, finish_at, which = cut(plain, stop)
    assert finish_at[0]
    torch.manual_seed(SEED)
    assert list(gpt.generate_tokens_stream(_ctx(3), BLOCK, NEW, stop=stop, **KW)) == want[0][P:]
    torch.manual_seed(SEED)
    tokens, info = gpt.generate_tokens(_ctx(3), BLOCK, NEW, stop=stop, **KW)
    assert tokens == want[0] and info == {"finish_reason": "stop", "stop_sequence": which[0]}


def test_logprob_lists_are_cut_with_the_rows(gpt, plain):
    stop = stops_from(plain)
    want, finish_at, which = cut(plain, stop)
    torch.manual_seed(SEED)
    _, whole = gpt.generate_batch(_ctx(3), BLOCK, NEW, logprobs=2, **KW)
    torch.manual_seed(SEED)
    contexts, infos = gpt.generate_batch(_ctx(3), BLOCK, NEW, stop=stop, logprobs=2, **KW)
    assert contexts == want
    for ctx, info, full, reason in zip(contexts, infos, whole, reasons(finish_at, which)):
        n = len(ctx) - P
        assert len(info["token_logprobs"]) == len(info["top_logprobs"]) == n
        assert info["token_logprobs"] == full["token_logprobs"][:n] and info["top_logprobs"] == full["top_logprobs"][:n]
        assert {k: info[k] for k in reason} == reason


def test_with_a_repetition_penalty(gpt):
    torch.manual_seed(SEED)
    rows = gpt.generate_batch(_ctx(3), BLOCK, NEW, repetition_penalty=1.3, **KW)
    stop = stops_from(rows)
    want, finish_at, which = cut(rows, stop)
    torch.manual_seed(SEED)
    contexts, infos = gpt.generate_batch(_ctx(3), BLOCK, NEW, stop=stop, repetition_penalty=1.3, **KW)
    assert contexts == want and infos == reasons(finish_at, which)


def test_another_stop_set_replays_the_same_graph_and_no_stop_is_off(gpt, plain):
    stop = stops_from(plain)
    torch.manual_seed(SEED)
    gpt.generate_batch(_ctx(3), BLOCK, NEW, stop=stop, **KW)
    dec = _dec(gpt, 3)
    graph = dec.graph
    assert dec._stop_on and isinstance(graph, torch.cuda.CUDAGraph)
    other = [[plain[2][P + 30]], plain[1][P + 3:P + 8]]
    want, finish_at, which = cut(plain, other)
    assert finish_at[1] and finish_at[2]
    torch.manual_seed(SEED)
    contexts, infos = gpt.generate_batch(_ctx(3), BLOCK, NEW, stop=other, **KW)
    assert dec.graph is graph and dec.stop.n_seqs.tolist() == [2]
    assert contexts == want and infos == reasons(finish_at, which)
    torch.manual_seed(SEED)
    assert gpt.generate_batch(_ctx(3), BLOCK, NEW, **KW) == plain
    assert not dec._stop_on and dec.graph is not graph
    torch.manual_seed(SEED)
    gpt.generate_batch(_ctx(3), BLOCK, NEW, stop=stop, **KW)
    assert dec._stop_on and dec.graph is graph


def test_stop_token_with_one_row_takes_the_device_check(monkeypatch):
    monkeypatch.setattr(gd, "DECODE_PROGRAM", False)  # the module-forward graph: same numerics as eager
    m = _gpt()
    ctx = _ctx(1)
    free = m.generate_tokens(ctx, BLOCK, NEW, temperature=0.0)[P:]
    at, s = max((free.index(t), t) for t in set(free))  # the token that first appears latest
    assert at >= 2, "the greedy run repeats itself from the start: take another prompt"
    eager = list(m._generate_eager(ctx, BLOCK, NEW, 0.0, None, s, True))[-1]
    assert eager == ctx[0] + free[:at + 1]
    runs = []
    run = gd.GraphDecoder.run

    def counted(self, last_tok, n_steps, start=0):
        runs.append(n_steps)
        return run(self, last_tok, n_steps, start)

    monkeypatch.setattr(gd.GraphDecoder, "run", counted)
    assert m.generate_tokens(ctx, BLOCK, NEW, temperature=0.0, stop_token=s) == eager
    assert 0 < len(runs) < at + 1 and max(runs) > 1
    dec = _dec(m, 1, 0.0)
    assert dec._stop_on and dec.stop.stop == [[s]]
    # several rows keep the host check: no device state, the step without the kernel
    before = len(runs)
    m.generate_tokens(_ctx(3), BLOCK, 8, temperature=0.0, stop_token=s)
    dec3 = _dec(m, 3, 0.0)
    assert not dec3._stop_on and dec3.stop is None and all(n == 1 for n in runs[before:])
