"""Prompt-lookup speculative decoding on MI355X (ops/speculative.py, csrc/kernels/spec_decode.hip,
``GraphDecoder(speculate=k)``): ``spec_advance`` against the Python definition, integer for integer; the
shared-cache ``kv_append`` plus the ``Tq = k + 1`` decode attention against fp32 torch attention, with the
one-row path as the yardstick; teacher-forced verify steps against a cache-free one-row forward, with a wrong
draft in row 1; and ``generate_tokens(..., speculate=k)`` end to end on random weights and on a copy model
whose argmax is the token it was fed, where every draft is accepted."""
import copy
import math
import random
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import bench
from penroz.models import graph_decode as gd
from penroz.models import kv_cache as kvc
from penroz.models.executor import GPTExecutor
from penroz.models.mapper import Mapper
from penroz.models.model import NeuralNetworkModel
from penroz.ops import attention as attn_ops
from penroz.ops import speculative as spec
from penroz.ops._ext import kernels

V, CAP = 256, 32
DEV = "cuda"


@lru_cache(maxsize=None)
def _model(kind):
    """The tiny bf16 models of the ragged decode tests."""
    if kind == "gpt":
        torch.manual_seed(11)
        m = NeuralNetworkModel("sp", Mapper(bench.gpt2_layers(V=V, C=128, L=2, H=2, P=64), {"adamw": {"lr": 1e-3}}))
    else:  # Gemma style: RoPE, head_dim 256, 4:1 GQA, RMSNorm, gated MLP
        tc = SimpleNamespace(vocab_size=V, hidden_size=64, num_attention_heads=4, num_key_value_heads=1, head_dim=256,
                             num_hidden_layers=2, intermediate_size=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                             attention_dropout=0.0, hidden_activation="gelu_pytorch_tanh", model_type="gemma3_text")
        torch.manual_seed(5)
        m = NeuralNetworkModel("spg", Mapper(Mapper.from_hf_config(tc), {"adamw": {"lr": 1e-3}}))
    return m.to("cuda").to(dtype=torch.bfloat16).eval()


@lru_cache(maxsize=None)
def _copy_model():
    """The GPT model with its position table, attention output projections and fc2 weights zeroed and the
    vocabulary projection set to the token table: the residual stream is the fed token's embedding, so the
    argmax is the token it was fed, whatever came before it."""
    src = _model("gpt")
    src.__dict__.pop("_graph_decoders", None)  # (captured graphs are not copied)
    m = copy.deepcopy(src)
    sp = GPTExecutor.match(m)
    with torch.no_grad():
        sp.wpe.weight.zero_()
        for b in sp.blocks:
            b.proj.weight.zero_()
            b.fc2.weight.zero_()
        sp.head.weight.copy_(sp.wte.weight)
    return m


# ------------------------------------------------------------------ 1. spec_advance
class _State:
    """The device state of a speculative step, loaded from Python values."""

    def __init__(self, cap, k):
        self.cap, self.k = cap, k
        self.hist = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
        self.ctr = torch.zeros(5, dtype=torch.int32, device=DEV)  # n, emitted, limit, steps, accepted
        self.cand = torch.zeros(k + 1, dtype=torch.long, device=DEV)
        self.idx = torch.zeros(k + 1, 1, dtype=torch.long, device=DEV)
        self.pos = torch.zeros(k + 1, dtype=torch.long, device=DEV)
        self.len = torch.zeros(1, dtype=torch.long, device=DEV)

    def load(self, hist, drafts, cand, emitted, limit, steps=3, accepted=2):
        self.hist.fill_(-7)
        self.hist[:len(hist)] = torch.tensor(hist, dtype=torch.int32)
        self.ctr.copy_(torch.tensor([len(hist), emitted, limit, steps, accepted], dtype=torch.int32))
        self.cand.copy_(torch.tensor(cand))
        self.idx.copy_(torch.tensor([hist[-1]] + list(drafts)).view(-1, 1))
        self.pos.copy_(torch.arange(len(hist) - 1, len(hist) + self.k))
        self.len.fill_(len(hist) + self.k)

    def run(self, draft_only=False):
        c = self.ctr
        kernels().spec_advance(self.hist, c[0:1], self.cand, self.idx, self.pos, self.len, c[1:2], c[2:3], c[3:4],
                               c[4:5], self.k, draft_only)

    def read(self):
        return (self.hist.tolist(), self.ctr.tolist(), self.idx.view(-1).tolist(), self.pos.tolist(), self.len.tolist())


def _expect(hist, drafts, cand, emitted, limit, cap, steps=3, accepted=2):
    """What the definition gives for one step from this state, in ``_State.read``'s form; None: frozen."""
    k, h = len(drafts), list(hist)
    e, acc = spec.advance(h, drafts, cand, emitted, limit, cap)
    if e == 0:
        return None
    n = len(h)
    return (h + [-7] * (cap - n), [n, emitted + e, limit, steps + 1, accepted + acc], [h[-1]] + spec.draft(h, k),
            list(range(n - 1, n + k)), [n + k])


def _check_step(st, hist, drafts, cand, emitted, limit):
    st.load(hist, drafts, cand, emitted, limit)
    before = st.read()
    st.run()
    want = _expect(hist, drafts, cand, emitted, limit, st.cap)
    assert st.read() == (before if want is None else want), (hist, drafts, cand, emitted, limit)
    return want is not None


@pytest.mark.parametrize("k", [1, 2, 3])
def test_spec_advance_is_the_python_definition(k):
    rng = random.Random(100 + k)
    cap = 40
    st = _State(cap, k)
    emitted_steps = frozen_steps = cut_steps = 0
    for n in (1, 2, 4, 9, cap - k - 1):
        for a in range(k + 1):
            for trial in range(4):
                hist = [rng.randrange(4) for _ in range(n)]  # a small alphabet: matches at every m
                drafts = spec.draft(hist, k) if trial % 2 == 0 else [rng.randrange(4) for _ in range(k)]
                cand = list(drafts[:a]) + [(drafts[a] + 1) % 4 if a < k else rng.randrange(4)] + \
                       [rng.randrange(4) for _ in range(k - a)]
                assert spec.accept(drafts, cand) == a
                # the limit far away, cutting the emission short (where a + 1 > 1), and reached (frozen)
                for emitted, limit in ((0, 100), (5, 6), (6, 6), (9, 6)):
                    ran = _check_step(st, hist, drafts, cand, emitted, limit)
                    emitted_steps += ran
                    frozen_steps += not ran
                    cut_steps += ran and limit - emitted < a + 1
    assert emitted_steps and frozen_steps and cut_steps
    # no room left for the next step's rows: frozen, whatever the limit says
    assert not _check_step(st, [1] * (cap - k), [1] * k, [1] * (k + 1), 0, 100)


@pytest.mark.parametrize("k", [1, 3])
def test_spec_advance_scans_a_long_history(k):
    """More than 256 tokens: every thread scans several starts, and the winner lies in any of them."""
    rng = random.Random(7 + k)
    cap = 700
    st = _State(cap, k)
    for n in (257, 300, 513, 690):
        for alphabet in (3, 50, 100000):  # dense matches at m = 3; sparse ones; none at all
            hist = [rng.randrange(alphabet) for _ in range(n)]
            if alphabet == 50:  # plant the only 3-gram match at a chosen start, early or late
                j = rng.choice([0, 5, 255, 256, 257, n - 8])
                hist[j:j + 3] = [1000, 1001, 1002]
                hist[n - 3:] = [1000, 1001, 1002]
            drafts = spec.draft(hist, k)
            assert _check_step(st, hist, drafts, drafts + [rng.randrange(alphabet)], 0, 100)  # a = k
            assert _check_step(st, hist, drafts, [drafts[0] + 1] * (k + 1), 0, 100)  # a = 0
            st.load(hist, [0] * k, [0] * (k + 1), 0, 100)
            st.run(draft_only=True)  # the draft half alone: nothing emitted, the rows of the first step
            got = st.read()
            assert got[0][:n] == hist and got[1] == [n, 0, 100, 3, 2]
            assert got[2:] == ([hist[-1]] + spec.draft(hist, k), list(range(n - 1, n + k)), [n + k])


# ------------------------------------------------------------------ 2. shared-cache append + Tq = R attention
ACAP = 2048  # the launch is sized for the capacity: with the in-launch merge, splits of >= 256 keys
CONTEXTS = (3, 255, 256, 257, 1500)  # one split; the rows straddle the first split boundary; six splits


def _reference_rows(q, kc, vc, ks, vs, n):
    """fp32 torch attention of row i of q [R, H, D] over the first n + i slots of the (dequantised) cache."""
    R, H, D = q.shape
    k, v = kc[0].float(), vc[0].float()  # [Hkv, cap, D]
    if ks is not None:
        k, v = k * ks[0][..., None], v * vs[0][..., None]
    G = H // k.shape[0]
    out = torch.empty(R, H * D, device=DEV)
    for i in range(R):
        kk = k[:, :n + i].repeat_interleave(G, dim=0)
        vv = v[:, :n + i].repeat_interleave(G, dim=0)
        s = torch.einsum("hd,hsd->hs", q[i].float(), kk) / math.sqrt(D)
        out[i] = torch.einsum("hs,hsd->hd", torch.softmax(s, dim=-1), vv).reshape(-1)
    return out


@pytest.mark.parametrize("quant", [False, True], ids=["bf16", "int8"])
@pytest.mark.parametrize("H,Hkv,D", [(2, 2, 64), (4, 1, 256)], ids=["d64-mha", "d256-gqa4"])
@pytest.mark.parametrize("R", [2, 4])
def test_shared_cache_append_and_multi_row_attention(R, H, Hkv, D, quant):
    g = torch.Generator(DEV).manual_seed(R * 1000 + D + quant)
    K = kernels()
    for n in CONTEXTS:
        if quant:
            kc = torch.randint(-127, 128, (1, Hkv, ACAP, D), device=DEV, generator=g, dtype=torch.int8)
            vc = torch.randint(-127, 128, (1, Hkv, ACAP, D), device=DEV, generator=g, dtype=torch.int8)
            ks = torch.rand(1, Hkv, ACAP, device=DEV, generator=g) / 64 + 1e-3
            vs = torch.rand(1, Hkv, ACAP, device=DEV, generator=g) / 64 + 1e-3
        else:
            kc = torch.randn(1, Hkv, ACAP, D, device=DEV, generator=g).bfloat16()
            vc = torch.randn(1, Hkv, ACAP, D, device=DEV, generator=g).bfloat16()
            ks = vs = None
        before = [t.clone() for t in (kc, vc, ks, vs) if t is not None]
        qkv = torch.randn(R, (H + 2 * Hkv) * D, device=DEV, generator=g).bfloat16()
        q, k, v = gd._qkv_views(qkv, H, Hkv, D)
        pos_t = torch.arange(n - 1, n - 1 + R, device=DEV)
        len_t = torch.tensor([n + R - 1], device=DEV)
        K.kv_append(k, v, kc, vc, ks, vs, pos_t, 0)
        # the R appended slots hold the rows (int8: as the one-row append quantises them), the others are unchanged
        one = [t.clone() for t in before]
        for i in range(R):
            K.kv_append(k[i:i + 1], v[i:i + 1], *one[:2], *(one[2:] or (None, None)), None, n - 1 + i)
        for got, alone, was in zip((kc, vc, ks, vs), one, before):
            assert torch.equal(got, alone)
            mask = torch.ones(ACAP, dtype=torch.bool, device=DEV)
            mask[n - 1:n - 1 + R] = False
            assert torch.equal(got[:, :, mask], was[:, :, mask])
        if not quant:
            assert torch.equal(kc[0, :, n - 1:n - 1 + R].transpose(0, 1), k.reshape(R, Hkv, D))
        out = attn_ops.decode_attention(gd._as_one_sequence(q), kc, vc, ACAP, ks, vs, seq_len_dev=len_t).view(R, H * D).float()
        ref = _reference_rows(q.reshape(R, H, D), kc, vc, ks, vs, n)
        # the yardstick: the existing one-row path on the same data, row i with its own device length
        ctl = torch.cat([attn_ops.decode_attention(q[i:i + 1], kc, vc, ACAP, ks, vs,
                                                   seq_len_dev=torch.tensor([n + i], device=DEV)).view(1, -1)
                         for i in range(R)]).float()
        err = ((out - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
        ctl_err = ((ctl - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
        print(f"R {R} H {H}/{Hkv} D {D} {'int8' if quant else 'bf16'} n {n}: rows {err:.3e}, one-row path {ctl_err:.3e}")
        assert err <= 2 * ctl_err, (n, err, ctl_err)
        assert err < 2e-2, (n, err)


# ------------------------------------------------------------------ 3. teacher-forced verify step
def _forced(dec, toks, first_pos):
    """One program step of ``dec`` on ``toks`` (R of them) at positions first_pos .. first_pos + R - 1 of the
    one sequence -> logits [R, V] (bf16, a copy)."""
    R = len(toks)
    dec.idx.copy_(torch.tensor(toks, device=DEV).view(R, 1))
    dec.cache.pos_t.copy_(torch.arange(first_pos, first_pos + R, device=DEV))
    dec.cache.len_t.fill_(first_pos + R)
    dec.cache.graph_mode = True
    dec.cache.begin_step()
    try:
        return dec.program.forward(dec.idx, dec.cache).clone()
    finally:
        dec.cache.graph_mode = False


def _rel(got, ref):
    return ((got.float() - ref).norm(dim=-1) / ref.norm(dim=-1))


@pytest.mark.parametrize("kind,k", [("gpt", 1), ("gpt", 3), ("gemma", 3)])
def test_teacher_forced_verify_step(kind, k):
    """Rows 0..k at positions n - 1 .. n - 1 + k against a one-row cache-free forward at those positions;
    the control is the uniform one-row decoder, teacher-forced over the same positions one at a time."""
    m, R, n = _model(kind), k + 1, 7
    seq = torch.randint(0, V, (n + R,), device=DEV, generator=torch.Generator(DEV).manual_seed(31 + k)).tolist()
    with torch.inference_mode():
        acts, _ = m._forward_nocache(torch.tensor([seq], device=DEV))
        ref = acts[-1][0].float()  # [n + R, V]: position p decides token p + 1
        dec = gd.GraphDecoder(m, R, CAP, 0.0, None, speculate=k)
        assert dec.cache.shared and dec.cache.pos_t.shape == (R,) and dec.cache.len_t.shape == (1,)
        uni = gd.GraphDecoder(m, 1, CAP, 0.0, None)
        prompt = torch.tensor([seq[:n - 1]], device=DEV)
        ctl = torch.empty(R + 1, V, device=DEV)
        uni.attach()
        try:
            m(prompt, skip_softmax=True)
            for i in range(R + 1):
                uni._set_state(torch.tensor([[seq[n - 1 + i]]], device=DEV), n - 1 + i)
                uni.cache.graph_mode = True
                uni.cache.begin_step()
                try:
                    ctl[i] = uni.program.forward(uni.idx, uni.cache)[0].float()
                finally:
                    uni.cache.graph_mode = False
        finally:
            uni.detach()
        dec.attach()
        try:
            m(prompt, skip_softmax=True)
            assert dec.cache._k[0].shape[0] == 1  # a cache of batch 1
            good = _forced(dec, seq[n - 1:n - 1 + R], n - 1)
            wrong = list(seq[n - 1:n - 1 + R])
            wrong[1] = (wrong[1] + 1) % V
            bad = _forced(dec, wrong, n - 1)  # a wrong draft in row 1 ...
            after = _forced(dec, seq[n:n + R], n)  # ... rejected (a = 0): the next step starts one position on
        finally:
            dec.detach()
    assert torch.equal(bad[0], good[0])  # row 0 sees nothing of row 1
    assert not torch.equal(bad[1], good[1])
    ctl_worst = _rel(ctl, ref[n - 1:n + R]).max().item()
    for name, got, want in (("verify", good, ref[n - 1:n - 1 + R]), ("after a rejection", after, ref[n:n + R])):
        rel = ((got.float() - want).norm() / want.norm()).item()
        worst = _rel(got, want).max().item()
        print(f"{kind} k {k} {name}: rel {rel:.3e} worst row {worst:.3e}; one-row control worst {ctl_worst:.3e}")
        assert rel < 2e-2, (name, rel)
        assert worst <= 2 * ctl_worst, (name, worst, ctl_worst)


# ------------------------------------------------------------------ 4. / 5. / 6. end to end
class _EagerGraph:
    """Stands in for a captured graph: replay() runs the decode step eagerly."""

    def __init__(self, dec):
        self.dec = dec

    def replay(self):
        self.dec._step()


def _eager_capture(self, last_tok, cache_len, start=0):
    self._set_state(last_tok, cache_len, start)
    self.graph = _EagerGraph(self)


def _shortfall(m, prompt, ctx):
    """How far the reference logit of every generated token lies below its row's maximum (one cache-free
    forward over prompt + generated tokens) -> (worst shortfall, largest row maximum)."""
    with torch.inference_mode():
        acts, _ = m._forward_nocache(torch.tensor([ctx[:-1]], device=DEV))
    logits = acts[-1][0, len(prompt) - 1:].float()
    chosen = torch.tensor(ctx[len(prompt):], device=DEV)
    mx = logits.amax(-1)
    return (mx - logits.gather(1, chosen.unsqueeze(1)).squeeze(1)).max().item(), mx.abs().max().item()


@pytest.mark.parametrize("kind", ["gpt", "gemma"])
def test_generate_tokens_speculative_end_to_end(monkeypatch, kind):
    m = _model(kind)
    m.__dict__.pop("_graph_decoders", None)
    prompt, block, new = [5, 9, 200, 5, 9, 17], 32, 20
    plain = m.generate_tokens([prompt], block, new, temperature=0.0)
    got = m.generate_tokens([prompt], block, new, temperature=0.0, speculate=3)
    assert len(got) == len(prompt) + new and got[:len(prompt)] == prompt
    decs = [d for d in m._graph_decoders.values() if d.speculate == 3]
    assert decs and decs[0].rows == 4 and isinstance(decs[0].graph, torch.cuda.CUDAGraph), "no graph captured by a speculative decoder"
    stats = m.last_speculation
    assert stats["drafted"] == 3 * stats["steps"] and stats["steps"] + stats["accepted"] == new
    ctl, _ = _shortfall(m, prompt, plain)
    short, top = _shortfall(m, prompt, got)
    bf16_step = 2.0 ** (math.floor(math.log2(max(top, 1e-30))) - 7)
    print(f"{kind}: speculative shortfall {short:.4g}, plain {ctl:.4g}, bf16 step {bf16_step:.4g}; {stats}; "
          f"same tokens: {got == plain}")
    assert short <= max(2 * ctl, bf16_step), (short, ctl, bf16_step)
    assert m.generate_batch([prompt], block, new, temperature=0.0, speculate=3) == [got]  # the graph, replayed
    m.__dict__.pop("_graph_decoders")
    monkeypatch.setattr(gd.GraphDecoder, "_capture", _eager_capture)
    assert m.generate_tokens([prompt], block, new, temperature=0.0, speculate=3) == got


def test_every_draft_is_accepted_on_the_copy_model():
    m = _copy_model()
    m.__dict__.pop("_graph_decoders", None)
    a, b, c = 40, 41, 42
    prompt, block, new = [b, c, a], 32, 17
    plain = m.generate_tokens([prompt], block, new, temperature=0.0)
    assert plain == prompt + [a] * new  # the argmax is the token it was fed
    assert m.generate_tokens([prompt], block, new, temperature=0.0, speculate=3) == plain
    want = {}
    assert spec.reference_generate(lambda h: h[-1], prompt, new, 3, want) == plain
    assert want == {"steps": 5, "drafted": 15, "accepted": 12}  # four full steps, all accepted; one token is left
    assert m.last_speculation == want
    for k in (1, 2):
        assert m.generate_tokens([prompt], block, new, temperature=0.0, speculate=k) == plain
        spec.reference_generate(lambda h: h[-1], prompt, new, k, want)
        assert m.last_speculation == want and want["accepted"] == new - want["steps"]
    # the first step drafts [b, c, a] behind the earlier a and the model answers a: rejected, a = 0
    prompt = [a, b, c, a]
    assert spec.draft(prompt, 3) == [b, c, a]
    plain = m.generate_tokens([prompt], block, new, temperature=0.0)
    assert m.generate_tokens([prompt], block, new, temperature=0.0, speculate=3) == plain == prompt + [a] * new
    spec.reference_generate(lambda h: h[-1], prompt, new, 3, want)
    # 1 token, then four steps of 4: five steps again, but the first one's three drafts are lost
    assert m.last_speculation == want == {"steps": 5, "drafted": 15, "accepted": 12}
    # a prompt of one token, and a call that fills the window exactly
    assert m.generate_tokens([[a]], block, block - 1 - 3, temperature=0.0, speculate=3) == [a] * (block - 3)


def test_stop_token_is_cut_by_the_host():
    m = _copy_model()
    m.__dict__.pop("_graph_decoders", None)
    a = 77
    prompt, block = [3, a], 32
    # the copy model repeats a: with stop_token a the first token ends the call, inside the first step's accepted run
    plain = m.generate_tokens([prompt], block, 12, temperature=0.0, stop_token=a)
    assert plain == prompt + [a]
    assert m.generate_tokens([prompt], block, 12, temperature=0.0, stop_token=a, speculate=3) == plain
    assert m.generate_batch([prompt], block, 12, temperature=0.0, stop_token=a, speculate=3) == [plain]
    r = _model("gpt")  # random weights: a stop token from the middle of the plain run
    free = r.generate_tokens([[5, 9, 200, 5, 9, 17]], block, 16, temperature=0.0, speculate=2)
    stop = free[6 + 9]
    cut = free[:6 + free[6:].index(stop) + 1]
    assert r.generate_tokens([[5, 9, 200, 5, 9, 17]], block, 16, temperature=0.0, speculate=2, stop_token=stop) == cut


@pytest.mark.parametrize("turbo", [False, True], ids=["bf16-cache", "int8-cache"])
def test_int8_weights_compose(monkeypatch, turbo):
    monkeypatch.setattr(kvc, "TURBO_QUANT_ENABLED", turbo)
    m = _copy_model()
    m.__dict__.pop("_graph_decoders", None)
    prompt, block, new = [8, 9, 8], 32, 17
    got = m.generate_tokens([prompt], block, new, temperature=0.0, speculate=3, weight_quant="int8")
    dec = next(d for d in m._graph_decoders.values() if d.speculate == 3)
    assert dec.weight_quant == "int8"
    assert isinstance(dec.cache, gd.StaticTurboKVCache if turbo else gd.StaticKVCache)
    assert got == prompt + [8] * new
    assert m.last_speculation == {"steps": 5, "drafted": 15, "accepted": 12}
    m.__dict__.pop("_graph_decoders", None)
