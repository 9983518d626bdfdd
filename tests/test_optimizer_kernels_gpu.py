"""Fused Adam / AdamW kernels (csrc/kernels/adamw.hip) against a plain fp64 reference (MI355X).

Every comparison is ONE step from an identical state, so the tolerance is one kernel's rounding:
elementwise |x − x_ref| ≤ K · 2⁻²⁴ · scale with scale_p = |p_ref| + |Δ_ref|, scale_m = |m_ref| +
|g_eff|, scale_v = v_ref + g_eff². The reference ``adam_ref``, the inputs, the three hyper-parameter
sets and K live in tests/adam_reference.py (this module skips itself at import without a device, and
the CPU suite must be able to check that the inputs separate a wrong step from a right one:
tests/test_adam_reference.py). K = 4 x the worst ratio of the same formula in fp32 torch ops against
fp64; measured ratios for p: 2.95 … 13.01 over the sets (K_p = 11.8 … 52.1; the table with m and v is
in the header of adam_reference.py).

* flat kernel: sizes around the float4 width and one with a grid-stride loop and a scalar tail; with /
  without the bf16 shadow; PENROZ_ADAM_NT = 0 / 1 / 2 and PENROZ_ADAM_GRID-limited launches bitwise
  equal to the default launch; misaligned slices refused on the host;
* per-range steps (``flat_step_ranges``, ``begin_flat_ranges().apply``) bitwise equal to the whole
  step, and writing nothing outside their range;
* row-split embedding step (``adam_rows_step``) against the dense step (bitwise) and fp64, with
  duplicate tokens, ids outside the table, more tokens than the 65536-workgroup cap, rows wider
  than one workgroup pass; mode 0 reads no gradient (NaN there), mode 1 leaves mask 2 / gradient 0.
  (Mode 0's own grid cap, 2²⁰ workgroups = 2²⁸ float4, cannot be reached at test sizes: its
  grid-stride loop is the same code the flat kernel's PENROZ_ADAM_GRID cases run.)
* list mode (``multi_tensor_adam`` through FusedAdamW / FusedAdam): tensor sizes on the 8192-element
  chunk boundary, 200 small tensors, fp32 / bf16 / mixed groups, maximize and grad_scale.

What they found when first run: 1 − β1, 1 − β2 and 1 − lr·wd formed in fp32 inside the kernel put p up
to 6.8x over the bound (β2 = 0.999), and with L2 decay the row-split step was not bitwise the dense
step (multiply-adds contracted differently per kernel instantiation). With both fixed in adamw.hip
the worst fp32 error is 0.30 of the bound, the worst bf16 one 0.996 (a full half-ulp of bf16).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU runner
    pytest.skip("needs a GPU", allow_module_level=True)

import adam_reference as A
from adam_reference import HYPER_SETS, adam_ref, make_inputs
from penroz.models.optim import FusedAdam, FusedAdamW
from penroz.ops import _ext, fused as Fu

DEV = "cuda"
BF = torch.bfloat16


def _args(h):
    return (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], h["grad_scale"], h["maximize"])


def _flat_run(inputs, h, decoupled, shadow):
    """One flat step on device copies -> (p, m, v, shadow or None, g)."""
    p, g, m, v = (t.to(DEV).clone() for t in inputs)
    sh = torch.full((p.numel(),), 13.0, dtype=BF, device=DEV) if shadow else None
    (Fu.adamw_step if decoupled else Fu.adam_step)(p, g, m, v, sh, *_args(h))
    torch.cuda.synchronize()
    return p, m, v, sh, g


def _check_fp64(got, inputs, h, decoupled, what):
    ref, sc = A.scales(*inputs, h, decoupled)
    A.assert_within(got, ref, sc, A.k_for(h, decoupled, inputs), what)


def test_extension_is_native():
    assert _ext.available()


def test_adam_ref_returns_the_update_term():
    p, g, m, v = make_inputs(64, 7)
    h = HYPER_SETS[1]
    rp, rm, rv, delta = adam_ref(p, g, m, v, decoupled=True, **h)
    assert torch.equal(rp, p.double() * (1.0 - h["lr"] * h["wd"]) - delta)


# --------------------------------------------------------------------------- flat kernel
FLAT_SIZES = [1, 3, 4, 5, 1023, 262147]


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
@pytest.mark.parametrize("si", range(len(HYPER_SETS)))
@pytest.mark.parametrize("n", FLAT_SIZES)
def test_flat_step_matches_fp64(n, si, decoupled):
    h = HYPER_SETS[si]
    inputs = make_inputs(n, h["step"])
    p, m, v, sh, g = _flat_run(inputs, h, decoupled, shadow=True)
    _check_fp64((p, m, v), inputs, h, decoupled, f"flat n={n} set {si}")
    assert torch.equal(sh, p.to(BF)), "shadow != the kernel's own p rounded to bf16"
    assert torch.equal(g.cpu(), inputs[1]), "the flat step must not write the gradient"
    p2, m2, v2, _, _ = _flat_run(inputs, h, decoupled, shadow=False)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), "no-shadow path differs"


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
@pytest.mark.parametrize("n", FLAT_SIZES)
def test_flat_step_launch_variants_agree_bitwise(monkeypatch, n, decoupled):
    """PENROZ_ADAM_NT = 0 / 1 / 2 (plain, non-temporal, non-temporal stores) and, at the large size,
    a grid of 1 or 3 workgroups (grid-stride loop + scalar tail) == the default launch, bitwise.
    The default launch is the one compared with fp64 above."""
    h = HYPER_SETS[1]
    inputs = make_inputs(n, h["step"])
    monkeypatch.delenv("PENROZ_ADAM_NT", raising=False)
    monkeypatch.delenv("PENROZ_ADAM_GRID", raising=False)
    base = _flat_run(inputs, h, decoupled, shadow=True)
    variants = [("PENROZ_ADAM_NT", nt) for nt in ("0", "1", "2")]
    if n == 262147:
        variants += [("PENROZ_ADAM_GRID", "1"), ("PENROZ_ADAM_GRID", "3")]
    for name, val in variants:
        with monkeypatch.context() as mp:
            mp.setenv(name, val)
            for shadow in (True, False):
                got = _flat_run(inputs, h, decoupled, shadow)
                for a, b, what in zip(base[:3], got[:3], "pmv"):
                    assert torch.equal(a, b), f"{name}={val} shadow={shadow}: {what} differs from the default launch"
                if shadow:
                    assert torch.equal(base[3], got[3]), f"{name}={val}: shadow differs"
    if n == 262147:  # both at once: the plain kernel in a 3-workgroup grid
        with monkeypatch.context() as mp:
            mp.setenv("PENROZ_ADAM_NT", "0")
            mp.setenv("PENROZ_ADAM_GRID", "3")
            got = _flat_run(inputs, h, decoupled, True)
            assert all(torch.equal(a, b) for a, b in zip(base[:4], got[:4]))


def test_flat_step_refuses_misaligned_slices():
    """A range that starts off a multiple of 4 elements (the kernel reads float4 / two packed bf16
    words from the base) is refused on the host, before anything is launched."""
    h = HYPER_SETS[0]
    n = 64
    p, g, m, v = (t.to(DEV) for t in make_inputs(n, 1))
    before = [t.clone() for t in (p, g, m, v)]
    for fn in (Fu.adamw_step, Fu.adam_step):
        for off in (1, 2, 3):
            with pytest.raises(RuntimeError, match="16-B aligned"):
                fn(p[off:], g[off:], m[off:], v[off:], None, *_args(h))
    sh = torch.zeros(n + 4, dtype=BF, device=DEV)
    for off in (1, 2, 3):  # aligned fp32 buffers, shadow off 8 bytes
        with pytest.raises(RuntimeError, match="8-B aligned"):
            Fu.adamw_step(p, g, m, v, sh[off:off + n], *_args(h))
    opt = FusedAdamW([torch.nn.Parameter(p)], lr=1e-3)
    opt.attach_flat(list(opt.param_groups[0]["params"]), p, g, None, [0])
    apply = opt.begin_flat_ranges()
    with pytest.raises(RuntimeError, match="16-B aligned"):
        apply(1, 9)
    torch.cuda.synchronize()
    for a, b in zip((p, g, m, v), before):
        assert torch.equal(a, b), "a refused call must not have written anything"


# --------------------------------------------------------------------------- per-range steps
# (shape, pad elements after it): uneven sizes, every offset a multiple of 4 — two of them only
# because of the pad that follows, the way the executor pads the lm_head rows; the last range
# ends in a scalar tail (4099 % 4 == 3)
RANGE_PARAMS = [((25, 8), 0), ((30,), 2), ((1000, 3), 0), ((7,), 1), ((4099,), 0)]


def _flat_optimizer(cls, h, seed=0):
    offsets, off = [], 0
    for shape, pad in RANGE_PARAMS:
        offsets.append(off)
        off += int(torch.Size(shape).numel()) + pad
    total = off
    assert all(o % 4 == 0 for o in offsets)
    p, g, m, v = (t.to(DEV) for t in make_inputs(total, h["step"], seed))
    keep = torch.zeros(total, dtype=torch.bool, device=DEV)
    for (shape, _), o in zip(RANGE_PARAMS, offsets):
        keep[o:o + int(torch.Size(shape).numel())] = True
    for t in (p, g, m, v):  # pad elements: zero parameter, gradient and moments
        t.mul_(keep)
    shadow = p.to(BF)
    params = [torch.nn.Parameter(p[o:o + int(torch.Size(s).numel())].view(s)) for (s, _), o in zip(RANGE_PARAMS, offsets)]
    opt = cls(params, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], maximize=h["maximize"])
    for q, o in zip(params, offsets):
        k = q.numel()
        opt.state[q] = {"step": torch.tensor(float(h["step"] - 1)), "exp_avg": m[o:o + k].view_as(q).clone(),
                        "exp_avg_sq": v[o:o + k].view_as(q).clone()}
    opt.attach_flat(params, p, g, shadow, offsets)
    inputs = tuple(t.cpu().clone() for t in (p, g, opt._flat["m"], opt._flat["v"]))
    return opt, params, offsets, total, inputs


def _flat_state(opt, params):
    f = opt._flat
    torch.cuda.synchronize()
    return (f["param"], f["m"], f["v"], f["shadow"]), [float(opt.state[q]["step"]) for q in params]


@pytest.mark.parametrize("si", [1, 2])
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_ranged_flat_steps_equal_the_whole_step(cls, si):
    h = HYPER_SETS[si]
    gs = h["grad_scale"]
    whole, pw, offsets, total, inputs = _flat_optimizer(cls, h)
    whole.step(grad_scale=gs)
    ref_bufs, ref_steps = _flat_state(whole, pw)
    assert ref_steps == [float(h["step"])] * len(pw)
    assert torch.equal(ref_bufs[3], ref_bufs[0].to(BF))
    _check_fp64(ref_bufs[:3], inputs, h, cls is FusedAdamW, f"{cls.__name__} whole flat step set {si}")
    # ranges that tile the buffer: the parameter offsets, the large parameters cut once more
    cuts = sorted(set(offsets + [offsets[2] + 1500, offsets[4] + 2048, total]))
    ranges = list(zip(cuts[:-1], cuts[1:]))
    assert all(s % 4 == 0 for s, _ in ranges) and any((e - s) % 4 for s, e in ranges)
    tiled, pt, _, _, _ = _flat_optimizer(cls, h)
    assert tiled.flat_step_ranges(ranges, grad_scale=gs)
    rev, pr, _, _, _ = _flat_optimizer(cls, h)
    apply = rev.begin_flat_ranges(grad_scale=gs)
    assert apply is not None
    for s, e in reversed(ranges):
        apply(s, e)
    for name, (opt, ps) in (("flat_step_ranges", (tiled, pt)), ("begin_flat_ranges", (rev, pr))):
        bufs, steps = _flat_state(opt, ps)
        assert steps == ref_steps, name
        for a, b, what in zip(ref_bufs, bufs, ("p", "m", "v", "shadow")):
            assert torch.equal(a, b), f"{name}: {what} differs from the one-launch step"
        assert torch.equal(opt._flat["grad"], whole._flat["grad"])


@pytest.mark.parametrize("length", [2048, 2051])  # % 4 == 0 and == 3 (scalar tail inside the buffer)
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_range_step_writes_nothing_outside_its_range(cls, length):
    h = HYPER_SETS[1]
    n, s = 4096, 1024
    e = s + length
    ip, ig, im, iv = (t.to(DEV) for t in make_inputs(length, h["step"], 3))
    p, g = torch.full((n,), 7.0, device=DEV), torch.full((n,), 11.0, device=DEV)
    shadow = torch.full((n,), 13.0, dtype=BF, device=DEV)
    p[s:e], g[s:e] = ip, ig
    param = torch.nn.Parameter(p)
    opt = cls([param], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"],
              maximize=h["maximize"])
    opt.state[param] = {"step": torch.tensor(float(h["step"] - 1)), "exp_avg": torch.full((n,), 3.0, device=DEV),
                        "exp_avg_sq": torch.full((n,), 5.0, device=DEV)}
    opt.attach_flat([param], p, g, shadow, [0])
    m, v = opt._flat["m"], opt._flat["v"]
    m[s:e], v[s:e] = im, iv
    bufs = {"p": p, "g": g, "m": m, "v": v, "shadow": shadow}
    before = {k: t.clone() for k, t in bufs.items()}
    opt.begin_flat_ranges(grad_scale=h["grad_scale"])(s, e)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t[:s], before[k][:s]) and torch.equal(t[e:], before[k][e:]), f"{k} written outside [s, e)"
    assert torch.equal(g, before["g"])
    # inside: the same values as a step on stand-alone copies, and within the fp64 bound
    alone = _flat_run((ip, ig, im, iv), h, cls is FusedAdamW, shadow=True)
    for a, b in zip((p[s:e], m[s:e], v[s:e], shadow[s:e]), alone[:4]):
        assert torch.equal(a, b)
    _check_fp64((p[s:e], m[s:e], v[s:e]), tuple(t.cpu() for t in (ip, ig, im, iv)), h, cls is FusedAdamW, "range")


# --------------------------------------------------------------------------- row-split kernel
def _token_lists(R, kind, gen):
    if kind == "one_row":          # heavy duplicates: every token in one row
        return torch.full((1000,), R // 2, dtype=torch.int64)
    half = torch.randperm(R, generator=gen)[: max(1, R // 2)]
    if kind == "half":             # about half the rows untouched, each touched row several times
        return half[torch.randint(0, half.numel(), (4 * R,), generator=gen)]
    if kind == "many":             # more tokens than the 65536-workgroup cap of mode 1
        return torch.randint(0, R, (70000,), generator=gen)
    assert kind == "out_of_range"  # ids outside the table mixed in: skipped by the kernel's bound check
    rows = half[torch.randint(0, half.numel(), (4 * R,), generator=gen)]
    rows[::3] = -100
    rows[1::5] = R
    return rows


ROW_HYPER = [
    (HYPER_SETS[2], True),
    (HYPER_SETS[2], False),
    (dict(HYPER_SETS[2], maximize=True), True),   # grad_scale 0.5 and maximize
]


@pytest.mark.parametrize("hi", range(len(ROW_HYPER)), ids=["adamw", "adam_l2", "adamw_scale_maximize"])
@pytest.mark.parametrize("kind", ["one_row", "half", "many", "out_of_range"])
@pytest.mark.parametrize("R,C", [(300, 8), (64, 1152), (5, 4)])
def test_row_split_step_matches_dense_step_and_fp64(R, C, kind, hi):
    h, decoupled = ROW_HYPER[hi]
    gen = torch.Generator().manual_seed(R + C)
    rows = _token_lists(R, kind, gen)
    valid = rows[(rows >= 0) & (rows < R)]
    touched = torch.zeros(R, dtype=torch.bool)
    touched[valid] = True
    assert touched.any()
    if kind != "many":
        assert not touched.all()
    ip, ig, im, iv = make_inputs(R * C, h["step"], 5)
    ig = ig * touched.repeat_interleave(C)   # a step's table gradient is zero on the untouched rows
    inputs = (ip, ig, im, iv)
    dense = _flat_run(inputs, h, decoupled, shadow=True)
    p, g, m, v = (t.to(DEV).clone() for t in inputs)
    g.view(R, C)[~touched.to(DEV)] = float("nan")   # mode 0 must not read the gradient
    shadow = torch.full((R * C,), 13.0, dtype=BF, device=DEV)
    rows_d = rows.to(DEV)
    mask = torch.full((R,), 7, dtype=torch.int32, device=DEV)
    mask.zero_()
    mask.index_fill_(0, valid.to(DEV), 1)
    Fu.adam_rows_step(p, g, m, v, shadow, C, mask, None, 0, *_args(h), decoupled=decoupled)
    torch.cuda.synchronize()
    t_d = touched.to(DEV)
    for a, b, what in zip((p, m, v, shadow), inputs[:1] + inputs[2:] + (None,), ("p", "m", "v", "shadow")):
        if b is not None:  # mode 0 leaves the touched rows alone
            assert torch.equal(a.view(R, C)[t_d].cpu(), b.view(R, C)[touched]), f"mode 0 wrote touched rows of {what}"
    assert torch.equal(mask.cpu(), touched.to(torch.int32)), "mode 0 must not change the mask"
    Fu.adam_rows_step(p, g, m, v, shadow, C, mask, rows_d, 1, *_args(h), decoupled=decoupled)
    torch.cuda.synchronize()
    for a, b, what in zip((p, m, v, shadow), dense[:4], ("p", "m", "v", "shadow")):
        assert torch.equal(a, b), f"{what}: row-split step differs from the dense step"
    assert torch.equal(shadow, p.to(BF))
    _check_fp64((p, m, v), inputs, h, decoupled, f"rows {R}x{C} {kind}")
    assert g.view(R, C)[t_d].abs().max().item() == 0.0, "touched rows' gradient must be cleared"
    assert torch.isnan(g.view(R, C)[~t_d]).all(), "untouched rows' gradient must not be written"
    assert torch.equal(mask.cpu(), 2 * touched.to(torch.int32)), "mask: 2 on the touched rows, 0 elsewhere"


# --------------------------------------------------------------------------- list mode
LIST_SHAPES = [(1,), (8191,), (8192,), (8193,), (3 * 8192,), (33, 17)] + [(i % 7 + 1,) for i in range(200)]
BF16_EXTRA = 2.0 ** -8   # one bf16 rounding of the stored value


def _list_case(cls, h, dtypes, seed=11):
    """One optimizer over LIST_SHAPES (dtype per tensor from ``dtypes``, cycled), warm state seeded
    through ``state[p]``, one step -> (params, inputs per tensor as the kernel saw them)."""
    total = sum(int(torch.Size(s).numel()) for s in LIST_SHAPES)
    flat = make_inputs(total, h["step"], seed)
    params, inputs, off = [], [], 0
    for i, shape in enumerate(LIST_SHAPES):
        k = int(torch.Size(shape).numel())
        dt = dtypes[i % len(dtypes)]
        p, g, m, v = (t[off:off + k].view(shape).to(dt) for t in flat)
        off += k
        inputs.append(tuple(t.float().reshape(-1) for t in (p, g, m, v)))
        q = torch.nn.Parameter(p.to(DEV))
        q.grad = g.to(DEV)
        params.append((q, m.to(DEV), v.to(DEV)))
    opt = cls([q for q, _, _ in params], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"],
              maximize=h["maximize"])
    for q, m, v in params:
        opt.state[q] = {"step": torch.tensor(float(h["step"] - 1)), "exp_avg": m, "exp_avg_sq": v}
    opt.step(grad_scale=h["grad_scale"])
    torch.cuda.synchronize()
    return opt, [q for q, _, _ in params], inputs


def _check_list(opt, params, inputs, h, decoupled, what):
    for dt in {q.dtype for q in params}:
        sel = [i for i, q in enumerate(params) if q.dtype == dt]
        got = tuple(torch.cat([x[i].detach().float().reshape(-1).cpu() for i in sel]) for x in (
            params, [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params]))
        inp = tuple(torch.cat([inputs[i][j] for i in sel]) for j in range(4))
        ref, sc = A.scales(*inp, h, decoupled)
        A.assert_within(got, ref, sc, A.k_for(h, decoupled, inp), f"{what} {dt}",
                        extra=BF16_EXTRA if dt == BF else None)
    for q, inp in zip(params, inputs):
        st = opt.state[q]
        assert float(st["step"]) == float(h["step"])
        assert st["exp_avg"].dtype == q.dtype and st["exp_avg_sq"].dtype == q.dtype
        assert torch.equal(q.grad.float().cpu().reshape(-1), inp[1]), "the gradient must stay as given"


@pytest.mark.parametrize("si", range(len(HYPER_SETS)))
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_list_mode_fp32_matches_fp64(cls, si):
    h = HYPER_SETS[si]
    opt, params, inputs = _list_case(cls, h, [torch.float32])
    _check_list(opt, params, inputs, h, cls is FusedAdamW, f"{cls.__name__} list fp32 set {si}")


@pytest.mark.parametrize("si", range(len(HYPER_SETS)))
@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_list_mode_bf16_within_one_rounding_of_fp64(cls, si):
    """bf16 parameters with bf16 state: one step from bf16 values against ``adam_ref`` fed the same
    values; each of p, m, v within one bf16 rounding (2⁻⁸·|ref|) plus the fp32 bound."""
    h = HYPER_SETS[si]
    opt, params, inputs = _list_case(cls, h, [BF])
    assert all(q.dtype == BF for q in params)
    _check_list(opt, params, inputs, h, cls is FusedAdamW, f"{cls.__name__} list bf16 set {si}")


@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam])
def test_list_mode_mixed_group_steps_both_dtypes(cls):
    h = HYPER_SETS[1]
    opt, params, inputs = _list_case(cls, h, [torch.float32, BF, BF])
    assert len(opt.param_groups) == 1 and {q.dtype for q in params} == {torch.float32, BF}
    for q, inp in zip(params, inputs):  # every tensor stepped (a skipped dtype would keep its moments)
        assert not torch.equal(opt.state[q]["exp_avg"].float().reshape(-1).cpu(), inp[2])
    _check_list(opt, params, inputs, h, cls is FusedAdamW, f"{cls.__name__} list mixed")
