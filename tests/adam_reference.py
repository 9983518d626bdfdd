"""fp64 reference of one Adam / AdamW step, the inputs and the tolerance the optimizer-kernel tests
share (tests/test_optimizer_kernels_gpu.py on the MI355X, tests/test_adam_reference.py on CPU).

Kept in a module of its own because the GPU test module skips itself at import without a device,
and the CPU suite must be able to run the checks that the inputs and the bound can tell a wrong
step from a right one.

Tolerance: elementwise |x_kernel − x_ref| ≤ K · 2⁻²⁴ · scale, with
    scale_p = |p_ref| + |Δ_ref|,  scale_m = |m_ref| + |g_eff|,  scale_v = v_ref + g_eff²
(g_eff: the gradient after scale, sign and the L2 term). K is 4x the worst ratio err / (2⁻²⁴ · scale)
of the SAME formula evaluated in fp32 with plain torch ops (``adam_fp32``) against fp64: the
reference's own rounding, not the kernel's; the factor 4 covers FMA contraction and a different
operation order in the kernel. ``k_for`` measures it per hyper-parameter set and decay kind on the
calibration inputs (``make_inputs`` at n = 1023 and 262147, seed 0: the flat tests' inputs) and, when
a test passes its own inputs, on those too (the larger ratio counts). Measured on CPU (x86-64,
torch 2.x), worst of the two sizes:

    set (lr, betas, eps, wd, step, grad_scale, maximize)     decay      ratio p  ratio m  ratio v
    0   1e-2 (0.9, 0.95)  1e-8 0.1   1     1.0  False         decoupled   3.33     0.11     0.10
                                                              L2         12.79  5067.11  5299.59
    1   1e-2 (0.9, 0.95)  1e-8 0.1   7     0.25 True          decoupled   5.95     1.09     2.16
                                                              L2         12.78     2.86     3.47
    2   3e-3 (0.9, 0.999) 1e-3 0.05  1000  0.5  False         decoupled  13.01     1.09     2.16
                                                              L2          2.95     3.56     2.17

so K_p = 13 … 52, K_m and K_v = 0.4 … 14, except set 0 with L2 decay, where K_m and K_v are 2.0e4 and
2.1e4: from zero moments m = 0.1·g_eff and v = 0.05·g_eff² with g_eff = g + wd·p, and among 262147
elements one has g ≈ −wd·p, so its g_eff (the scale) is ~1e-4 of the terms whose rounding it carries.
The scale is kept as stated and K absorbs it; p of the same set is unaffected (Δ ≈ lr·sign(g_eff)).
test_adam_reference.py re-measures the p ratios on every CPU run.
"""
from __future__ import annotations

import math

import torch

# (lr, b1, b2, eps, wd, step, grad_scale, maximize)
HYPER_SETS = (
    dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, step=1, grad_scale=1.0, maximize=False),
    dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, step=7, grad_scale=0.25, maximize=True),
    dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-3, wd=0.05, step=1000, grad_scale=0.5, maximize=False),
)

EPS32 = 2.0 ** -24

MUTATIONS = ("swap_decoupled", "step_minus_1", "drop_bc2", "eps_in_sqrt", "eps_before_bc2", "scale_after_l2")


def make_inputs(n: int, step: int, seed: int = 0):
    """fp32 CPU (p, g, m, v): p ~ N(0,1); g ~ N(0,1) times a log-spaced factor 1e-4 … 10; warm
    moments m ~ 0.1·N(0,1), v = (0.1·N(0,1))², zero for step 1."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * torch.logspace(-4, 1, n)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = 0.1 * torch.randn(n, generator=gen)
        v = (0.1 * torch.randn(n, generator=gen)) ** 2
    return p, g, m, v


def _adam64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, maximize, decoupled, mutation=None):
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    if mutation == "swap_decoupled":
        decoupled = not decoupled
    sign = -1.0 if maximize else 1.0
    if decoupled:
        g = sign * (g * grad_scale)
        p = p * (1.0 - lr * wd)
    elif mutation == "scale_after_l2":
        g = (sign * g + wd * p) * grad_scale  # (wrong) the L2 term scaled with the gradient
    else:
        g = sign * (g * grad_scale) + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    t = step - 1 if mutation == "step_minus_1" else step
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 if mutation == "drop_bc2" else 1.0 - b2 ** t
    if mutation == "eps_in_sqrt":
        denom = (v / bc2 + eps).sqrt()
    elif mutation == "eps_before_bc2":
        denom = (v.sqrt() + eps) / math.sqrt(bc2) if bc2 > 0 else torch.full_like(v, float("inf"))
    else:
        denom = v.sqrt() / math.sqrt(bc2) + eps if bc2 > 0 else torch.full_like(v, float("inf"))
    delta = (lr / bc1) * m / denom if bc1 != 0 else torch.full_like(m, float("nan"))
    return p - delta, m, v, delta


def adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, maximize, decoupled):
    """One step in fp64 -> (p, m, v, Δ): the gradient is scaled, then negated (maximize), then
    p *= 1 − lr·wd (decoupled) or g += wd·p (L2); m += (g − m)(1 − β1); v = β2·v + (1 − β2)·g²;
    Δ = (lr / bc1) · m / (sqrt(v) / sqrt(bc2) + eps); p −= Δ."""
    return _adam64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, maximize, decoupled)


def adam_ref_mutated(mutation, p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, maximize, decoupled):
    """``adam_ref`` with one deliberate mistake (``MUTATIONS``)."""
    assert mutation in MUTATIONS
    return _adam64(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, maximize, decoupled, mutation)


def g_eff_ref(p, g, wd, grad_scale, maximize, decoupled):
    """The gradient the moments see, fp64."""
    p, g = p.detach().double().cpu(), g.detach().double().cpu()
    g = g * grad_scale
    if maximize:
        g = -g
    return g if decoupled else g + wd * p


def adam_fp32(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, maximize, decoupled):
    """The same formula in fp32 with plain torch ops -> (p, m, v): the yardstick for K."""
    p, g, m, v = (t.detach().float().cpu().clone() for t in (p, g, m, v))
    # scalar factors (1 − β, 1 − lr·wd, lr / bc1, sqrt(bc2)) are formed in double and rounded to
    # fp32 once, when torch multiplies an fp32 tensor by a Python number
    g = g * grad_scale
    if maximize:
        g = -g
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def scales(p, g, m, v, hyper: dict, decoupled: bool):
    """-> (ref (p, m, v) fp64, scale (p, m, v) fp64) for one step from (p, g, m, v)."""
    rp, rm, rv, delta = adam_ref(p, g, m, v, decoupled=decoupled, **hyper)
    ge = g_eff_ref(p, g, hyper["wd"], hyper["grad_scale"], hyper["maximize"], decoupled)
    return (rp, rm, rv), (rp.abs() + delta.abs(), rm.abs() + ge.abs(), rv + ge * ge)


_K_CACHE: dict = {}
CALIBRATION_SIZES = (1023, 262147)


def fp32_ratios(p, g, m, v, hyper: dict, decoupled: bool):
    """Worst err / (2⁻²⁴ · scale) of ``adam_fp32`` against fp64 on these inputs, for (p, m, v)."""
    ref, sc = scales(p, g, m, v, hyper, decoupled)
    return worst_ratios(adam_fp32(p, g, m, v, decoupled=decoupled, **hyper), ref, sc)


def k_for(hyper: dict, decoupled: bool, inputs=None):
    """(K_p, K_m, K_v) = 4 x the fp32 formula's worst ratio on the calibration inputs (and on
    ``inputs`` = (p, g, m, v), when given)."""
    key = (tuple(sorted(hyper.items())), decoupled)
    if key not in _K_CACHE:
        worst = [0.0, 0.0, 0.0]
        for n in CALIBRATION_SIZES:
            r = fp32_ratios(*make_inputs(n, hyper["step"], 0), hyper, decoupled)
            worst = [max(a, b) for a, b in zip(worst, r)]
        _K_CACHE[key] = worst
    worst = _K_CACHE[key]
    if inputs is not None:
        worst = [max(a, b) for a, b in zip(worst, fp32_ratios(*inputs, hyper, decoupled))]
    return tuple(4.0 * r for r in worst)


def worst_ratios(got, ref, scale):
    """max over elements of |got − ref| / (2⁻²⁴ · scale), per quantity (0 / 0 counts as 0, anything
    non-finite as inf)."""
    out = []
    for x, r, s in zip(got, ref, scale):
        err = (x.detach().double().cpu().reshape(-1) - r.reshape(-1)).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / (EPS32 * s.reshape(-1)))
        ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
        out.append(ratio.max().item() if ratio.numel() else 0.0)
    return out


def assert_within(got, ref, scale, K, what="", extra=None):
    """Elementwise |got − ref| ≤ K·2⁻²⁴·scale (+ ``extra``, e.g. one bf16 rounding), for p, m, v."""
    for name, x, r, s, k in zip("pmv", got, ref, scale, K):
        x = x.detach().double().cpu().reshape(-1)
        r, s = r.reshape(-1), s.reshape(-1)
        err = (x - r).abs()
        lim = k * EPS32 * s
        if extra is not None:
            lim = lim + extra * r.abs()
        bad = ~(err <= lim)  # NaN counts as bad
        worst = torch.where(err > 0, err / lim, torch.zeros_like(err))  # (0 / 0: within)
        worst = worst.max().item() if worst.numel() else 0.0
        print(f"{what} {name}: worst err / bound = {worst:.3g}")
        assert not bad.any(), (f"{what} {name}: {int(bad.sum())} of {x.numel()} elements out of bound, "
                               f"worst err / bound = {worst:.3g}")
