"""fp64 restatement of torch.optim's single-tensor Adam / AdamW (amsgrad = maximize = False) and of the reference's LR
schedule LambdaLR(opt, lambda s: 1 - s / T), written from the formulas of include/ffc_amd.h, with the case tables of
tests/test_optim_refs_cpu.py, tests/test_gpu_optim_abi.py and tests/test_gpu_optim.py.

Bound per result element: |got - ref| <= TOL * sum |terms|, the terms being the summands of that element's update
  p   |p|, |lr wd p| and |step_size m / denom|      (m, v: the new moments)
  m   |m| and |(g - m)(1 - beta1)|
  v   |beta2 v| and |(1 - beta2) g^2|
After k steps the bound is the sum of the k steps' bounds, the terms taken along the float64 run: a step passes the
error it inherits on with a factor of at most 1 (beta1 for m, beta2 for v, 1 - lr wd for p), so the errors of the
steps add, each in proportion to its own step's terms -- an element that is large in one step and nearly cancels in
the next still carries the first step's rounding.

TOL = 1e-6 is the smallest power of ten at which plain fp32 torch on the CPU (torch.optim.AdamW / Adam,
foreach=False) stays under ROOM = 0.25 of every bound over all of CASES: the worst share is 0.159 (v of "Adam, tiny
gradients"; p takes 0.143 there and 0.135 in "fgan128 AdamW, first step"), so 1e-7 would leave it 1.59.
test_optim_refs_cpu.py asserts both.  (Worst case by counting roundings: p * decay, the final fma and about six
roundings on the way to m / denom, each 2^-24 relative: under 0.5 of the bound.)"""
import math

import numpy as np

TOL = 1e-6
ROOM = 0.25
ADAMW, ADAM = 0, 1
DEFECTS = ("no_bias_correction", "coupled_decay", "eps_in_sqrt", "t_off_by_one", "stale_schedule", "beta2_on_g2")


def lr_eff(lr0, s, T):
    """the reference's lambda, clamped at 0: LambdaLR(opt, lambda s: 1 - s / T) after s scheduler steps; T = 0: lr0"""
    return lr0 * max(0.0, 1 - s / T) if T else lr0


def step(p, g, m, v, t, lr, beta1, beta2, eps, wd, mode, defect=None):
    """one update in float64: the state before the step whose count is t (>= 1) -> (p, m, v, scales (p, m, v))"""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    if defect == "t_off_by_one":
        t = t + 1
    coupled = mode == ADAM or defect == "coupled_decay"
    decay = 0.0 if coupled else lr * wd
    if coupled:
        g = g + wd * p
    p1 = p * (1.0 - decay)
    dm = (g - m) * (1.0 - beta1)
    m1 = m + dm
    if defect == "beta2_on_g2":
        a, b = (1.0 - beta2) * v, beta2 * g * g
    else:
        a, b = beta2 * v, (1.0 - beta2) * g * g
    v1 = a + b
    bc1 = 1.0 if defect == "no_bias_correction" else 1.0 - beta1 ** t
    bc2 = 1.0 if defect == "no_bias_correction" else 1.0 - beta2 ** t
    if defect == "eps_in_sqrt":
        denom = np.sqrt(v1 / bc2 + eps)
    else:
        denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        upd = (lr / bc1) * m1 / denom
    p2 = p1 - upd
    return p2, m1, v1, (np.abs(p) + np.abs(decay * p) + np.abs(upd), np.abs(m) + np.abs(dm), np.abs(a) + np.abs(b))


# ---------------------------------------------------------------------------- cases
# mode, betas, wd, lr, t0 (steps already taken), steps, T (decay_steps; the schedule ticks after every step), gscale
def _case(name, mode, betas, wd, lr=2e-4, t0=0, steps=1, T=0, gscale=1.0, eps=1e-8):
    return dict(name=name, mode=mode, betas=betas, wd=wd, lr=lr, t0=t0, steps=steps, T=T, gscale=gscale, eps=eps)


CASES = [
    _case("fgan128 AdamW, first step", ADAMW, (0.5, 0.999), 0.01),
    _case("fgan128 AdamW, five steps", ADAMW, (0.5, 0.999), 0.01, steps=5),
    _case("fgan128 AdamW, five steps under the schedule", ADAMW, (0.5, 0.999), 0.01, steps=5, T=4),
    _case("AdamW defaults, no decay", ADAMW, (0.9, 0.999), 0.0, lr=1e-3, steps=5),
    _case("SNGAN Adam, beta1 = 0", ADAM, (0.0, 0.9), 0.0, steps=5),
    _case("SNGAN Adam, beta1 = 0, L2", ADAM, (0.0, 0.9), 0.01, steps=5),
    _case("Adam defaults, L2", ADAM, (0.9, 0.999), 0.01, lr=1e-3, steps=5),
    _case("AdamW at t = 100000", ADAMW, (0.5, 0.999), 0.01, t0=99999),
    _case("tiny gradients, five steps", ADAMW, (0.5, 0.999), 0.01, steps=5, gscale=1e-5),
    _case("Adam, tiny gradients", ADAM, (0.9, 0.999), 0.0, lr=1e-3, gscale=1e-5),
]
N = 4099


def inputs(case, n=N, seed=0):
    """fp32 arrays: p ~ N(0, 0.1), one g ~ N(0, gscale) per step, and for t0 > 0 moments as after many such steps"""
    rng = np.random.default_rng(1000 + seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    gs = [(case["gscale"] * rng.standard_normal(n)).astype(np.float32) for _ in range(case["steps"])]
    if case["t0"]:
        m = (0.3 * case["gscale"] * rng.standard_normal(n)).astype(np.float32)
        v = (case["gscale"] ** 2 * (0.5 + rng.random(n))).astype(np.float32)
    else:
        m, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    return p, gs, m, v


def run(case, p, gs, m, v, defect=None):
    """the case's steps in float64, the schedule ticking after each -> (p, m, v, scales summed over the steps)"""
    b1, b2 = case["betas"]
    total = None
    for k, g in enumerate(gs):
        s = max(k - 1, 0) if defect == "stale_schedule" else k
        lr = lr_eff(case["lr"], s, case["T"])
        p, m, v, sc = step(p, g, m, v, case["t0"] + k + 1, lr, b1, b2, case["eps"], case["wd"], case["mode"], defect)
        total = sc if total is None else tuple(a + b for a, b in zip(total, sc))
    return p, m, v, total


def shares(got, ref, tol=TOL):
    """got (p, m, v), ref = run(...) -> {'p', 'm', 'v'}: the largest |got - ref| / (tol * scale); inf when not finite"""
    out = {}
    for k, x, r, s in zip("pmv", got, ref[:3], ref[3]):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        err = np.abs(x - r.reshape(-1))
        if not np.isfinite(x).all():
            out[k] = float("inf")
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / (tol * s.reshape(-1)))
        out[k] = float(q.max()) if q.size else 0.0
    return out


def torch_run(case, p, gs, m, v, dtype, foreach=False):
    """the case on torch.optim.AdamW / Adam on the CPU in ``dtype``, LambdaLR stepping after each step -> (p, m, v)"""
    import torch
    w = torch.nn.Parameter(torch.tensor(p, dtype=dtype))
    cls = torch.optim.AdamW if case["mode"] == ADAMW else torch.optim.Adam
    opt = cls([w], lr=case["lr"], betas=case["betas"], eps=case["eps"], weight_decay=case["wd"], foreach=foreach)
    opt.state[w] = dict(step=torch.tensor(float(case["t0"])), exp_avg=torch.tensor(m, dtype=dtype),
                        exp_avg_sq=torch.tensor(v, dtype=dtype))
    T = case["T"]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: max(0.0, 1 - s / T)) if T else None
    for g in gs:
        w.grad = torch.tensor(g, dtype=dtype)
        opt.step()
        if sched is not None:
            sched.step()
    st = opt.state[w]
    return w.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


# ---------------------------------------------------------------------------- the C ABI tests
ABI_NUMELS = (1, 3, 4, 5, 255, 256, 257, 70001)


def abi_inputs(numels, seed, gscale=1.0, zero=False):
    """per tensor fp32 (p, g, m, v): moments as in the middle of training; zero: g = m = v = 0"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for n in numels:
        p = (0.1 * rng.standard_normal(n)).astype(np.float32)
        if zero:
            z = np.zeros(n, dtype=np.float32)
            out.append((p, z, z.copy(), z.copy()))
        else:
            out.append((p, (gscale * rng.standard_normal(n)).astype(np.float32),
                        (0.3 * gscale * rng.standard_normal(n)).astype(np.float32),
                        (gscale ** 2 * (0.5 + rng.random(n))).astype(np.float32)))
    return out
