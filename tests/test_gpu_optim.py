"""FusedAdamW / FusedAdam (fastfourierconvolution_amd/optim.py) on the GPU: the ops under torch.library.opcheck,
five steps against torch.optim.AdamW / Adam in float64 on the CPU (bound: tests/optim_refs.py, TOL = 1e-6 times the
sum of the absolute terms of each element's five updates), parameters without a gradient, the state dict in both
directions, one training iteration against torch's foreach AdamW, the LR schedule inside a captured graph and the
adaptive-weight critic step.

Observed on the first MI355X run: five steps over Discriminator32's 16 tensors (2.9 M elements) take p 0.126, m 0.060,
v 0.147 of the bound with FusedAdamW and p 0.078, m 0, v 0.106 with FusedAdam at beta1 = 0; the training iteration
differs from torch's foreach AdamW by 2.7e-6 normwise at most; the slowest test is opcheck at 2.5 s."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import optim_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _F():
    import fastfourierconvolution_amd as F
    return F


def _models(sn_hip=False):
    F = _F()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):   # the model constructors print their channel split
        G = F.FGenerator32(128, 4)
    D = F.Discriminator32(sn=True, mg=4)
    G, D = G.to(DEV).train(), D.to(DEV).train()
    return G, (F.set_sn_hip(D) if sn_hip else D)


def _batch(B=2):
    gen = torch.Generator().manual_seed(11)
    return (torch.randn(B, 128, generator=gen).to(DEV), torch.randn(B, 128, generator=gen).to(DEV),
            (torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1).to(DEV))


# --------------------------------------------------------------------------- opcheck
def test_opcheck():
    from fastfourierconvolution_amd import _autograd as ag
    gen = torch.Generator().manual_seed(1)
    shapes = [(3, 5), (8192 + 3,), (0,), (1,)]
    mk = lambda s=1.0: [(s * torch.randn(x, generator=gen)).to(DEV) for x in shapes]   # noqa: E731
    state = torch.zeros(2, ag.OPTIM_STATE, dtype=torch.int64, device=DEV)
    args = (mk(0.1), mk(), mk(0.3), [t.square() for t in mk()], state[1], 2e-4, 0.5, 0.999, 1e-8, 0.01, 4, 0)
    for op, a in ((torch.ops.ffc.optim_step.default, args), (torch.ops.ffc.optim_tick.default, (state,))):
        res = torch.library.opcheck(op, a, None, raise_exception=False)
        bad = {k: v for k, v in res.items() if v != "SUCCESS"}
        assert not bad, f"{op}: {bad}"


# --------------------------------------------------------------------------- five steps against float64 torch
def _five_steps(cls_name, kw):
    F = _F()
    with contextlib.redirect_stdout(io.StringIO()):
        shapes = [p.shape for p in F.Discriminator32(sn=True, mg=4).parameters()]
    gen = torch.Generator().manual_seed(21)
    init = [0.05 * torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(5)]
    dev = [torch.nn.Parameter(x.to(DEV)) for x in init]
    cpu = [torch.nn.Parameter(x.double()) for x in init]
    opt = getattr(F, cls_name)(dev, **kw)
    ref = getattr(torch.optim, cls_name[5:])(cpu, foreach=True, **kw)
    for gs in grads:
        for p, q, g in zip(dev, cpu, gs):
            p.grad, q.grad = g.to(DEV), g.double()
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    mode = R.ADAMW if cls_name == "FusedAdamW" else R.ADAM
    case = dict(betas=kw["betas"], lr=kw["lr"], T=0, t0=0, eps=kw["eps"], wd=kw["weight_decay"], mode=mode)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, (p, q, x) in enumerate(zip(dev, cpu, init)):
        st, rs = opt.state[p], ref.state[q]
        z = np.zeros(x.numel())
        run = R.run(case, x.numpy().reshape(-1), [gs[i].numpy().reshape(-1) for gs in grads], z, z)
        want = (q.detach().numpy(), rs["exp_avg"].numpy(), rs["exp_avg_sq"].numpy())
        for a, b in zip(run[:3], want):    # the restated five steps are torch's
            assert np.linalg.norm(a - b.reshape(-1)) <= 1e-12 * np.linalg.norm(b)
        got = (p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
        for key, val in R.shares(got, (*want, run[3])).items():
            worst[key] = max(worst[key], val)
    print(f"OBS {cls_name} five steps over {len(dev)} tensors, {sum(p.numel() for p in dev)} elements: "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert float(ref.state[cpu[0]]["step"]) == 5 and opt.state_dict()["state"][0]["step"].item() == 5


def test_fused_adamw_five_steps_match_fp64_torch():
    _five_steps("FusedAdamW", dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.01))


def test_fused_adam_five_steps_match_fp64_torch():
    _five_steps("FusedAdam", dict(lr=2e-4, betas=(0.0, 0.9), eps=1e-8, weight_decay=0.0))


# --------------------------------------------------------------------------- parameters without a gradient
def test_parameter_without_gradient_is_skipped():
    F = _F()
    a, b = (torch.nn.Parameter(torch.ones(7, device=DEV)) for _ in range(2))
    opt = F.FusedAdamW([a, b], lr=1e-2)
    a.grad = torch.ones_like(a)
    opt.step()
    assert torch.equal(b, torch.ones_like(b)) and not opt.state.get(b)
    assert not torch.equal(a, torch.ones_like(a)) and set(opt.state[a]) == {"exp_avg", "exp_avg_sq"}
    assert set(opt.state_dict()["state"]) == {0}
    opt.zero_grad()
    opt.step()      # no gradient at all: nothing runs, the count stays
    assert opt.state_dict()["state"][0]["step"].item() == 1


def test_constructor_rejections():
    F = _F()
    w = torch.nn.Parameter(torch.zeros(3, device=DEV))
    with pytest.raises(NotImplementedError, match="fp32"):
        F.FusedAdamW([torch.nn.Parameter(torch.zeros(3, device=DEV, dtype=torch.float16))])
    with pytest.raises(NotImplementedError, match="fp32"):
        F.FusedAdam([w, torch.nn.Parameter(torch.zeros(3, device=DEV, dtype=torch.float64))])
    with pytest.raises(NotImplementedError, match="GPU only"):
        F.FusedAdamW([w, torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(NotImplementedError, match="amsgrad"):
        F.FusedAdamW([w], amsgrad=True)
    opt = F.FusedAdamW([w], lr=1e-3, decay_steps=10)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5)     # a host scheduler still drives param_groups
    assert opt.param_groups[0]["lr"] == 5e-4 and sched.get_last_lr() == [5e-4] and opt.get_last_lr() == [5e-4]


# --------------------------------------------------------------------------- state dict
def _pair(cls, seed, **kw):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in ((5, 3), (8192 + 1,), (2,))]
    return ps, cls(ps, **kw)


def _grads(ps, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)


def test_state_dict_round_trip_with_torch():
    F = _F()
    kw = dict(lr=1e-3, betas=(0.5, 0.999), weight_decay=0.01)
    ps, ours = _pair(F.FusedAdamW, 3, decay_steps=8, **kw)
    for k in range(2):
        _grads(ps, 30 + k)
        ours.step()
        ours.lr_step()
    sd = ours.state_dict()
    assert sd["param_groups"][0]["ffc_lr_ticks"] == 2 and all(float(s["step"]) == 2 for s in sd["state"].values())
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    # ours -> torch: the moments and the count arrive, the next steps agree to rounding (torch has no schedule:
    # it gets the decayed lr by hand)
    qs, theirs = _pair(torch.optim.AdamW, 3, foreach=False, **kw)
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    theirs.load_state_dict(copy.deepcopy(sd))    # torch's load_state_dict keeps the tensors it is handed
    assert all(float(theirs.state[q]["step"]) == 2 and torch.equal(theirs.state[q]["exp_avg"], ours.state[p]["exp_avg"])
               for q, p in zip(qs, ps))
    # torch -> ours, through torch's own state dict: the copy continues bit for bit like the original
    rs, back = _pair(F.FusedAdamW, 3, decay_steps=8, **kw)
    with torch.no_grad():
        for r, p in zip(rs, ps):
            r.copy_(p)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert back.get_last_lr() == ours.get_last_lr() == [1e-3 * (1 - 2 / 8)]
    theirs.param_groups[0]["lr"] = 1e-3 * (1 - 2 / 8)
    for opt, xs in ((ours, ps), (back, rs), (theirs, qs)):
        _grads(xs, 40)
        opt.step()
    torch.cuda.synchronize()
    for p, r, q in zip(ps, rs, qs):
        assert torch.equal(p, r) and torch.equal(ours.state[p]["exp_avg"], back.state[r]["exp_avg"])
        assert torch.equal(ours.state[p]["exp_avg_sq"], back.state[r]["exp_avg_sq"])
        assert float((p - q).detach().norm()) <= 1e-5 * float(q.detach().norm()), "the step after loading into torch.optim.AdamW"
        assert float(theirs.state[q]["step"]) == 3
    assert back.state_dict()["state"][0]["step"].item() == 3
    # torch -> ours from a torch run
    _grads(qs, 41)
    theirs.step()
    ts, fresh = _pair(F.FusedAdamW, 3, **kw)
    with torch.no_grad():
        for t, q in zip(ts, qs):
            t.copy_(q)
    fresh.load_state_dict(copy.deepcopy(theirs.state_dict()))
    theirs.param_groups[0]["lr"] = fresh.param_groups[0]["lr"] = 1e-3
    for opt, xs in ((fresh, ts), (theirs, qs)):
        _grads(xs, 42)
        opt.step()
    for t, q in zip(ts, qs):
        assert float((t - q).detach().norm()) <= 1e-5 * float(q.detach().norm())
        assert float((fresh.state[t]["exp_avg_sq"] - theirs.state[q]["exp_avg_sq"]).norm()) <= \
            1e-5 * float(theirs.state[q]["exp_avg_sq"].norm())
    assert fresh.state_dict()["state"][0]["step"].item() == 5


# --------------------------------------------------------------------------- a training iteration
def test_train_iteration_matches_torch_foreach_adamw():
    """Bound 1e-5 normwise per tensor, the project's kernel-level bound: both runs see bit-identical gradients
    (the layers' kernels are deterministic), so only the update's own rounding differs."""
    from fastfourierconvolution_amd.training import train_iteration
    F = _F()
    z_g, z_d, real = _batch()
    res = []
    for fused in (True, False):
        G, D = _models()
        kw = dict(lr=2e-4, betas=(0.5, 0.999))
        if fused:
            oG, oD = F.FusedAdamW(G.parameters(), **kw), F.FusedAdamW(D.parameters(), **kw)
        else:
            oG, oD = (torch.optim.AdamW(m.parameters(), foreach=True, **kw) for m in (G, D))
        init = [p.detach().clone() for m in (G, D) for p in m.parameters()]
        torch.manual_seed(5)       # the NoiseInjection draws
        train_iteration(G, D, oG, oD, z_g, z_d, real)
        torch.cuda.synchronize()
        res.append(([p.detach().clone() for m in (G, D) for p in m.parameters()], init))
    (a, ia), (b, ib) = res
    assert all(torch.equal(x, y) for x, y in zip(ia, ib)), "the two runs start from different weights"
    worst = 0.0
    assert sum(not torch.equal(y, i) for y, i in zip(b, ib)) > len(b) // 2, "the iteration moved few parameters"
    for x, y in zip(a, b):
        worst = max(worst, float((x - y).norm()) / max(float(y.norm()), 1e-30))
    print(f"OBS train_iteration: worst normwise difference {worst:.3e}")
    assert worst <= 1e-5, worst


# --------------------------------------------------------------------------- the schedule inside a captured graph
def test_schedule_lives_in_the_captured_graph():
    from fastfourierconvolution_amd.graphs import capture_step
    from fastfourierconvolution_amd.training import discriminator_step, generator_step
    F = _F()
    z_g, z_d, real = _batch()
    G, D = _models()
    lr0 = 2e-4
    kw = dict(lr=lr0, betas=(0.5, 0.999), weight_decay=0.0, decay_steps=4)
    oG, oD = F.FusedAdamW(G.parameters(), **kw), F.FusedAdamW(D.parameters(), **kw)

    def step():
        generator_step(G, D, oG, oD, z_g)
        discriminator_step(G, D, oG, oD, z_d, real)
        oG.lr_step()
        oD.lr_step()
    g = capture_step(step, warmup=1)
    if g is None:
        pytest.skip("graph capture is not available on this machine")
    oG.reset_lr_schedule()
    oD.reset_lr_schedule()
    params = [p for m in (G, D) for p in m.parameters()]
    for k in range(1, 6):
        before = [p.detach().clone() for p in params]
        g.replay()
        torch.cuda.synchronize()
        want = [lr0 * max(0.0, 1 - k / 4)]
        assert oG.get_last_lr() == want and oD.get_last_lr() == want, (k, oG.get_last_lr(), want)
        same = [torch.equal(p, q) for p, q in zip(params, before)]
        if k == 5:
            assert all(same), "lr_eff = 0 in the 5th replay must leave every parameter bit-unchanged"
        else:
            assert sum(same) < len(same) // 2, f"replay {k} left {sum(same)} of {len(same)} parameters unchanged"
    assert want == [0.0] and oG.state_dict()["state"][0]["step"].item() == 6


# --------------------------------------------------------------------------- the adaptive-weight critic step
def test_aw_discriminator_step_with_fused_adamw():
    from fastfourierconvolution_amd.training import aw_discriminator_step
    F = _F()
    z_g, z_d, real = _batch()
    G, D = _models(sn_hip=True)
    oG = F.FusedAdamW(G.parameters(), lr=2e-4, betas=(0.5, 0.999))
    oD = F.FusedAdamW(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    before = [p.detach().clone() for p in D.parameters()]
    loss = aw_discriminator_step(G, D, oG, oD, z_d, real, F.aw_method())
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in D.parameters())
    assert sum(not torch.equal(p, q) for p, q in zip(D.parameters(), before)) > len(before) // 2
