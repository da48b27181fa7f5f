"""Spectral norm on the GPU (set_sn_hip): the kernels of csrc/sn_kernels.hip through the ffc::sn_weight /
ffc::sn_weight_bwd ops against the float64 restatement of torch's hook (tests/sn_refs.py) at their edge
shapes, table-vs-single and run-to-run bitwise equality, the switch-off path against the hook itself,
and the critics with the switch on against the switch off.

Bounds: kernels against float64 1e-5 normwise (as tests/test_gpu_train_kernels.py); whole models, switch
on against switch off, 1e-4 normwise in fp32.  Every test prints what it measured.

Weights are N(0, 0.02); u and v are normalised N(0, 1) vectors, as torch initialises them.

Observed maxima on the first MI355X run (normwise): kernels against float64 at the edge shapes 1.9e-7
(eval-mode sigma of 512 x 8192), the per-layer route against the hook 2.5e-7 (eval-mode dW_orig), models
on against off 3.1e-6 (fc.weight_orig.grad of Discriminator32), their buffers 1.6e-7.
"""
import copy
import functools

import pytest
import torch

import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
import sn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_K = 1e-5    # kernels against float64
TOL_M = 1e-4    # models, fp32, switch on against switch off

# name: (weight shape, dim) -> the matrix (M, K)
CASES = {
    "conv3x3_64x27": ((64, 3, 3, 3), 0),        # K % 4 != 0: the 4-byte forms
    "linear_1x2048": ((1, 2048), 0),            # M = 1: u is one element, +-1
    "conv1x1_32x16": ((32, 16, 1, 1), 0),       # smaller than one wave
    "conv4x4_130x1040": ((130, 65, 4, 4), 0),   # > 1 row chunk and > 1 column chunk, ragged on both axes
    "convT_20x192": ((12, 20, 4, 4), 1),        # ConvTranspose2d(12, 20, 4): dim = 1, read through strides
    "conv4x4_512x8192": ((512, 512, 4, 4), 0),  # 16 MB: the two-axis split at full width
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(w_orig, u, v, g) on the CPU in fp32, and three float64 steps of the restatement; computed once"""
    shape, dim = CASES[name]
    gen = torch.Generator().manual_seed(NAMES.index(name) + 11)
    w = torch.randn(shape, generator=gen) * 0.02
    M = shape[dim]
    K = w.numel() // M
    u = torch.nn.functional.normalize(torch.randn(M, generator=gen), dim=0, eps=1e-12)
    v = torch.nn.functional.normalize(torch.randn(K, generator=gen), dim=0, eps=1e-12)
    g = torch.randn(shape, generator=gen)
    steps = []
    ru, rv = u, v
    for _ in range(3):
        rw, ru, rv, rs = R.sn_ref(w, ru, rv, dim, True)
        steps.append((rw, ru, rv, rs))
    return dict(w=w, u=u, v=v, g=g, dim=dim, M=M, K=K, steps=steps, eval=R.sn_ref(w, u, v, dim, False))


def _forward(names, training, state=None, save=True):
    """one ffc::sn_weight call over a table -> per job dict(w, u, v, sigma, saved); fresh device copies
    of the inputs unless ``state`` (a previous result) carries u / v on"""
    cs = [_case(n) for n in names]
    w_orig = [c["w"].to(DEV) for c in cs]
    u = [(state[i]["u"] if state else c["u"].to(DEV)).clone() for i, c in enumerate(cs)]
    v = [(state[i]["v"] if state else c["v"].to(DEV)).clone() for i, c in enumerate(cs)]
    w = [torch.full_like(t, float("nan")) for t in w_orig]
    sigma = torch.full((len(cs),), float("nan"), device=DEV)
    saved = torch.full((sum(c["M"] + c["K"] for c in cs) if save else 0,), float("nan"), device=DEV)
    torch.ops.ffc.sn_weight(w_orig, u, v, w, sigma, saved, [c["dim"] for c in cs], training)
    torch.cuda.synchronize()
    out, pos = [], 0
    for i, c in enumerate(cs):
        d = dict(w_orig=w_orig[i], w=w[i], u=u[i], v=v[i], sigma=sigma[i:i + 1])
        if save:
            d["saved"] = saved[pos:pos + c["M"] + c["K"]]
            pos += c["M"] + c["K"]
        out.append(d)
    return out


def _backward(names, fwd):
    cs = [_case(n) for n in names]
    saved = torch.cat([f["saved"] for f in fwd])
    sigma = torch.cat([f["sigma"] for f in fwd])
    out = torch.ops.ffc.sn_weight_bwd([c["g"].to(DEV) for c in cs], [f["w_orig"] for f in fwd], saved, sigma,
                                      [c["dim"] for c in cs])
    torch.cuda.synchronize()
    return out


def _check(what, out, ref, tol=TOL_K):
    assert not torch.isnan(out).any(), what
    e = R.normwise(out, ref)
    print(f"  {what}: {e:.2e}")
    assert e <= tol, (what, e)
    return e


def _same(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)


@pytest.mark.parametrize("name", NAMES)
def test_train_forward_against_float64(name):
    c = _case(name)
    (o,) = _forward([name], True)
    rw, ru, rv, rs = c["steps"][0]
    _check(f"{name} w", o["w"], rw)
    _check(f"{name} u'", o["u"], ru)
    _check(f"{name} v'", o["v"], rv)
    _check(f"{name} sigma", o["sigma"], rs.reshape(1))
    # the copies the backward reads are this call's u' and v'
    assert torch.equal(o["saved"][:c["M"]], o["u"]) and torch.equal(o["saved"][c["M"]:], o["v"])
    assert _same([o], _forward([name], True)), "two runs from the same state differ"


@pytest.mark.parametrize("name", NAMES)
def test_eval_forward_against_float64(name):
    c = _case(name)
    (o,) = _forward([name], False)
    rw, _, _, rs = c["eval"]
    _check(f"{name} eval w", o["w"], rw)
    _check(f"{name} eval sigma", o["sigma"], rs.reshape(1))
    assert torch.equal(o["u"].cpu(), c["u"]) and torch.equal(o["v"].cpu(), c["v"])   # bitwise untouched
    assert torch.equal(o["saved"][:c["M"]].cpu(), c["u"]) and torch.equal(o["saved"][c["M"]:].cpu(), c["v"])
    assert _same([o], _forward([name], False))


@pytest.mark.parametrize("name", NAMES)
def test_backward_against_float64(name):
    c = _case(name)
    fwd = _forward([name], True)
    (dw,) = _backward([name], fwd)
    # against the restatement at the kernels' own (u', v', sigma): the backward kernels alone ...
    o = fwd[0]
    ref_own = R.sn_ref_backward(c["g"], c["w"], o["u"].cpu(), o["v"].cpu(), o["sigma"].cpu().double()[0], c["dim"])
    _check(f"{name} dW_orig (own u, v, sigma)", dw, ref_own)
    # ... and end to end against float64 throughout
    _, ru, rv, rs = c["steps"][0]
    _check(f"{name} dW_orig", dw, R.sn_ref_backward(c["g"], c["w"], ru, rv, rs, c["dim"]))
    (dw2,) = _backward([name], fwd)
    assert torch.equal(dw, dw2)


def test_one_table_equals_single_jobs_bitwise():
    for training in (True, False):
        table = _forward(NAMES, training)
        single = [_forward([n], training)[0] for n in NAMES]
        assert _same(table, single), training
        if training:
            dws = _backward(NAMES, table)
            for n, s, dw in zip(NAMES, single, dws):
                assert torch.equal(dw, _backward([n], [s])[0]), n


@pytest.mark.parametrize("name", NAMES)
def test_three_refreshes_track_the_restatement(name):
    c = _case(name)
    state = None
    for k in range(3):
        state = _forward([name], True, state, save=False)
        rw, ru, rv, rs = c["steps"][k]
        for what, out, ref in (("w", state[0]["w"], rw), ("u", state[0]["u"], ru), ("v", state[0]["v"], rv),
                               ("sigma", state[0]["sigma"], rs.reshape(1))):
            _check(f"{name} step {k + 1} {what}", out, ref)


def test_autograd_function_against_float64():
    """SpectralNormWeight over two layers: the gradients reach weight_orig; a second forward before the
    backward (the critic is called on real and fake images) does not disturb the first one's"""
    from fastfourierconvolution_amd._autograd import SpectralNormWeight
    names = ["conv4x4_130x1040", "convT_20x192"]
    cs = [_case(n) for n in names]
    ws = [c["w"].to(DEV).requires_grad_() for c in cs]
    layers = [(c["u"].to(DEV), c["v"].to(DEV), c["dim"]) for c in cs]
    out1 = SpectralNormWeight.apply(layers, True, *ws)
    out2 = SpectralNormWeight.apply(layers, True, *ws)   # advances u, v in place
    for c, o1, o2 in zip(cs, out1, out2):
        _check("first call w", o1, c["steps"][0][0])
        _check("second call w", o2, c["steps"][1][0])
    g1 = torch.autograd.grad(sum((o * c["g"].to(DEV)).sum() for o, c in zip(out1, cs)), ws)
    g2 = torch.autograd.grad(sum((o * c["g"].to(DEV)).sum() for o, c in zip(out2, cs)), ws)
    for c, a, b in zip(cs, g1, g2):
        _check("first call dW_orig", a, R.sn_ref_backward(c["g"], c["w"], *c["steps"][0][1:], c["dim"]))
        _check("second call dW_orig", b, R.sn_ref_backward(c["g"], c["w"], *c["steps"][1][1:], c["dim"]))


# --------------------------------------------------------------------------- modules and models
def _sn_modules(model):
    return [(n, m) for n, m in model.named_modules() if hasattr(m, "weight_u")]


def _randomize(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.02 if p.dim() > 1 else 0.1))
    return model


def _buffers_close(on, off, tol=TOL_M):
    pairs = list(zip(_sn_modules(on), _sn_modules(off)))
    assert pairs
    for (n, a), (_, b) in pairs:
        _check(f"{n}.weight_u", a.weight_u, b.weight_u.cpu().double(), tol)
        _check(f"{n}.weight_v", a.weight_v, b.weight_v.cpu().double(), tol)
    return len(pairs)


def test_switch_off_is_the_hook_bitwise():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _runtime as rt
    for make in (lambda: torch.nn.Conv2d(5, 7, 3), lambda: torch.nn.ConvTranspose2d(6, 10, 4),
                 lambda: torch.nn.Linear(33, 9)):
        torch.manual_seed(5)
        mod = torch.nn.utils.spectral_norm(make()).to(DEV).train()
        F.set_sn_hip(F.set_sn_hip(mod), False)
        ref = copy.deepcopy(mod)
        with torch.no_grad():
            rt.sn_refresh(mod)
            w, u, v = R.run_hook(ref)
        assert torch.equal(mod.weight, w) and torch.equal(mod.weight_u, u) and torch.equal(mod.weight_v, v)


def test_sn_refresh_per_layer_route():
    """sn_refresh / sn_refresh_train with a table of one, train and eval, against the hook on a copy"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _runtime as rt
    for make in (lambda: torch.nn.Conv2d(5, 7, 3), lambda: torch.nn.ConvTranspose2d(6, 10, 4)):
        for training in (True, False):
            torch.manual_seed(6)
            mod = torch.nn.utils.spectral_norm(make()).to(DEV).train(training)
            ref = copy.deepcopy(mod)
            F.set_sn_hip(mod)
            w, u, v = R.run_hook(ref)
            rt.sn_refresh_train(mod)
            _check(f"train={training} w", mod.weight, w.detach().cpu().double(), TOL_M)
            g = torch.randn_like(w)
            (ga,) = torch.autograd.grad((mod.weight * g).sum(), mod.weight_orig)
            (gb,) = torch.autograd.grad((w * g).sum(), ref.weight_orig)
            _check(f"train={training} dW_orig", ga, gb.cpu().double(), TOL_M)
            with torch.no_grad():
                rt.sn_refresh(mod)
                w, u, v = R.run_hook(ref)
            _check(f"train={training} second w", mod.weight, w.cpu().double(), TOL_M)
            _check(f"train={training} u", mod.weight_u, u.cpu().double(), TOL_M)
            _check(f"train={training} v", mod.weight_v, v.cpu().double(), TOL_M)
            ver = mod.weight._version
            keep = mod.weight
            with torch.no_grad():
                rt.sn_refresh(mod)
            assert mod.weight is keep and keep._version > ver   # persistent tensor, its version moves


def test_discriminator32_on_against_off():
    import fastfourierconvolution_amd as F
    off = _randomize(F.Discriminator32(sn=True, mg=4), 1).to(DEV).train()
    on = F.set_sn_hip(copy.deepcopy(off))
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(4, 3, 32, 32, generator=gen).to(DEV)
    g = torch.randn(4, 1, generator=gen).to(DEV)
    outs = []
    for model in (on, off):
        out = model(x)
        (out * g).sum().backward()
        outs.append(out)
    torch.cuda.synchronize()
    _check("output", outs[0], outs[1].detach().cpu().double(), TOL_M)
    pa, pb = dict(on.named_parameters()), dict(off.named_parameters())
    assert set(pa) == set(pb) and len(pa) == 16
    for n in sorted(pa):
        assert pa[n].grad is not None and pb[n].grad is not None, n
        _check(f"{n}.grad", pa[n].grad, pb[n].grad.cpu().double(), TOL_M)
    assert _buffers_close(on, off) == 8


def test_discriminator32_one_table_per_forward():
    """with the switch on the whole critic's spectral norm is three forward launches and two backward
    ones: one ffc::sn_weight and one ffc::sn_weight_bwd call"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _autograd as ag
    on = F.set_sn_hip(_randomize(F.Discriminator32(sn=True, mg=4), 1).to(DEV).train())
    x = torch.randn(4, 3, 32, 32, device=DEV)
    calls = []
    fwd, bwd = ag.sn_weight_impl, ag.sn_weight_bwd_impl
    ag.sn_weight_impl = lambda *a: (calls.append(("fwd", len(a[0]))), fwd(*a))[1]
    ag.sn_weight_bwd_impl = lambda *a: (calls.append(("bwd", len(a[0]))), bwd(*a))[1]
    try:
        on(x).sum().backward()
    finally:
        ag.sn_weight_impl, ag.sn_weight_bwd_impl = fwd, bwd
    print(f"  calls: {calls}")
    assert calls == [("fwd", 8), ("bwd", 8)]


def test_snffc_layer_on_against_off():
    import fastfourierconvolution_amd as F
    off = _randomize(F.SNFFC(16, 16, 3, 0.5, 0.5, padding=1), 3).to(DEV).train()
    on = F.set_sn_hip(copy.deepcopy(off))
    gen = torch.Generator().manual_seed(4)
    xl = torch.randn(2, 8, 8, 8, generator=gen).to(DEV)
    xg = torch.randn(2, 8, 8, 8, generator=gen).to(DEV)
    with torch.no_grad():
        a, b = on((xl, xg)), off((xl, xg))
    for k, name in enumerate(("out_l", "out_g")):
        _check(name, a[k], b[k].cpu().double(), TOL_M)
    assert _buffers_close(on, off) >= 4


def test_cond_critic_slices_see_this_calls_weight():
    """CondDiscriminator32 feeds conv1 through _ConvSlice: the slices read the table's W, and every
    buffer advances by exactly one power iteration per forward"""
    import fastfourierconvolution_amd as F
    off = _randomize(F.CondDiscriminator32(sn=True, mg=4, num_classes=10), 5).to(DEV).train()
    on = F.set_sn_hip(copy.deepcopy(off))
    start = {n: (m.weight_orig.detach().cpu(), m.weight_u.cpu().clone(), m.weight_v.cpu().clone())
             for n, m in _sn_modules(off)}
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    labels = torch.tensor([1, 0, 9, 4], device=DEV)
    with torch.no_grad():
        a, b = on(x, labels), off(x, labels)
    _check("output", a, b.cpu().double(), TOL_M)
    assert _buffers_close(on, off) == 8
    for n, m in _sn_modules(on):
        w0, u0, v0 = start[n]
        _, u1, v1, _ = R.sn_ref(w0, u0, v0, 0, True)
        _, u2, v2, _ = R.sn_ref(w0, u1, v1, 0, True)
        _check(f"{n}.weight_v, one iteration", m.weight_v, v1)
        if v0.numel() > 1 and R.normwise(v2, v1) > 1e-3:   # a second iteration would show
            assert R.normwise(m.weight_v, v2) > 1e-3, n
        _check(f"{n}.weight, this call's W", m.weight, R.sn_ref(w0, u0, v0, 0, True)[0])


def test_captured_forward_replays_the_eager_sequence():
    import fastfourierconvolution_amd as F
    eager = _randomize(F.Discriminator32(sn=True, mg=4), 7).to(DEV).train()
    F.set_sn_hip(eager)
    captured = copy.deepcopy(eager)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(8)).to(DEV)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            captured(x)                      # warm-up: the first power iteration
        torch.cuda.current_stream().wait_stream(s)
        eager(x)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = captured(x)
        for k in range(2):
            graph.replay()
            torch.cuda.synchronize()
            ref = eager(x)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), k
            for (n, a), (_, b) in zip(_sn_modules(captured), _sn_modules(eager)):
                assert torch.equal(a.weight_u, b.weight_u) and torch.equal(a.weight_v, b.weight_v), (k, n)
