"""The 8*mg family at mg = 6 (48x48 images) on the GPU: FourierUnitSN and the transposed FFC_BN_ACT at
24 -> 48 against the fp64 oracle, FGenerator32 / Discriminator32 / FDiscriminator32 against the
reference's own fp64 outputs and gradients (tests/golden/gen_golden_fgan48.py), one train iteration,
and a captured-graph replay of the eval forward.

Tolerance: normwise 1e-4, the project's parity bound (test_gpu_parity.py, test_gpu_train.py).  Conv
biases in front of a train-mode BatchNorm (FDiscriminator32 main.1..3) have exact gradient 0; as in
test_gpu_cond.py their residue is checked against TOL x the norm of the same layer's weight gradient.
Gradients stored as norms only (``gnorm.<key>``: parameters of more than 40 000 elements) are compared
as norms.

The uint8 image may differ from the reference's by one level in at most 0.1 % of the pixels, and only
where the reference's 255 * (x / 2 + 1 / 2) lies within 1e-3 of an integer."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import ffc_bn_act, fourier_unit, normwise_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _cases():
    with open(os.path.join(GOLDEN, "manifest_fgan48.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _golden(name):
    """-> (case, module on the GPU in the case's mode, inputs as GPU tensors, fixture arrays)"""
    import fastfourierconvolution_amd as F
    c = _cases()[name]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    state = make_state(c["seed"], c["specs"])
    for k in data.files:
        if k.startswith("before."):
            state[k[len("before."):]] = data[k]
    mod = _quiet(getattr(F, c["kind"]), **c["ctor"])
    mod.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    mod = mod.to(DEV).train(c["mode"] == "train")
    tin = {k: torch.from_numpy(input_array(c["seed"], k, shp)).to(DEV) for k, shp in c["inputs"].items()}
    return c, mod, tin, data


def _noises(tin):
    return [(tin[f"noise{n}_l"], tin[f"noise{n}_g"]) for n in (2, 3, 4)]


def _randomize(mod, gen):
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            if not v.is_floating_point():
                continue
            if k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=gen))
            elif v.dim() > 1:
                v.copy_(torch.randn(v.shape, generator=gen) / max(1, v[0].numel()) ** 0.5)
            else:
                v.copy_((1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=gen))
    return mod


def _sd64(mod):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in mod.state_dict().items()}


# --------------------------------------------------------------------------- layers against the oracle
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("C,H", [(16, 24), (8, 48), (5, 48)])
def test_fourier_unit_3x2k_vs_oracle(C, H, train):
    """FourierUnitSN on the x2 nearest-upsampled input, as SpectralTransform runs it at 12 -> 24 and 24 -> 48
    (FourierUnitSN._run, up = 2: the upsample happens inside the kernel); the oracle gets the upsampled tensor"""
    import fastfourierconvolution_amd as F
    gen = torch.Generator().manual_seed(C * H)
    fu = _randomize(F.FourierUnitSN(C, C), gen).train(train)
    sd = _sd64(fu)
    t = torch.randn(3, C, H // 2, H // 2, generator=gen)
    fu = fu.to(DEV)
    with torch.no_grad():
        out = fu._run(t.to(DEV), up=2)
        x = t.double().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        ref = fourier_unit(x, sd, "", train)
    err = normwise_err(out.cpu(), ref)
    print(f"FourierUnitSN ({C}, {H}, {H}) up=2 train={train}: {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("C", [8, 5])
def test_fourier_unit_direct_24_vs_oracle(C, train):
    """FourierUnitSN.forward on a (B, C, 24, 24) input (up = 1)"""
    import fastfourierconvolution_amd as F
    gen = torch.Generator().manual_seed(24 + C)
    fu = _randomize(F.FourierUnitSN(C, C), gen).train(train)
    sd = _sd64(fu)
    x = torch.randn(3, C, 24, 24, generator=gen)
    fu = fu.to(DEV)
    with torch.no_grad():
        out = fu(x.to(DEV))
        ref = fourier_unit(x.double(), sd, "", train)
    err = normwise_err(out.cpu(), ref)
    print(f"FourierUnitSN ({C}, 24, 24) direct train={train}: {err:.2e}")
    assert err <= TOL


def test_direct_3x2k_input_raises():
    """up = 1 on a 48 plane and any 12 x 12 plane have no kernel: NotImplementedError, not a library error"""
    import fastfourierconvolution_amd as F
    fu = F.FourierUnitSN(8, 8).to(DEV)
    with torch.no_grad():
        for H, up in ((48, 1), (12, 1), (12, 2)):
            with pytest.raises(NotImplementedError):
                fu._run(torch.randn(2, 8, H // up, H // up, device=DEV), up=up)


@pytest.mark.parametrize("train", [True, False])
def test_transposed_ffc_bn_act_24_to_48_vs_oracle(train):
    """the generator's conv4: SpectralTransform stride 2 + upsample, its Fourier unit on (8, 48, 48) up 2"""
    import fastfourierconvolution_amd as F
    gen = torch.Generator().manual_seed(48)
    cfg = dict(in_channels=128, out_channels=64, kernel_size=4, ratio_gin=0.25, ratio_gout=0.25, stride=2, padding=1,
               norm_layer="BatchNorm2d", activation_layer="GELU", upsampling=True)
    blk = _quiet(F.FFC_BN_ACT, 128, 64, 4, 0.25, 0.25, stride=2, padding=1, activation_layer=nn.GELU,
                 norm_layer=nn.BatchNorm2d, upsampling=True)
    blk = _randomize(blk, gen).train(train)
    sd = _sd64(blk)
    xl, xg = torch.randn(2, 96, 24, 24, generator=gen), torch.randn(2, 32, 24, 24, generator=gen)
    blk = blk.to(DEV)
    with torch.no_grad():
        ol, og = blk((xl.to(DEV), xg.to(DEV)))
        rl, rg = ffc_bn_act((xl.double(), xg.double()), sd, "", cfg, train)
    assert tuple(ol.shape) == (2, 48, 48, 48) and tuple(og.shape) == (2, 16, 48, 48)
    el, eg = normwise_err(ol.cpu(), rl), normwise_err(og.cpu(), rg)
    print(f"FFC_BN_ACT 24->48 train={train}: local {el:.2e} global {eg:.2e}")
    assert el <= TOL and eg <= TOL


# --------------------------------------------------------------------------- goldens
def test_fgan48_generator_train_golden():
    c, G, tin, data = _golden("fgan48_gen_train")
    with torch.no_grad():
        out = G(tin["z"], _noises(tin))
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 48, 48)
    err = normwise_err(out.cpu(), torch.from_numpy(data["ref.out"]))
    print(f"fgan48_gen_train: {err:.2e}")
    assert err <= TOL
    sd = G.state_dict()
    for k in data.files:
        if k.startswith("after.") and k.endswith(("running_mean", "running_var")):
            assert normwise_err(sd[k[len("after."):]].cpu(), torch.from_numpy(data[k])) <= TOL, k


def test_fgan48_generator_eval_golden():
    c, G, tin, data = _golden("fgan48_gen_eval")
    with torch.no_grad():
        fl = G.forward_float(tin["z"])
        q = G(tin["z"])
    ref = torch.from_numpy(data["ref.out"])
    err = normwise_err(fl.cpu(), ref)
    print(f"fgan48_gen_eval float image: {err:.2e}")
    assert err <= TOL
    assert q.dtype == torch.uint8 and tuple(q.shape) == (2, 3, 48, 48)
    d = (q.cpu().int() - torch.from_numpy(data["ref.out_u8"]).int()).abs()
    lv = 255.0 * (ref.double() * 0.5 + 0.5)
    near = (lv - lv.round()).abs() < 1e-3
    print(f"fgan48_gen_eval uint8: max {int(d.max())} level, share {float((d > 0).float().mean()):.2e}, "
          f"{int(near.sum())} reference pixels within 1e-3 of an edge")
    assert int(d.max()) <= 1 and float((d > 0).float().mean()) <= 1e-3
    assert bool(near[d > 0].all())


@pytest.mark.parametrize("name", ["fgan48_disc", "fgan48_fdisc"])
def test_fgan48_critic_golden(name):
    c, D, tin, data = _golden(name)
    with torch.no_grad():
        out = D(tin["x"])
    assert tuple(out.shape) == (2, 1)
    err = normwise_err(out.cpu(), torch.from_numpy(data["ref.out"]))
    print(f"{name}: {err:.2e}")
    assert err <= TOL
    sd = D.state_dict()
    for k in data.files:
        if k.startswith("after.") and k.endswith(("running_mean", "running_var", "weight_u", "weight_v")):
            assert normwise_err(sd[k[len("after."):]].cpu(), torch.from_numpy(data[k])) <= TOL, k


def _check_grads(mod, data, first, first_key, zero_bias=()):
    errs = {first_key: normwise_err(first.grad.cpu(), torch.from_numpy(data["gin." + first_key]))}
    params = dict(mod.named_parameters())
    for k in data.files:
        if k.startswith("gpar."):
            name = k[len("gpar."):]
            got, ref = params[name].grad.cpu(), torch.from_numpy(data[k])
            if name in zero_bias:   # exact gradient 0: see the module docstring
                errs[name] = float(got.double().norm()) / float(params[name.replace("bias", "weight")].grad.norm())
            else:
                errs[name] = normwise_err(got, ref)
        elif k.startswith("gnorm."):
            name = k[len("gnorm."):]
            ref = float(data[k])
            errs["|" + name + "|"] = abs(float(params[name].grad.double().norm()) - ref) / ref
    print({k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    return errs


def test_fgan48_generator_grad_golden():
    c, G, tin, data = _golden("grad_fgan48_gen")
    z = tin["z"].requires_grad_(True)
    out = G.forward_float(z, _noises(tin))
    assert normwise_err(out.detach().cpu(), torch.from_numpy(data["ref.out"])) <= TOL
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", list(out.shape))).to(DEV)
    (out * cot).sum().backward()
    errs = _check_grads(G, data, z, "z")
    assert {"conv4.ffc.convg2g.fu.conv_layer.weight", "conv3.ffc.convg2g.fu.bn.weight", "glb_noise4.weight",
            "|noise_to_feature.0.weight|"} <= set(errs)


def test_fgan48_fdiscriminator_grad_golden():
    c, D, tin, data = _golden("grad_fgan48_fdisc")
    x = tin["x"].requires_grad_(True)
    out = D(x)
    assert normwise_err(out.detach().cpu(), torch.from_numpy(data["ref.out"])) <= TOL
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", list(out.shape))).to(DEV)
    (out * cot).sum().backward()
    errs = _check_grads(D, data, x, "x", zero_bias=tuple(f"main.{i}.ffc.convl2l.bias" for i in (1, 2, 3)))
    assert {"main.0.ffc.convl2l.weight", "main.3.bn_l.weight", "fc.weight_orig"} <= \
        {k.strip("|") for k in errs}


# --------------------------------------------------------------------------- GaussianNoise
def test_gaussian_noise_train_and_eval():
    """train mode adds N(0, stddev) of x's shape (layers/gaussian_noise.py:11-14): over n = 13 824 elements the
    sample mean lies within 5 stddev / sqrt(n) of 0 and the sample std within 5 / sqrt(2 n) (3 %) of stddev;
    two calls draw different noise; a strided x gives the same statistics; eval mode returns x itself"""
    import fastfourierconvolution_amd as F
    torch.manual_seed(11)
    gn = F.GaussianNoise(0.05).train()
    x = torch.randn(2, 3, 48, 48, device=DEV)
    n = x.numel()
    outs = [gn(x), gn(x), gn(x.transpose(2, 3))]
    refs = [x, x, x.transpose(2, 3)]
    for y, r in zip(outs, refs):
        d = (y - r).double()
        assert y.shape == r.shape and torch.isfinite(y).all()
        assert abs(float(d.mean())) <= 5 * 0.05 / n ** 0.5, float(d.mean())
        assert abs(float(d.std()) / 0.05 - 1) <= 5 / (2 * n) ** 0.5, float(d.std())
    assert not torch.equal(outs[0], outs[1])
    assert gn.eval()(x) is x
    with pytest.raises(NotImplementedError):   # the op's planes are H * W % 4 == 0
        gn.train()(torch.randn(1, 2, 3, 3, device=DEV))


# --------------------------------------------------------------------------- training, capture
def _pair(mg, critic, seed=0):
    import fastfourierconvolution_amd as F
    torch.manual_seed(seed)
    G = _quiet(F.FGenerator32, 16, mg=mg)
    D = _quiet(getattr(F, critic), mg=mg)
    with torch.no_grad():
        for k, p in G.named_parameters():
            if k.startswith(("lcl_noise", "glb_noise")):
                p.normal_(0.0, 0.2)
    return G.to(DEV), D.to(DEV)


@pytest.mark.parametrize("mg,critic", [(6, "FDiscriminator32"), (6, "Discriminator32"), (4, "FDiscriminator32")])
def test_train_iteration(mg, critic):
    """generator_step + discriminator_step at B = 4: finite losses, every live parameter of G and D changed"""
    from fastfourierconvolution_amd import training
    G, D = _pair(mg, critic)
    G.train()
    D.train()
    oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
    oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
    gen = torch.Generator().manual_seed(mg)
    z_g, z_d = torch.randn(4, 16, generator=gen).to(DEV), torch.randn(4, 16, generator=gen).to(DEV)
    real = torch.tanh(torch.randn(4, 3, 8 * mg, 8 * mg, generator=gen)).to(DEV)
    before = {id(p): p.detach().clone() for m in (G, D) for p in m.parameters()}
    grads = {}   # id(parameter) -> None (no gradient reached it) / whether its gradient had a nonzero element

    def record(opt):
        inner = opt.step

        def step(*a, **k):
            for grp in opt.param_groups:
                for p in grp["params"]:
                    grads[id(p)] = None if p.grad is None else bool((p.grad != 0).any())
            return inner(*a, **k)
        opt.step = step
    record(oG)
    record(oD)
    loss_G, loss_D = training.train_iteration(G, D, oG, oD, z_g, z_d, real)
    assert torch.isfinite(loss_G).item() and torch.isfinite(loss_D).item()
    # not counted: the SpectralTransform's lfu parameters, dead in the reference too
    # (spectral_transform.py:66-87), and FDiscriminator32's conv biases in front of a train-mode BatchNorm,
    # whose exact gradient is 0
    dead = lambda k: ".lfu." in k or (k.startswith(("main.1.", "main.2.", "main.3.")) and k.endswith("convl2l.bias"))  # noqa: E731
    named = [(k, p) for m in (G, D) for k, p in m.named_parameters() if not dead(k)]
    unreached = [k for k, p in named if grads.get(id(p)) is None]
    assert not unreached, unreached
    # an SE gate's hidden layer is 2 or 4 ReLU units on per-sample channel means that hardly differ between
    # samples: under the default init all of them can be off for the whole batch, and the gate's two
    # weights then have an exactly zero gradient.  The critic's fc.bias: d loss_D / d bias is
    # mean[fake > -1] - mean[real < 1], exactly 0 while every hinge term is active (an untrained critic).
    # Nothing else may
    zero = [k for k, p in named if grads[id(p)] is False]
    assert all(".se_block." in k or k == "fc.bias" for k in zero), zero
    same = [k for k, p in named if grads[id(p)] and torch.equal(p.detach(), before[id(p)])]
    assert not same, same
    for m in (G, D):
        for k, v in m.state_dict().items():
            assert torch.isfinite(v.float()).all(), k


def test_eval_forward_graph_replay_is_bitwise_eager():
    from fastfourierconvolution_amd.graphs import capture_step
    G, _ = _pair(6, "Discriminator32", seed=1)
    G.eval()
    z = torch.randn(8, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        eager = G(z).clone()
        fl = G.forward_float(z).clone()

        def step():
            return G(z), G.forward_float(z)
        g = capture_step(step)
        assert g is not None, "capture failed"
        g.replay()
        torch.cuda.synchronize()
    q, f = g.ffc_output
    assert eager.dtype == torch.uint8 and torch.equal(q, eager) and torch.equal(f, fl)
