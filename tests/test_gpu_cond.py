"""Class-conditional fgan128 on the GPU (fgan128_cond_complete.py:33-180): the fused generator stem
against a float64 torch restatement, FCondGenerator / FCondDiscriminator against the reference's own
fp64 outputs and gradients (tests/golden/gen_golden_cond.py), bitwise-reproducible label_embed
gradients, hipGraph replay with labels rewritten in place, a B = 4 conditional train step against a
float64 composition of the oracle's blocks, and opcheck of the two new ops.

Tolerance: normwise 1e-4, the bound of the fgan128 golden and gradient tests (test_gpu_parity.py,
test_gpu_fgan_train.py).

Conv biases in front of a train-mode BatchNorm (input_conv.0.bias, label_conv.0.bias): BatchNorm
subtracts the batch mean, so their exact gradient is 0 and the fp64 reference holds rounding residue
(~1e-17); a ratio to that is meaningless.  Such a gradient is the sum of the pre-BN gradient over
samples and positions, the weight gradient of the same layer is the same sum weighted by O(1)
inputs, so the residue is checked against TOL x the norm of the layer's weight gradient."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as tF

from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
SIDES = (8, 16, 32, 64, 128)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _cases():
    with open(os.path.join(GOLDEN, "manifest_cond.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _golden(name):
    """-> (case, module on the GPU in the case's mode, inputs as GPU tensors, labels, fixture arrays)"""
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
    labels = torch.tensor(c["labels"], dtype=torch.int64, device=DEV)
    return c, mod, tin, labels, data


def _noises(tin):
    return [(tin[f"noise{n}_l"], tin[f"noise{n}_g"]) for n in (2, 3, 4, 5, 6)]


def _check_grads(mod, data, first, first_key):
    errs = {first_key: normwise_err(first.grad.cpu(), torch.from_numpy(data["gin." + first_key]))}
    params = dict(mod.named_parameters())
    for k in data.files:
        if not k.startswith("gpar."):
            continue
        name = k[len("gpar."):]
        got, ref = params[name].grad.cpu(), torch.from_numpy(data[k])
        if name in ("input_conv.0.bias", "label_conv.0.bias"):   # exact gradient 0: see the module docstring
            scale = float(params[name.replace("bias", "weight")].grad.norm())
            errs[name] = float(got.double().norm()) / scale
        else:
            errs[name] = normwise_err(got, ref)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    return errs


# --------------------------------------------------------------------------- the stem
class _Stem(nn.Module):
    """the stem's modules alone, under the reference's names (fgan128_cond_complete.py:74-87)"""

    def __init__(self, z_size, num_classes):
        super().__init__()
        self.label_conv = nn.Sequential(nn.ConvTranspose2d(num_classes, 256, 4, 1, 0), nn.BatchNorm2d(256), nn.GELU())
        self.input_conv = nn.Sequential(nn.ConvTranspose2d(z_size, 256, 4, 1, 0), nn.BatchNorm2d(256), nn.GELU())
        self.label_embed = nn.Embedding(num_classes, num_classes)

    def forward(self, z, labels):   # :91-101 restated on torch modules (the float64 reference of the test)
        e = self.label_embed(labels).view(labels.shape[0], -1, 1, 1)
        return torch.cat([self.input_conv(z.reshape(z.size(0), -1, 1, 1)), self.label_conv(e)], dim=1)


def _label_patterns(B, nc, gen):
    """all samples of one class; and (when there is more than one class) a batch that leaves classes out"""
    pats = [torch.full((B,), nc - 1, dtype=torch.int64)]
    if nc > 1:
        pats.append(torch.randint(0, nc - 1, (B,), generator=gen))   # the last class is always absent
    return pats


@pytest.mark.parametrize("nc", [1, 3, 10])
@pytest.mark.parametrize("z_size", [8, 100])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_stem_vs_float64_torch(B, z_size, nc):
    """ffc::cond_stem forward, running statistics after one step and every gradient against
    Embedding -> ConvTranspose2d -> BatchNorm2d -> GELU -> cat in float64, train and eval"""
    from fastfourierconvolution_amd import _autograd as ag
    gen = torch.Generator().manual_seed(100 * B + z_size + nc)
    ref = _Stem(z_size, nc)
    with torch.no_grad():
        for bn in (ref.label_conv[1], ref.input_conv[1]):
            bn.weight.copy_(1 + 0.1 * torch.randn(256, generator=gen))
            bn.bias.copy_(0.1 * torch.randn(256, generator=gen))
            bn.running_mean.copy_(0.1 * torch.randn(256, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(256, generator=gen))
    for train in (True, False):
        for labels in _label_patterns(B, nc, gen):
            mine = _Stem(z_size, nc)
            mine.load_state_dict(ref.state_dict())
            mine = mine.to(DEV).train(train)
            gold = _Stem(z_size, nc)
            gold.load_state_dict(ref.state_dict())
            gold = gold.double().train(train)
            z = torch.randn(B, z_size, generator=gen)
            cot = torch.randn(B, 512, 4, 4, generator=gen)
            zg, zr = z.to(DEV).requires_grad_(True), z.double().requires_grad_(True)
            y = ag.cond_stem(mine, zg, labels.to(DEV))
            (y * cot.to(DEV)).sum().backward()
            yr = gold(zr, labels)
            (yr * cot.double()).sum().backward()
            what = (B, z_size, nc, train, labels.tolist())
            assert normwise_err(y.detach().cpu(), yr.detach()) <= TOL, what
            for (k, v), (_, r) in zip(mine.state_dict().items(), gold.state_dict().items()):
                if k.endswith(("running_mean", "running_var")):
                    assert normwise_err(v.cpu(), r) <= TOL, (what, k)
                elif k.endswith("num_batches_tracked"):
                    assert int(v) == int(r), (what, k)
            errs = {"z": normwise_err(zg.grad.cpu(), zr.grad)}
            pg = dict(gold.named_parameters())
            for k, p in mine.named_parameters():
                assert p.grad is not None, (what, k)
                if train and k.endswith("0.bias"):   # exact gradient 0: see the module docstring
                    errs[k] = float(p.grad.double().norm()) / float(pg[k.replace("bias", "weight")].grad.norm())
                else:
                    errs[k] = normwise_err(p.grad.cpu(), pg[k].grad)
            bad = {k: v for k, v in errs.items() if not v <= TOL}
            assert not bad, (what, bad)
            absent = [c for c in range(nc) if c not in labels.tolist()]
            assert all(bool((mine.label_embed.weight.grad[c] == 0).all()) for c in absent), what


# --------------------------------------------------------------------------- goldens
def test_cond_generator_train_golden():
    c, G, tin, labels, data = _golden("cond_gen_train")
    with torch.no_grad():
        out = G(tin["z"], labels, _noises(tin))
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 128, 128)
    err = normwise_err(out.cpu(), torch.from_numpy(data["ref.out"]))
    print(f"cond_gen_train: {err:.2e}")
    assert err <= TOL
    sd = G.state_dict()
    for k in data.files:
        if k.startswith("after.") and k.endswith(("running_mean", "running_var")):
            assert normwise_err(sd[k[len("after."):]].cpu(), torch.from_numpy(data[k])) <= TOL, k


def test_cond_generator_eval_golden():
    c, G, tin, labels, data = _golden("cond_gen_eval")
    with torch.no_grad():
        fl = G.forward_float(tin["z"], labels)
        q = G(tin["z"], labels)
    err = normwise_err(fl.cpu(), torch.from_numpy(data["ref.out"]))
    print(f"cond_gen_eval float image: {err:.2e}")
    assert err <= TOL
    assert q.dtype == torch.uint8
    d = (q.cpu().int() - torch.from_numpy(data["ref.out_u8"]).int()).abs()
    print(f"cond_gen_eval uint8: max {int(d.max())} level, share {float((d > 0).float().mean()):.2e}")
    assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 1e-3   # the fgan128 eval test's allowance


def test_cond_discriminator_golden():
    c, D, tin, labels, data = _golden("cond_disc")
    with torch.no_grad():
        out = D(tin["x"], labels)
    err = normwise_err(out.cpu(), torch.from_numpy(data["ref.out"]))
    print(f"cond_disc: {err:.2e}")
    assert err <= TOL
    sd = D.state_dict()
    for k in ("conv1.weight_u", "conv1.weight_v", "fc.weight_u"):
        assert normwise_err(sd[k].cpu(), torch.from_numpy(data["after." + k])) <= TOL, k


def test_cond_generator_grad_golden():
    c, G, tin, labels, data = _golden("grad_cond_gen")
    z = tin["z"].requires_grad_(True)
    out = G.forward_float(z, labels, _noises(tin))
    assert normwise_err(out.detach().cpu(), torch.from_numpy(data["ref.out"])) <= TOL
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", list(out.shape))).to(DEV)
    (out * cot).sum().backward()
    errs = _check_grads(G, data, z, "z")
    assert {"label_embed.weight", "label_conv.0.weight", "input_conv.0.weight", "input_conv.1.weight"} <= set(errs)
    assert bool((G.label_embed.weight.grad[1] == 0).all())   # class 1 is absent from the case


def test_cond_discriminator_grad_golden():
    c, D, tin, labels, data = _golden("grad_cond_disc")
    x = tin["x"].requires_grad_(True)
    out = D(x, labels)
    assert normwise_err(out.detach().cpu(), torch.from_numpy(data["ref.out"])) <= TOL
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", list(out.shape))).to(DEV)
    (out * cot).sum().backward()
    errs = _check_grads(D, data, x, "x")
    assert {"label_embed.weight", "conv1.weight_orig", "conv1.bias"} <= set(errs)
    g = D.label_embed.weight.grad
    assert bool((g[0] == 0).all()) and bool((g[2] == 0).all())   # classes 0 and 2 are absent


# --------------------------------------------------------------------------- determinism, capture
def _models(z_size=16, nc=3, seed=0):
    import fastfourierconvolution_amd as F
    torch.manual_seed(seed)
    G = _quiet(F.FCondGenerator, z_size, num_classes=nc)
    D = F.FCondDiscriminator(num_classes=nc)
    with torch.no_grad():
        for m in (G, D):
            for k, p in m.named_parameters():
                if k.startswith(("lcl_noise", "glb_noise")):
                    p.normal_(0.0, 0.2)
    return G.to(DEV), D.to(DEV)


def test_label_embed_grad_is_bitwise_reproducible():
    """10 fresh backward passes at B = 5 with repeated labels: bit-identical label_embed.weight.grad for
    G and D; the rows of the absent class are exactly 0"""
    G, D = _models(nc=4)
    G.train()
    D.eval()   # fixed spectral-norm u / v: the ten passes see the same weights
    gen = torch.Generator().manual_seed(3)
    B = 5
    z = torch.randn(B, 16, generator=gen).to(DEV)
    x = torch.randn(B, 3, 128, 128, generator=gen).to(DEV)
    labels = torch.tensor([1, 3, 1, 0, 1], dtype=torch.int64, device=DEV)   # class 2 absent
    noises = [tuple(torch.randn(B, 1, s, s, generator=gen).to(DEV) for _ in range(2)) for s in SIDES]
    cot = torch.randn(B, 3, 128, 128, generator=gen).to(DEV)
    got = {"G": [], "D": []}
    for _ in range(10):
        G.zero_grad(set_to_none=True)
        D.zero_grad(set_to_none=True)
        (G(z, labels, noises) * cot).sum().backward()
        D(x, labels).sum().backward()
        got["G"].append(G.label_embed.weight.grad.clone())
        got["D"].append(D.label_embed.weight.grad.clone())
    for k, gs in got.items():
        assert all(torch.equal(gs[0], g) for g in gs[1:]), k
        assert bool((gs[0][2] == 0).all()), k
        assert bool(torch.isfinite(gs[0]).all()) and float(gs[0].abs().sum()) > 0, k


def test_captured_forward_follows_labels_rewritten_in_place():
    from fastfourierconvolution_amd.graphs import capture_step
    G, _ = _models()
    G.eval()
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(4, 16, generator=gen).to(DEV)
    labels = torch.tensor([0, 1, 2, 0], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        g = capture_step(lambda: G.forward_float(z, labels), warmup=2)
        assert g is not None, "capture failed"
        g.replay()
        first = g.ffc_output.clone()
        labels.copy_(torch.tensor([2, 2, 0, 1], dtype=torch.int64, device=DEV))
        g.replay()
        second = g.ffc_output.clone()
        eager = G.forward_float(z, labels)
    assert torch.equal(second, eager)
    assert not torch.equal(second, first)


# --------------------------------------------------------------------------- a larger-batch train step
def _oracle_G(z, labels, sd, noises):
    """FCondGenerator.forward in train mode, float64: torch stem (:91-101) + the oracle's FFC_BN_ACT blocks"""
    from oracle.ffc_oracle import batch_norm, ffc_bn_act, fgan128_layers, noise_injection, resizer
    B = z.shape[0]
    e = tF.embedding(labels, sd["label_embed.weight"]).view(B, -1, 1, 1)
    br = []
    for name, x in (("input_conv", z.reshape(B, -1, 1, 1)), ("label_conv", e)):
        t = tF.conv_transpose2d(x, sd[name + ".0.weight"], sd[name + ".0.bias"])
        br.append(tF.gelu(batch_norm(t, sd, name + ".1.", True)))
    x = torch.cat(br, dim=1)
    for i, (name, cfg) in enumerate(fgan128_layers(64, 0.25)):
        x = ffc_bn_act(x, sd, name + ".", cfg, True, "torch")
        if name != "conv7":
            n = int(name[-1])
            x = (noise_injection(x[0], sd, f"lcl_noise{n}.", noises[i][0]),
                 noise_injection(x[1], sd, f"glb_noise{n}.", noises[i][1]))
    return resizer(x)


class _Kinks:
    """stand-in for torch.nn.functional inside the oracle (as test_gpu_train._KinkF): ReLU / LeakyReLU
    take their active set from the HIP path's own recorded outputs, in call order, so the oracle
    differentiates the same piece of the piecewise-linear network (one flipped LeakyReLU moves a
    gradient by far more than the kernels' error: test_gpu_train._layer_checks).  Recorded outputs of
    other shapes (the GELU BatchNorms, which have no kink) are skipped; a call nothing was recorded
    for (the SE layer's hidden ReLU) is torch's."""

    def __init__(self, outs):
        self.outs = [o.double() for o in outs]

    def __getattr__(self, name):
        return getattr(tF, name)

    def _take(self, x):
        for i, y in enumerate(self.outs):
            if tuple(y.shape) == tuple(x.shape):
                del self.outs[:i + 1]
                return y
        return None

    def relu(self, x):
        y = self._take(x)
        return tF.relu(x) if y is None else x * (y > 0).to(x.dtype)

    def leaky_relu(self, x, slope):
        y = self._take(x)
        if y is None:
            return tF.leaky_relu(x, slope)
        return x * torch.where(y > 0, torch.ones_like(x), torch.full_like(x, slope))


def _oracle_D(x, labels, sd):
    from oracle.ffc_oracle import fgan128_discriminator
    plane = tF.embedding(labels, sd["label_embed.weight"]).view(x.shape[0], 1, 128, 128)
    return fgan128_discriminator(torch.cat([x, plane], dim=1), sd, True)


def test_conditional_train_step_b4_vs_float64_composition():
    """generator_step + discriminator_step with labels (fgan128_cond_complete.py:296-324) at B = 4:
    losses and the gradients of the parameters the conditional models add vs float64 on the CPU --
    the oracle's FFC_BN_ACT blocks and critic plus torch stems, ReLU / LeakyReLU active sets from
    the HIP path (_Kinks), the critic step on the HIP path's own fake as test_gpu_fgan_d.py does"""
    import oracle.ffc_oracle as O
    from fastfourierconvolution_amd import _autograd as ag
    from fastfourierconvolution_amd.training import (discriminator_step, generator_step, hinge_loss_dis,
                                                     hinge_loss_gen)
    G, D = _models(seed=11)
    G.train()
    D.train()
    new_G = [k for k, _ in G.named_parameters() if k.startswith(("label_embed", "label_conv", "input_conv"))]
    new_D = ["label_embed.weight", "conv1.weight_orig", "conv1.bias"]

    def f64(m, grads):
        sd = {k: (v.detach().cpu().double().clone() if v.is_floating_point() else v.detach().cpu().clone())
              for k, v in m.state_dict().items()}
        for k in grads:
            sd[k].requires_grad_(True)
        return sd
    sdG, sdD = f64(G, new_G), f64(D, new_D)
    gen = torch.Generator().manual_seed(12)
    B = 4
    z_g, z_d = torch.randn(B, 16, generator=gen), torch.randn(B, 16, generator=gen)
    real = torch.rand(B, 3, 128, 128, generator=gen) * 2 - 1
    labels = torch.tensor([2, 0, 2, 2], dtype=torch.int64)   # class 1 absent
    noises = [tuple(torch.randn(B, 1, s, s, generator=gen) for _ in range(2)) for s in SIDES]
    nz_gpu = [tuple(t.to(DEV) for t in p) for p in noises]
    nz64 = [tuple(t.double() for t in p) for p in noises]
    optG, optD = torch.optim.SGD(G.parameters(), lr=0.0), torch.optim.SGD(D.parameters(), lr=0.0)
    lab = labels.to(DEV)
    ag.RECORD = []
    try:
        loss_G = generator_step(G, D, optG, optD, z_g.to(DEV), nz_gpu, labels=lab)
        rec_G = [t.cpu() for t in ag.RECORD if t.dim() == 4]
        gG = {k: dict(G.named_parameters())[k].grad.detach().cpu().clone() for k in new_G}
        with torch.no_grad():
            fake_hip = G(z_d.to(DEV), lab, nz_gpu).cpu()   # train-mode BN: the step below forms the same fake
        ag.RECORD = []
        loss_D = discriminator_step(G, D, optG, optD, z_d.to(DEV), real.to(DEV), nz_gpu, labels=lab)
        rec_D = [t.cpu() for t in ag.RECORD[-18:]]
    finally:
        ag.RECORD = None
    gD = {k: dict(D.named_parameters())[k].grad.detach().cpu().clone() for k in new_D}
    # float64: the same two steps (D's spectral-norm u / v advance with every call, as on the GPU;
    # G's BN running statistics do not enter a train-mode forward)
    old = O.F
    try:
        O.F = _Kinks(rec_G)
        out_G = _oracle_D(_oracle_G(z_g.double(), labels, sdG, nz64), labels, sdD)
        with torch.no_grad():
            O.F = old
            fake_ref = _oracle_G(z_d.double(), labels, sdG, nz64)
        O.F = _Kinks(rec_D)
        out_dg, out_dr = _oracle_D(fake_hip.double(), labels, sdD), _oracle_D(real.double(), labels, sdD)
    finally:
        O.F = old
    ref_G = hinge_loss_gen(out_G)
    ref_G.backward()
    rG = {k: sdG[k].grad.clone() for k in new_G}
    for k in new_D:
        sdD[k].grad = None
    ref_D = hinge_loss_dis(out_dg, out_dr)
    ref_D.backward()
    errs = {"fake": normwise_err(fake_hip, fake_ref),
            "loss_G": abs(loss_G.item() - ref_G.item()) / abs(ref_G.item()),
            "loss_D": abs(loss_D.item() - ref_D.item()) / abs(ref_D.item())}
    for k in new_G:
        if k.endswith("0.bias"):   # exact gradient 0: see the module docstring
            errs["G." + k] = float(gG[k].double().norm()) / float(rG[k.replace("bias", "weight")].norm())
        else:
            errs["G." + k] = normwise_err(gG[k], rG[k])
    for k in new_D:
        errs["D." + k] = normwise_err(gD[k], sdD[k].grad)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert bool((gG["label_embed.weight"][1] == 0).all()) and bool((gD["label_embed.weight"][1] == 0).all())


# --------------------------------------------------------------------------- opcheck
def _opcheck(op, args):
    res = torch.library.opcheck(op, args, None, raise_exception=False)
    bad = {k: v for k, v in res.items() if v != "SUCCESS"}
    assert not bad, f"{op}: {bad}"


@pytest.mark.parametrize("use_batch", [True, False])
def test_opcheck_cond_stem(use_batch):
    torch.manual_seed(0)
    B, K, NC = 2, 8, 3
    r = lambda *s: torch.randn(*s, device=DEV, requires_grad=True)   # noqa: E731
    labels = torch.tensor([2, 0], dtype=torch.int64, device=DEV)
    bn = lambda: ((1 + 0.1 * torch.randn(256, device=DEV)).requires_grad_(),   # noqa: E731
                  (0.1 * torch.randn(256, device=DEV)).requires_grad_())
    (g_i, b_i), (g_l, b_l) = bn(), bn()
    rm = lambda: 0.1 * torch.randn(256, device=DEV)   # noqa: E731
    rv = lambda: 0.5 + torch.rand(256, device=DEV)   # noqa: E731
    _opcheck(torch.ops.ffc.cond_stem.default,
             (r(B, K), labels, r(NC, NC), r(K, 256, 4, 4), r(256), r(NC, 256, 4, 4), r(256), g_i, b_i, g_l, b_l,
              rm(), rv(), rm(), rv(), use_batch, 1e-5))


def test_opcheck_embed_rows():
    torch.manual_seed(0)
    w = torch.randn(3, 16, device=DEV, requires_grad=True)
    labels = torch.tensor([1, 1, 0], dtype=torch.int64, device=DEV)
    _opcheck(torch.ops.ffc.embed_rows.default, (w, labels))
    _opcheck(torch.ops.ffc.embed_rows_backward.default, (torch.randn(3, 16, device=DEV), labels, 3))
    _opcheck(torch.ops.ffc.cond_stem_backward.default,
             (torch.randn(2, 512, 4, 4, device=DEV), torch.randn(2, 8, device=DEV), labels[:2],
              torch.randn(3, 3, device=DEV), torch.randn(8, 256, 4, 4, device=DEV),
              torch.randn(3, 256, 4, 4, device=DEV), [True] * 6))
