"""The ResNet SNGAN family on the GPU -- GBlock, DBlock, SNGANGenerator128, SNGANDiscriminator128 -- against the
reference's own fp64 outputs, gradients, running statistics and power-iteration vectors
(tests/golden/gen_golden_resnet.py), with set_sn_hip off and on; plus determinism, the caller's tensor left
alone by DBlock, a captured-graph replay of the generator's eval forward, training steps and the refusals.

Tolerance: normwise 1e-4, the project's parity bound for a model forward (test_gpu_parity.py), taken for the
gradients as test_gpu_baseline.py takes it: parameters stored as norms (``gnorm.<key>``: more than 10 000
elements) are compared as norms; biases with exact gradient 0 (the manifest's ``dead`` list) are held to TOL x the
norm of the same layer's weight gradient."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
TAGS = ["sngan_g32", "sngan_g64", "sngan_d32", "sngan_d96", "gblock_cond", "dblock_same", "dblock_down"]


def _cases():
    with open(os.path.join(GOLDEN, "manifest_resnet.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _golden(name, sn_hip):
    import fastfourierconvolution_amd as F
    c = _cases()[name]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    state = make_state(c["seed"], c["specs"])
    mod = getattr(F, c["kind"])(**c["ctor"])
    mod.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)
    mod = mod.to(DEV).train(c["mode"] == "train")
    if sn_hip:
        F.set_sn_hip(mod)
    (iname, ishape), = c["inputs"].items()
    x = torch.from_numpy(input_array(c["seed"], iname, ishape)).to(DEV)
    args = [torch.tensor(c["labels"], dtype=torch.int64, device=DEV)] if "labels" in c else []
    return c, mod, iname, x, args, data


@pytest.mark.parametrize("sn_hip", [False, True], ids=["hook", "sn_hip"])
@pytest.mark.parametrize("tag", TAGS)
def test_train_step_golden(tag, sn_hip):
    """output, running statistics and weight_u / weight_v after one step, input and parameter gradients"""
    c, mod, iname, x, args, data = _golden(tag + "_train", sn_hip)
    x.requires_grad_(True)
    x_before = x.detach().clone()
    out = mod(x, *args)
    assert torch.equal(x.detach(), x_before), "the caller's tensor was written"
    ref = torch.from_numpy(data["ref.out"])
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape)
    errs = {"out": normwise_err(out.detach().cpu(), ref)}
    sd = mod.state_dict()
    n_u = 0
    for k in data.files:
        if k.startswith("after."):
            name = k[len("after."):]
            if name.endswith("num_batches_tracked"):
                assert int(sd[name]) == int(data[k]) == 1, name
            else:
                errs[name] = normwise_err(sd[name].cpu(), torch.from_numpy(data[k]))
                n_u += name.endswith("weight_u")
    assert n_u >= 2
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", list(out.shape))).to(DEV)
    (out * cot).sum().backward()
    errs["gin"] = normwise_err(x.grad.cpu(), torch.from_numpy(data["gin." + iname]))
    params = dict(mod.named_parameters())
    seen = set()
    for k in data.files:
        if k.startswith("gpar."):
            name = k[len("gpar."):]
            errs["g:" + name] = normwise_err(params[name].grad.cpu(), torch.from_numpy(data[k]))
            seen.add(name)
        elif k.startswith("gnorm."):
            name = k[len("gnorm."):]
            r = float(data[k])
            errs["|g:" + name + "|"] = abs(float(params[name].grad.double().norm()) - r) / r
            seen.add(name)
    assert set(params) - seen == set(c["dead"])
    for name in c["dead"]:   # exact gradient 0
        w = name[:-4] + ("weight_orig" if name[:-4] + "weight_orig" in params else "weight")
        errs["0:" + name] = float(params[name].grad.double().norm()) / float(params[w].grad.double().norm())
    print({k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


@pytest.mark.parametrize("sn_hip", [False, True], ids=["hook", "sn_hip"])
@pytest.mark.parametrize("tag", TAGS)
def test_eval_golden(tag, sn_hip):
    c, mod, iname, x, args, data = _golden(tag + "_eval", sn_hip)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    with torch.no_grad():
        out = mod(x, *args)
    err = normwise_err(out.cpu(), torch.from_numpy(data["ref.out"]))
    print(f"{tag}_eval: {err:.2e}")
    assert err <= TOL
    for k, v in mod.state_dict().items():   # eval mode moves no buffer: running statistics, u, v
        assert torch.equal(v, before[k]), k


def _pair(seed=0):
    import fastfourierconvolution_amd as F
    torch.manual_seed(seed)
    G = F.SNGANGenerator128(nz=16, ngf=64, bottom_width=1).to(DEV)
    D = F.SNGANDiscriminator128(ndf=64).to(DEV)
    return F.set_sn_hip(G), F.set_sn_hip(D)


def test_forward_and_backward_are_deterministic():
    G, D = _pair()
    G.train(), D.train()
    st = {k: v.clone() for m in (G, D) for k, v in m.state_dict(prefix=type(m).__name__).items()}
    z0 = torch.randn(4, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for _ in range(2):
        for m in (G, D):   # the same u / v and running statistics for both runs
            m.load_state_dict({k[len(type(m).__name__):]: v for k, v in st.items() if k.startswith(type(m).__name__)})
            m.zero_grad()
        z = z0.clone().requires_grad_(True)
        img = G(z)
        out = D(img)
        out.square().sum().backward()
        runs.append([img.detach().clone(), out.detach().clone(), z.grad.clone()]
                    + [p.grad.clone() for m in (G, D) for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_eval_forward_graph_replay_is_bitwise_eager():
    """the generator's eval forward with set_sn_hip captured into a hipGraph: two replays on new z"""
    from fastfourierconvolution_amd.graphs import capture_step
    G, _ = _pair(seed=1)
    G.eval()
    gen = torch.Generator().manual_seed(5)
    zs = [torch.randn(4, 16, generator=gen).to(DEV) for _ in range(3)]
    z = zs[0].clone()
    with torch.no_grad():
        eager = [G(v).clone() for v in zs]
        g = capture_step(lambda: G(z))
        assert g is not None, "capture failed"
        for i in (1, 2):
            z.copy_(zs[i])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(g.ffc_output, eager[i])
    assert tuple(eager[0].shape) == (4, 3, 32, 32) and not torch.equal(eager[1], eager[2])


def test_training_steps_reach_every_parameter():
    """generator_step + discriminator_step, then aw_discriminator_step, on the 32 x 32 pair at B = 4"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import training
    G, D = _pair(seed=2)
    G.train(), D.train()
    oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
    oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
    gen = torch.Generator().manual_seed(9)
    z_g, z_d = torch.randn(4, 16, generator=gen).to(DEV), torch.randn(4, 16, generator=gen).to(DEV)
    real = torch.tanh(torch.randn(4, 3, 32, 32, generator=gen)).to(DEV)
    assert tuple(G(z_g).shape) == (4, 3, 32, 32) and tuple(D(real).shape) == (4, 1)
    loss_G = training.generator_step(G, D, oG, oD, z_g)
    none_G = [k for k, p in G.named_parameters() if p.grad is None]
    loss_D = training.discriminator_step(G, D, oG, oD, z_d, real)
    none_D = [k for k, p in D.named_parameters() if p.grad is None]
    assert torch.isfinite(loss_G).item() and torch.isfinite(loss_D).item()
    assert not none_G and not none_D, (none_G, none_D)
    for p in D.parameters():
        p.grad = None
    loss_aw = training.aw_discriminator_step(G, D, oG, oD, z_d, real, F.aw_method())
    loss_aw = loss_aw[0] if isinstance(loss_aw, (tuple, list)) else loss_aw
    assert torch.isfinite(torch.as_tensor(loss_aw)).all().item()
    assert not [k for k, p in D.named_parameters() if p.grad is None]
    for m in (G, D):
        for k, v in m.state_dict().items():
            assert torch.isfinite(v.float()).all(), k


def test_refusals():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd._lib import FFCError
    D = F.SNGANDiscriminator128(ndf=32).to(DEV)
    with pytest.raises(NotImplementedError, match="odd"):
        D(torch.randn(1, 3, 36, 36, device=DEV))          # 36 -> 18 -> 9: block3 pools an odd plane
    c, D48, _, x, _, _ = _golden("sngan_d48_eval", False)   # 48 -> 24 -> 12 -> 6 -> 3: block5 (the reference floors)
    with pytest.raises(NotImplementedError, match="odd 3x3"), torch.no_grad():
        D48(x)
    with pytest.raises(NotImplementedError, match="odd"):
        F.DBlock(4, 8, downsample=True).to(DEV)(torch.randn(1, 4, 5, 6, device=DEV))
    with pytest.raises(NotImplementedError, match="odd"):
        torch.ops.ffc.pool2_act(torch.randn(1, 2, 3, 4, device=DEV), 1, 0.0)
    with pytest.raises(FFCError, match="fp32"):
        D(torch.randn(1, 3, 32, 32, device=DEV, dtype=torch.float16))
    with pytest.raises(FFCError, match="no CPU fallback"):
        F.GBlock(4, 4, upsample=True).to(DEV)(torch.randn(1, 4, 2, 2))
    with pytest.raises(TypeError):
        F.GBlock(4, 4, upsample=True, num_classes=3).to(DEV)(torch.randn(1, 4, 2, 2, device=DEV))


def test_ops_match_aten_with_autograd():
    """ffc::up2_bilinear / ffc::pool2_act / ffc::relu_sum_pool / ffc::act and their backwards against ATen in
    fp64 on an odd plane (the kernels themselves: test_gpu_resample_abi.py)"""
    import torch.nn.functional as Fn
    import fastfourierconvolution_amd  # noqa: F401
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 7, 9, generator=gen)
    for op, ref in ((lambda t: torch.ops.ffc.up2_bilinear(t, None, None, 0, 0.0),
                     lambda t: Fn.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)),
                    (lambda t: torch.ops.ffc.relu_sum_pool(t), lambda t: torch.relu(t).sum((2, 3))),
                    (lambda t: torch.ops.ffc.act(t, 1, 0.0), torch.relu),
                    (lambda t: torch.ops.ffc.pool2_act(torch.ops.ffc.up2_bilinear(t, None, None, 0, 0.0), 1, 0.0),
                     lambda t: torch.relu(Fn.avg_pool2d(Fn.interpolate(t, scale_factor=2, mode="bilinear",
                                                                          align_corners=False), 2)))):
        a = x.clone().to(DEV).requires_grad_(True)
        b = x.clone().double().requires_grad_(True)
        ya, yb = op(a), ref(b)
        cot = torch.randn(yb.shape, generator=gen)
        (ya * cot.to(DEV)).sum().backward()
        (yb * cot.double()).sum().backward()
        assert normwise_err(ya.detach().cpu(), yb.detach()) <= 1e-6
        assert normwise_err(a.grad.cpu(), b.grad) <= 1e-6
    sc, sh = torch.randn(5, generator=gen), torch.randn(5, generator=gen)
    y = torch.ops.ffc.up2_bilinear(x.to(DEV), sc.to(DEV), sh.to(DEV), 1, 0.0)
    r = Fn.interpolate(torch.relu(x.double() * sc.double().view(1, 5, 1, 1) + sh.double().view(1, 5, 1, 1)),
                       scale_factor=2, mode="bilinear", align_corners=False)
    assert normwise_err(y.cpu(), r) <= 1e-6
