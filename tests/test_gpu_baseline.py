"""The baseline generators on the GPU -- Generator32, Generator64 and DCGenerator32 -- against the reference's
own fp64 outputs, running statistics and gradients (tests/golden/gen_golden_baseline.py), plus determinism, a
captured-graph replay of the eval forward, the memory the attention needs, and one training iteration.

Tolerance: normwise 1e-4, the project's parity bound (test_gpu_parity.py, test_gpu_fgan48.py).  Gradients
stored as norms only (``gnorm.<key>``: parameters of more than 40 000 elements) are compared as norms.  The
biases of the transposed convs in front of a train-mode BatchNorm and the attention's key bias (a shift of
every logit of a softmax row) have exact gradient 0 (not stored): their
residue is checked against TOL x the norm of the same layer's weight gradient, as test_gpu_fgan48.py does.

The uint8 image may differ from the reference's by one level in at most 0.1 % of the pixels, and only where
the reference's 255 * (x / 2 + 1 / 2) lies within 1e-3 of an integer (the FGenerator32 rule)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import baseline_refs as R
from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
TAGS = ["g32_mg1", "g32_mg2", "g64_mg1", "g64_mg2", "dc32"]
# class, mg, image side, critic mg (Discriminator32 takes 8 * mg pixels)
TRAIN = {"Generator32": (1, 8, 1), "Generator64": (1, 16, 2), "DCGenerator32": (4, 32, 4)}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _cases():
    with open(os.path.join(GOLDEN, "manifest_baseline.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _golden(name):
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
    z = torch.from_numpy(input_array(c["seed"], "z", c["inputs"]["z"])).to(DEV)
    return c, mod, z, data


@pytest.mark.parametrize("tag", TAGS + ["g32_mg3"])
def test_train_step_golden(tag):
    """float image, running statistics after one step, input and parameter gradients"""
    c, G, z, data = _golden(tag + "_train")
    z.requires_grad_(True)
    out = G(z)
    ref = torch.from_numpy(data["ref.out"])
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape)
    errs = {"out": normwise_err(out.detach().cpu(), ref)}
    sd = G.state_dict()
    n_stats = 0
    for k in data.files:
        if k.startswith("after."):
            name = k[len("after."):]
            if name.endswith("num_batches_tracked"):
                assert int(sd[name]) == int(data[k]) == 1, name
            else:
                errs[name] = normwise_err(sd[name].cpu(), torch.from_numpy(data[k]))
                n_stats += 1
    assert n_stats >= 6
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", list(out.shape))).to(DEV)
    (out * cot).sum().backward()
    errs["gin.z"] = normwise_err(z.grad.cpu(), torch.from_numpy(data["gin.z"]))
    params = dict(G.named_parameters())
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
    for name in set(params) - seen:   # exact gradient 0 (module docstring)
        assert name.endswith(".bias"), name
        errs["0:" + name] = float(params[name].grad.double().norm()) / \
            float(params[name[:-4] + "weight"].grad.double().norm())
    print({k: f"{v:.1e}" for k, v in errs.items()})
    head = "model.12.weight" if c["kind"] == "DCGenerator32" else "last.0.weight"
    assert "g:" + head in errs and ("g:attn.gamma" in errs or c["kind"] == "DCGenerator32")
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


@pytest.mark.parametrize("tag", TAGS)
def test_eval_golden(tag):
    c, G, z, data = _golden(tag + "_eval")
    with torch.no_grad():
        fl = G.forward_float(z)
        q = G(z)
    ref = torch.from_numpy(data["ref.out"])
    err = normwise_err(fl.cpu(), ref)
    print(f"{tag}_eval float image: {err:.2e}")
    assert err <= TOL
    assert q.dtype == torch.uint8 and tuple(q.shape) == tuple(ref.shape)
    d = (q.cpu().int() - torch.from_numpy(data["ref.out_u8"]).int()).abs()
    lv = 255.0 * (ref.double() * 0.5 + 0.5)
    near = (lv - lv.round()).abs() < 1e-3
    print(f"{tag}_eval uint8: max {int(d.max())} level, share {float((d > 0).float().mean()):.2e}")
    assert int(d.max()) <= 1 and float((d > 0).float().mean()) <= 1e-3
    assert bool(near[d > 0].all())
    for k, v in G.state_dict().items():   # eval mode leaves the running statistics alone
        if k.endswith(("running_mean", "running_var")):
            assert torch.equal(v.cpu(), torch.from_numpy(data["before." + k])), k


def _model(kind, mg, seed=0):
    import fastfourierconvolution_amd as F
    return R.normal_state(_quiet(getattr(F, kind), 16, mg), seed).to(DEV)


@pytest.mark.parametrize("kind", list(TRAIN))
def test_forward_and_backward_are_deterministic(kind):
    mg = TRAIN[kind][0]
    G = _model(kind, mg).train()
    z0 = torch.randn(3, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for _ in range(2):
        G.zero_grad()
        z = z0.clone().requires_grad_(True)
        out = G(z)
        out.square().sum().backward()
        runs.append([out.detach().clone(), z.grad.clone()] + [p.grad.clone() for p in G.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("kind", list(TRAIN))
def test_eval_forward_graph_replay_is_bitwise_eager(kind):
    """two replays on new z written into the captured input"""
    from fastfourierconvolution_amd.graphs import capture_step
    mg = TRAIN[kind][0]
    G = _model(kind, mg, seed=1).eval()
    gen = torch.Generator().manual_seed(5)
    zs = [torch.randn(4, 16, generator=gen).to(DEV) for _ in range(3)]
    z = zs[0].clone()
    with torch.no_grad():
        eager = [(G(v).clone(), G.forward_float(v).clone()) for v in zs]
        g = capture_step(lambda: (G(z), G.forward_float(z)))
        assert g is not None, "capture failed"
        for i in (1, 2):
            z.copy_(zs[i])
            g.replay()
            torch.cuda.synchronize()
            q, f = g.ffc_output
            assert q.dtype == torch.uint8 and torch.equal(q, eager[i][0]) and torch.equal(f, eager[i][1])
    assert not torch.equal(eager[1][1], eager[2][1])


@pytest.mark.parametrize("kind,mg", [("Generator32", 4), ("Generator64", 2)])
def test_attention_matrix_is_never_allocated(kind, mg):
    """B = 2 on a 32 x 32 attention plane (N = 1024): the forward's peak allocation above what is live before
    it stays under one (B, N, N) fp32 matrix (8 MiB), in eval and in train mode with gradients"""
    G = _model(kind, mg)
    z = torch.randn(2, 16, generator=torch.Generator().manual_seed(7)).to(DEV)
    matrix = 2 * 1024 * 1024 * 4
    for train in (False, True):
        G.train(train)
        with torch.set_grad_enabled(train):
            out = G.forward_float(z)          # plans, packs and the library's buffers exist after this call
            del out
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = G.forward_float(z)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        print(f"{kind} train={train}: peak {peak / 2 ** 20:.2f} MiB over the live set, matrix {matrix / 2 ** 20:.0f} MiB")
        assert tuple(out.shape) == (2, 3, 32, 32) and peak < matrix
        del out


@pytest.mark.parametrize("kind", list(TRAIN))
def test_train_iteration(kind):
    """generator_step + discriminator_step at B = 4 against Discriminator32 of the matching input size: finite
    losses, every parameter of G and D reached by a gradient and changed"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import training
    mg, side, dmg = TRAIN[kind]
    torch.manual_seed(0)
    G = _model(kind, mg).train()
    D = _quiet(F.Discriminator32, mg=dmg).to(DEV).train()
    oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
    oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
    gen = torch.Generator().manual_seed(mg)
    z_g, z_d = torch.randn(4, 16, generator=gen).to(DEV), torch.randn(4, 16, generator=gen).to(DEV)
    real = torch.tanh(torch.randn(4, 3, side, side, generator=gen)).to(DEV)
    before = {id(p): p.detach().clone() for m in (G, D) for p in m.parameters()}
    loss_G = training.generator_step(G, D, oG, oD, z_g)
    gG = {k: None if p.grad is None else bool((p.grad != 0).any()) for k, p in G.named_parameters()}
    loss_D = training.discriminator_step(G, D, oG, oD, z_d, real)
    gD = {k: None if p.grad is None else bool((p.grad != 0).any()) for k, p in D.named_parameters()}
    assert torch.isfinite(loss_G).item() and torch.isfinite(loss_D).item()
    assert not [k for k, v in {**gG, **gD}.items() if v is None]
    # exact-zero gradients: conv biases in front of a train-mode BatchNorm and the attention's key bias are not
    # counted (round-off residue moves them); the critic's fc.bias while every hinge term is active (test_gpu_fgan48.py)
    convs = {k for k, _ in G.named_parameters() if k.endswith(".bias") and k.replace(".bias", ".weight") in gG
             and G.get_parameter(k.replace(".bias", ".weight")).dim() == 4 and k not in ("last.0.bias", "model.12.bias")
             and not k.startswith("attn.")} | {"attn.key_conv.bias"}
    zero = [k for k, v in {**gG, **gD}.items() if v is False and k not in convs]
    assert all(k == "fc.bias" for k in zero), zero
    same = [k for m, gr in ((G, gG), (D, gD)) for k, p in m.named_parameters()
            if gr[k] and k not in convs and torch.equal(p.detach(), before[id(p)])]
    assert not same, same
    for m in (G, D):
        for k, v in m.state_dict().items():
            assert torch.isfinite(v.float()).all(), k
