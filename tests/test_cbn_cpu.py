"""Conditional batch norm on the CPU (no GPU): the float64 restatement of tests/cbn_refs.py against the
reference's own fp64 runs (fixtures of tests/golden/gen_golden_cbn.py, stored as float32: bound 1e-6
normwise, observed <= 6e-8), the two-pass backward algebra of csrc/cbn_kernels.hip against torch
autograd in float64 (bound 1e-12, observed <= 4e-15), FakeTensor tracing of the conditional layer and of
FCondGenerator32 (compute through ffc:: ops only), and the state_dict keys of the four models."""
import contextlib
import io
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.proxy_tensor import make_fx

import cbn_refs as R
import fastfourierconvolution_amd as F
import train_refs as tr
from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import normwise_err

with open(os.path.join(GOLDEN, "manifest_cbn.json")) as f:
    MANIFEST = json.load(f)
CASES = {c["name"]: c for c in MANIFEST["cases"]}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def ref_case(c):
    """the fp64 restatement on a fixture case -> (outputs, input grads, parameter grads, state after)"""
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_state(c["seed"], c["specs"]).items()}
    sd = {k: (v.double().requires_grad_(not k.endswith(("running_mean", "running_var")))
              if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    labels = torch.tensor(c["labels"], dtype=torch.int64)
    tin = {k: torch.from_numpy(input_array(c["seed"], k, s)).double().requires_grad_(True)
           for k, s in c["inputs"].items()}
    train = c["mode"] == "train"
    if c["kind"] == "ConditionalBatchNorm2d":
        outs = {"out": R.cond_bn(tin["x"], sd, "", labels, train)}
    else:
        x = tin["x"] if "x" in tin else (tin["x_l"], tin["x_g"])
        ol, og = R.ffc_bn_act_cond(x, sd, "", c["ctor"], labels, train)
        outs = {n: o for n, o in (("out_l", ol), ("out_g", og)) if isinstance(o, torch.Tensor)}
    loss = sum((o * torch.from_numpy(input_array(c["seed"] + 11, "cot:" + n, list(o.shape))).double()).sum()
               for n, o in outs.items())
    loss.backward()
    gpar = {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}
    return outs, {k: t.grad for k, t in tin.items()}, gpar, sd


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_fixtures(name):
    c = CASES[name]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    outs, gin, gpar, sd = ref_case(c)
    worst = 0.0
    for k in data.files:
        kind, key = k.split(".", 1)
        got = {"ref": outs, "gin": gin, "gpar": gpar, "after": sd}[kind][key]
        if key.endswith("num_batches_tracked"):
            assert int(got) == int(data[k])
            continue
        want = torch.from_numpy(data[k]).double()
        if kind == "gpar" and key.endswith(".bias") and c["mode"] == "train":
            # a conv bias in front of batch statistics: its gradient vanishes analytically (1e-17 here), so
            # the error is taken relative to the same conv's weight gradient
            e = (got - want).abs().max().item() / float(np.abs(data[k[:-len("bias")] + "weight"]).max())
        else:
            e = normwise_err(got, want)
        worst = max(worst, e)
        assert e <= 1e-6, (k, e)
    assert {k for k in data.files if k.startswith("gpar.")} == {"gpar." + k for k in gpar}
    print(f"{name}: worst normwise error against the reference {worst:.2e}")


@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 8, 1), (4, 4, 16)])
@pytest.mark.parametrize("train", [True, False])
def test_backward_formulas_match_autograd(shape, train):
    """sums / scatter / coefficients / dx of the issue's two-pass backward == float64 autograd"""
    worst = 0.0
    for act in tr.ACTS:
        inp = R.kernel_inputs(shape, 3, train)
        dx_ref, dtable_ref = R.kernel_autograd(inp, act, train)
        _, dtable, dx = R.kernel_formulas(inp, act, train)
        worst = max(worst, normwise_err(dx, dx_ref), normwise_err(dtable, dtable_ref))
    print(f"{shape} train={train}: worst {worst:.2e}")
    assert worst <= 1e-12


# --------------------------------------------------------------------------- tracing
ALLOWED = {"<built-in function getitem>", "aten.detach.default", "aten.empty.memory_format", "aten.new_empty.default",
           "aten.normal.default", "aten.normal_.default", "aten.view.default", "aten.squeeze.default",
           "aten._unsafe_view.default", "aten.reshape.default", "aten.alias.default", "aten.slice.Tensor"}


def _trace(mod, fn, shapes, nlabels, grad=False, train=True):
    with FakeTensorMode(allow_non_fake_inputs=True):
        mod = mod.to("cuda").train(train)
        ins = [torch.empty(s, device="cuda") for s in shapes]
        labels = torch.empty((nlabels,), device="cuda", dtype=torch.int64)
        ctx = contextlib.nullcontext() if grad else torch.no_grad()

        def f(*xs):
            with ctx:
                return fn(mod, *xs)
        g = make_fx(f, tracing_mode="real")(*ins, labels)
        outs = f(*ins, labels)
    cnt = Counter(str(n.target) for n in g.graph.nodes if n.op == "call_function")
    bad = {k: v for k, v in cnt.items() if not k.startswith("ffc.") and k not in ALLOWED}
    assert not bad, f"non-ffc compute on the hot path: {bad}"
    return cnt, outs


def test_ops_registered_with_fake():
    from torch._library.simple_registry import singleton
    for name in ("cbn_act", "cbn_act_backward"):
        op = getattr(torch.ops.ffc, name).default
        assert singleton.find(op.name()).fake_impl.kernel is not None, name


@pytest.mark.parametrize("grad", [False, True])
def test_conditional_layer_traces_to_ffc_ops(grad):
    blk = _quiet(F.FFC_BN_ACT, 32, 16, 4, 0.25, 0.25, 2, 1, activation_layer=nn.GELU,
                 norm_layer=F.ConditionalBatchNorm2d, upsampling=True, num_classes=4)
    F.set_cond_bn(blk)
    cnt, (ol, og) = _trace(blk, lambda m, a, b, y: m((a, b), y), [(4, 24, 8, 8), (4, 8, 8, 8)], 4, grad=grad)
    # running statistics: bn_l, bn_g, and on the training path the spectral branch's bn1 and fu.bn as ops
    assert cnt["ffc.cbn_act.default"] == 2 and cnt["ffc.bn_update_running.default"] == (4 if grad else 2)
    assert cnt["ffc.conv_layer.default" if grad else "ffc.ffc_bn_act.default"] >= 1
    assert tuple(ol.shape) == (4, 12, 16, 16) and tuple(og.shape) == (4, 4, 16, 16)


@pytest.mark.parametrize("train", [True, False])
def test_generator_traces_to_ffc_ops(train):
    g = _quiet(F.FCondGenerator32, 16, 4, 3)
    cnt, out = _trace(g, lambda m, z, y: m(z, y), [(4, 16)], 4, train=train)
    assert cnt["ffc.cond_stem.default"] == 1 and cnt["ffc.cbn_act.default"] == 6
    assert cnt["ffc.quantize_u8.default"] == (0 if train else 1)
    assert tuple(out.shape) == (4, 3, 32, 32)


# --------------------------------------------------------------------------- modules without a GPU
@pytest.mark.parametrize("name", sorted(MANIFEST["models"]))
def test_model_state_dict_keys_match_reference(name):
    m = MANIFEST["models"][name]
    mod = _quiet(getattr(F, name), **m["ctor"])
    sd = mod.state_dict()
    assert set(sd) == set(m["keys"]), set(sd) ^ set(m["keys"])
    for k, shp in m["keys"].items():
        assert list(sd[k].shape) == shp, k
    assert all(b.cond_bn_only for b in mod.modules() if isinstance(b, F.FFC_BN_ACT))


def test_module_init_and_keys():
    torch.manual_seed(0)
    m = F.ConditionalBatchNorm2d(64, 5)
    assert set(m.state_dict()) == {"bn.running_mean", "bn.running_var", "bn.num_batches_tracked", "embed.weight"}
    w = m.embed.weight.detach()
    assert torch.all(w[:, 64:] == 0) and abs(float(w[:, :64].mean()) - 1.0) < 0.01
    assert 0.01 < float(w[:, :64].std()) < 0.03
    blk = _quiet(F.FFC_BN_ACT, 8, 8, 3, 0.5, 0.5, 1, 1, norm_layer=F.ConditionalBatchNorm2d, num_classes=3)
    assert blk.cond_bn_only is False
    assert F.set_cond_bn(blk) is blk and blk.cond_bn_only is True
    assert F.set_cond_bn(blk, False).cond_bn_only is False


def test_errors_without_gpu():
    from fastfourierconvolution_amd._lib import FFCError
    m = F.ConditionalBatchNorm2d(4, 3)
    with pytest.raises(FFCError, match="no CPU fallback"):
        m(torch.randn(2, 4, 3, 3), torch.tensor([0, 1]))
    blk = _quiet(F.FFC_BN_ACT, 8, 8, 3, 0.5, 0.5, 1, 1, norm_layer=F.ConditionalBatchNorm2d, num_classes=3)
    with pytest.raises(TypeError, match="missing 1 required positional argument: 'y'"):
        blk((torch.randn(2, 4, 8, 8), torch.randn(2, 4, 8, 8)))
    plain = _quiet(F.FFC_BN_ACT, 8, 8, 3, 0.0, 0.0, 1, 1, norm_layer=nn.BatchNorm2d)
    with pytest.raises(TypeError, match="takes no label"):
        plain(torch.randn(2, 8, 8, 8), torch.tensor([0, 1]))
