"""The baseline generators (Generator32, Generator64, DCGenerator32) and the small-M 3x3 transposed head on the
CPU: state_dict keys and shapes against the reference's (manifest_baseline.json), the 'convT3' route of
rt.conv_route with its refusals, the router's cap against the kernel's constant, and the float64 references
of baseline_refs.py against float64 autograd of conv_transpose2d -- with the headroom check of the GPU
kernel test: PyTorch's own fp32 conv_transpose2d stays under a quarter of the kernel bound on every case's
input (observed worst 0.12 forward, 0.05 data gradient), so the bound leaves room for a correct fp32 kernel.
"""
import contextlib
import io
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import baseline_refs as R
from conftest import GOLDEN
from fastfourierconvolution_amd import _plan
from fastfourierconvolution_amd import _runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _manifest():
    with open(os.path.join(GOLDEN, "manifest_baseline.json")) as f:
        return json.load(f)


def test_exports():
    import fastfourierconvolution_amd as P
    for name in ("Generator32", "Generator64", "DCGenerator32"):
        assert name in P.__all__ and isinstance(getattr(P, name), type)


@pytest.mark.parametrize("tag", sorted(_manifest()["state_dict_keys"]))
def test_state_dict_is_the_references(tag):
    import fastfourierconvolution_amd as P
    m = _manifest()
    kind, mg = tag.split(":mg")
    with contextlib.redirect_stdout(io.StringIO()):
        mod = getattr(P, kind)(z_size=16, mg=int(mg))
    sd = mod.state_dict()
    assert list(sd) == m["state_dict_keys"][tag]
    assert {k: list(v.shape) for k, v in sd.items()} == m["state_dict_shapes"][tag]


def test_generators_do_not_ask_for_the_attention_matrix():
    import fastfourierconvolution_amd as P
    assert P.Self_Attn.need_attention is True
    for cls in (P.Generator32, P.Generator64):
        G = cls(16, mg=1)
        assert G.attn.need_attention is False and isinstance(G.noise_to_feature, torch.nn.Linear)
    assert P.Self_Attn(16, "relu").need_attention is True
    assert not hasattr(P.DCGenerator32(16, 4), "attn")


# --------------------------------------------------------------------------- route
def ct3(C, H=8, W=None):
    return _plan.Seg("convT", C, H, W or H, 3, 1, 1), 1


# id: (segments, M, bias per segment, addend, bn, switches off, route on both paths)
ROUTES = {
    "head": ([ct3(64)], 3, [1], 0, 0, (), "convT3"),
    "head_M4_nobias": ([ct3(64)], 4, [0], 0, 0, (), "convT3"),
    "head_odd_width": ([ct3(64, 33, 7)], 3, [1], 0, 0, (), "convT3"),
    "head_48": ([ct3(64, 48)], 3, [1], 0, 0, (), "convT3"),
    "head_cap": ([ct3(256)], 3, [1], 0, 0, (), "convT3"),
    "M5": ([ct3(64)], 5, [1], 0, 0, (), None),
    "over_cap": ([ct3(257)], 3, [1], 0, 0, (), None),
    "two_segments": ([ct3(32), ct3(32)], 3, [1, 0], 0, 0, (), None),
    "two_biases": ([ct3(32), ct3(32)], 3, [1, 1], 0, 0, (), None),
    "addend": ([ct3(64)], 3, [1], 1, 0, (), None),
    "bn": ([ct3(64)], 3, [1], 0, 1, (), None),
    "smallm_off": ([ct3(64)], 3, [1], 0, 0, ("USE_SMALLM",), None),
    "conv_layout": ([(ct3(64)[0], 0)], 3, [1], 0, 0, (), None),
    "stride2": ([(_plan.Seg("convT", 64, 8, 8, 3, 2, 1), 1)], 3, [1], 0, 0, (), None),
    "pad0": ([(_plan.Seg("convT", 64, 8, 8, 3, 1, 0), 1)], 3, [1], 0, 0, (), None),
    "out_pad": ([(_plan.Seg("convT", 64, 8, 8, 3, 1, 1, 1, 1), 1)], 3, [1], 0, 0, (), None),
}


def _weights(segs, M, biases):
    out = []
    for (sg, lay), b in zip(segs, biases):
        shape = (sg.C, M, sg.k, sg.k) if lay == 1 else (M, sg.C, sg.k, sg.k)
        out.append(rt.ConvWeight(torch.zeros(shape), lay, sg.k, sg.k, torch.zeros(M) if b else None))
    return out


@pytest.mark.parametrize("name", list(ROUTES))
def test_convt3_route(name, monkeypatch):
    segs, M, biases, addend, bn, off, want = ROUTES[name]
    for knob in off:
        monkeypatch.setattr(rt, knob, False)
    sgs = [sg for sg, _ in segs]
    w = _weights(segs, M, biases)
    assert rt.conv_route(sgs, w, M, bool(addend), bool(bn), rt.INFER_ROUTES) == want
    if not bn:
        assert rt.conv_route(sgs, w, M, bool(addend), False, rt.TRAIN_ROUTES, training=True) == want
    assert rt.conv_route(sgs, w, M, bool(addend), bool(bn), frozenset(("convT", "full", "conv3", "dense"))) is None


def test_router_cap_is_the_kernels():
    with open(os.path.join(ROOT, "fastfourierconvolution_amd", "csrc", "convt3_smallm.hip")) as f:
        m = re.search(r"constexpr\s+int\s+CT3_CMAX\s*=\s*(\d+)\s*;", f.read())
    assert m is not None and rt.RouteCaps.CONVT3_SMALLM_CMAX == int(m.group(1))


def test_backward_finds_the_head_job():
    """the data gradient goes to the direct kernel exactly where the forward took the 'convT3' route"""
    from fastfourierconvolution_amd import _autograd as ag
    sg = _plan.Seg("convT", 64, 8, 8, 3, 1, 1)
    spec = ag.conv_spec([(3, 3, 0.0)], [(0, 0, sg, 1, 0)])
    outs, edges = ag.parse_conv_spec(spec)
    x, w = torch.zeros(2, 64, 8, 8), torch.zeros(64, 3, 3, 3)
    assert ag._is_convt3_job(outs, edges, 0, x, [w])
    spec2 = ag.conv_spec([(3, 3, 0.0)], [(0, 0, sg, 1, 0), (0, 1, sg, 1, -1)])
    outs2, edges2 = ag.parse_conv_spec(spec2)
    assert not ag._is_convt3_job(outs2, edges2, 0, x, [w, w])
    spec3 = ag.conv_spec([(8, 0, 0.0)], [(0, 0, sg, 1, 0)])
    outs3, edges3 = ag.parse_conv_spec(spec3)
    assert not ag._is_convt3_job(outs3, edges3, 0, x, [torch.zeros(64, 8, 3, 3)])


# --------------------------------------------------------------------------- references
@pytest.mark.parametrize("name", list(R.CASES))
def test_references_against_float64_autograd(name):
    """head_ref / dgrad_ref (tap by tap) against conv_transpose2d and its float64 autograd; and the fp32
    conv_transpose2d against the references: under a quarter of the kernel bound"""
    B, C, M, H, W, has_bias, act, _ = R.CASES[name]
    x, w, bias, dpre = R.inputs(name)
    ref = R.head_ref(x, w, bias, act)
    xd = x.double().requires_grad_(True)
    pre = F.conv_transpose2d(xd, w.double(), None if bias is None else bias.double(), stride=1, padding=1)
    auto = R.act64(pre, act)
    assert tuple(ref.shape) == (B, M, H, W) and float((ref - auto.detach()).abs().max()) <= 1e-13
    (gx,) = torch.autograd.grad(pre, xd, dpre.double())
    dref = R.dgrad_ref(dpre, w)
    assert tuple(dref.shape) == (B, C, H, W) and float((dref - gx).abs().max()) <= 1e-12
    x32 = x.clone().requires_grad_(True)
    pre32 = F.conv_transpose2d(x32, w, bias, stride=1, padding=1)
    out32 = torch.tanh(pre32) if act == R.TANH else pre32
    (gx32,) = torch.autograd.grad(pre32, x32, dpre)
    wf, wd = R.worst(out32.detach(), ref), R.worst(gx32, dref)
    print(f"{name}: fp32 share of the bound forward {wf:.3f} dgrad {wd:.3f}")
    assert wf <= 0.25 and wd <= 0.25
