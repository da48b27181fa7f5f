"""Self_Attn on the GPU: the kernels of csrc/attn_kernels.hip through the layer (stacked projection on the
pointwise GEMM, ffc::self_attn, ffc::self_attn_matrix, ffc::self_attn_bwd) against the float64 restatement
of tests/attn_refs.py at their edge shapes, the directed cases (late maximum, mask, gamma = 0), run-to-run
bitwise equality of the backward, the memory bound without the attention matrix, hipGraph capture, and
the reference's own fixtures.

Bound: 1e-5 normwise against float64 (as tests/test_gpu_sn.py); the key bias's gradient, which is exactly
zero, against the scale of its cancellation (attn_refs.grad_err).  tests/test_attn_cpu.py proves that plain
fp32 ATen meets the same bound on every input used here.  Every test prints what it measured.

Observed maxima on the first MI355X run (normwise): out 2.3e-7, attention 1.2e-6, gradients 8.6e-6
(query_conv.weight of the late-maximum case; 3.4e-6 on the random shapes, gamma at (2, 64, 8, 8)).
"""
import json
import os

import numpy as np
import pytest
import torch

import attn_refs as R
import fastfourierconvolution_amd as F
from conftest import GOLDEN
from fixture_weights import input_array, make_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_K = 1e-5


def _layer(p, need_attention=True):
    C = p["value_conv.weight"].shape[0]
    mod = F.Self_Attn(C, "relu")
    mod.load_state_dict(p)
    mod.need_attention = need_attention
    return mod.to(DEV)


def _run(p, x, dy, need_attention=True):
    """forward + backward of the layer -> (out, attention, {name: gradient})"""
    mod = _layer(p, need_attention)
    xd = x.to(DEV).requires_grad_(True)
    out, attention = mod(xd)
    (out * dy.to(DEV)).sum().backward()
    grads = {k: v.grad for k, v in mod.named_parameters()}
    grads["x"] = xd.grad
    return out.detach(), attention, grads


def _errors(name, c, out, attention, grads):
    errs = {"out": R.normwise(out, c["ref"]["out"]), "attention": R.normwise(attention, c["ref"]["attention"]),
            "x": R.normwise(grads["x"], c["grads"]["x"])}
    for k in R.NAMES:
        errs[k] = R.grad_err(k, grads[k], c["grads"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    return errs


@pytest.mark.parametrize("name", list(R.SHAPES) + ["late_max", "mask"])
def test_forward_and_gradients_against_fp64(name):
    c = R.case(name)
    out, attention, grads = _run(c["p"], c["x"], c["dy"])
    assert attention.shape == c["ref"]["attention"].shape and not attention.requires_grad
    errs = _errors(name, c, out, attention, grads)
    assert max(errs.values()) <= TOL_K, errs


def test_gamma_zero_returns_x_bit_for_bit():
    c = R.case("gamma0")
    out, attention, grads = _run(c["p"], c["x"], c["dy"])
    assert torch.equal(out.cpu(), c["x"])
    assert torch.equal(grads["x"].cpu(), c["dy"])   # do = 0: only the residual carries a gradient
    for k in R.NAMES[:-1]:
        assert float(grads[k].abs().max()) == 0.0, k
    errs = {"gamma": R.normwise(grads["gamma"], c["grads"]["gamma"]),
            "attention": R.normwise(attention, c["ref"]["attention"])}
    print("gamma0", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL_K, errs


def test_backward_is_deterministic():
    c = R.case("b1_c64_24x24")
    _, _, g1 = _run(c["p"], c["x"], c["dy"], need_attention=False)
    _, _, g2 = _run(c["p"], c["x"], c["dy"], need_attention=False)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    print("deterministic:", sorted(g1))


def test_without_attention_nothing_n_by_n_is_allocated():
    B, C, H, W = 4, 64, 64, 64
    N = H * W
    gen = torch.Generator().manual_seed(301)
    p = R._random_params(C, gen)
    for n in ("query_conv", "key_conv"):   # the N^2 = 16.8 M scores of a sample stay inside +-12 (see attn_refs.case)
        p[n + ".weight"].mul_(0.7)
    x = torch.randn(B, C, H, W, generator=gen)
    mod = _layer(p, need_attention=False)
    xd = x.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with torch.no_grad():
        out, attention = mod(xd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"need_attention off: peak rose by {rise / 2 ** 20:.1f} MiB (one matrix: {B * N * N * 4 / 2 ** 20:.0f} MiB)")
    assert attention is None
    assert rise < B * N * N * 4
    mod.need_attention = True
    with torch.no_grad():
        out2, attention = mod(xd)
    assert tuple(attention.shape) == (B, N, N)
    assert torch.equal(out, out2)
    # one row block (the first 64 queries of sample 0) and sample 0's output against float64
    p0 = {k: v.double() for k, v in p.items()}
    r = R.attn_ref(x[:1], p0)
    errs = {"attention[0, :64]": R.normwise(attention[0, :64], r["attention"][0, :64]),
            "out[0]": R.normwise(out[0], r["out"][0])}
    print({k: f"{v:.2e}" for k, v in errs.items()}, f"max |S| {float(r['S'].abs().max()):.2f}")
    assert max(errs.values()) <= TOL_K, errs


def test_no_grad_forward_captures_into_a_graph():
    c, c2 = R.case("b2_c32_10x10"), R.case("mask")   # the same shape, other x
    mod = _layer(c["p"], need_attention=False)
    static_x = c["x"].to(DEV).clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out, _ = mod(static_x)
        graph.replay()
        e0 = R.normwise(static_out, c["ref"]["out"])
        static_x.copy_(c2["x"].to(DEV))
        mod.gamma.fill_(-1.3)
        graph.replay()
        p2 = dict(c["p"], gamma=torch.full((1,), -1.3))
        e1 = R.normwise(static_out, R.attn_ref(c2["x"], p2)["out"])
    print(f"graph replay: {e0:.2e}; with a changed x and gamma: {e1:.2e}")
    assert max(e0, e1) <= TOL_K


@pytest.mark.parametrize("name", ["attn16", "attn64"])
def test_layer_against_reference_fixtures(name):
    with open(os.path.join(GOLDEN, "manifest_attn.json")) as f:
        c = next(c for c in json.load(f)["cases"] if c["name"] == name)
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    p = {k: torch.from_numpy(v) for k, v in make_state(c["seed"], c["specs"]).items()}
    x = torch.from_numpy(input_array(c["seed"], "x", c["inputs"]["x"]))
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", c["inputs"]["x"]))
    out, attention, grads = _run(p, x, cot)
    scale = R.attn_ref_backward(x, p, cot)["key_conv.bias.scale"]
    errs = {"out": R.normwise(out, torch.from_numpy(data["ref.out"])),
            "attention": R.normwise(attention, torch.from_numpy(data["ref.attention"])),
            "x": R.normwise(grads["x"], torch.from_numpy(data["gin.x"]))}
    for k in R.NAMES:
        ref = {k: torch.from_numpy(data["gpar." + k]).double(), "key_conv.bias.scale": scale}
        errs[k] = R.grad_err(k, grads[k], ref)
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL_K, errs


def test_unsupported_channels_raise_not_implemented():
    mod = F.Self_Attn(24, "relu").to(DEV)
    mod.chanel_in = 12
    with pytest.raises(NotImplementedError, match=r"\(1, 12, 4, 4\)"):
        mod(torch.zeros(1, 12, 4, 4, device=DEV))
