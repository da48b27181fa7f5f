"""Self_Attn without a GPU: the float64 restatement (tests/attn_refs.py) against the reference's own
fixtures (tests/golden/gen_golden_attn.py) and against torch autograd, the conditioning of every input the
GPU tests use, the layer's state_dict, the ffc_attn_* shape query and refusals, and the CPU refusal.

Bounds: the restatement against the float32-stored fixtures 1e-6 normwise (the fixtures' own rounding is
6e-8 per element); its gradients against float64 autograd 1e-12; the fp32 ATen composition on the CPU
against float64 1e-5, the kernels' bound (tests/test_gpu_attn_kernels.py): an input that misses it is
changed, never the bound.  Every test prints what it measured.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import attn_refs as R
import fastfourierconvolution_amd as F
from conftest import GOLDEN
from fastfourierconvolution_amd import _lib
from fixture_weights import input_array, make_state

TOL_K = 1e-5


def _manifest():
    with open(os.path.join(GOLDEN, "manifest_attn.json")) as f:
        return json.load(f)


def _golden(c):
    data = np.load(os.path.join(GOLDEN, c["name"] + ".npz"))
    p = {k: torch.from_numpy(v) for k, v in make_state(c["seed"], c["specs"]).items()}
    x = torch.from_numpy(input_array(c["seed"], "x", c["inputs"]["x"]))
    cot = torch.from_numpy(input_array(c["seed"] + 11, "cot:out", c["inputs"]["x"]))
    return data, p, x, cot


@pytest.mark.parametrize("name", ["attn16", "attn64"])
def test_refs_match_reference_fixtures(name):
    c = next(c for c in _manifest()["cases"] if c["name"] == name)
    data, p, x, cot = _golden(c)
    assert abs(float(p["gamma"])) > 0.1
    r = R.attn_ref(x, p)
    g = R.attn_ref_backward(x, p, cot)
    errs = {"out": R.normwise(r["out"], torch.from_numpy(data["ref.out"])),
            "attention": R.normwise(r["attention"], torch.from_numpy(data["ref.attention"])),
            "x": R.normwise(g["x"], torch.from_numpy(data["gin.x"]))}
    for k in R.NAMES:
        errs[k] = R.grad_err(k, torch.from_numpy(data["gpar." + k]), g)
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-6, errs


@pytest.mark.parametrize("name", list(R.SHAPES)[:4] + list(R.DIRECTED))
def test_ref_gradients_match_autograd_fp64(name):
    c = R.case(name)
    p = {k: v.double().requires_grad_(True) for k, v in c["p"].items()}
    x = c["x"].double().requires_grad_(True)
    out, _ = R.aten_composition(x, p)
    (out * c["dy"].double()).sum().backward()
    errs = {"x": R.normwise(c["grads"]["x"], x.grad)}
    for k in R.NAMES:
        errs[k] = R.grad_err(k, p[k].grad, c["grads"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("name", list(R.SHAPES) + list(R.DIRECTED))
def test_gpu_inputs_are_well_conditioned(name):
    """proves the inputs, not the kernel: plain fp32 ATen on the CPU is inside the kernels' bound"""
    c = R.case(name)
    S = c["ref"]["S"]
    print(name, f"scores: std {float(S.std(unbiased=False)):.2f}, max |S| {float(S.abs().max()):.2f}")
    if name in R.SHAPES:
        assert float(S.abs().max()) <= 12.0
        if S.numel() > 1:
            assert 1.0 <= float(S.std(unbiased=False)) <= 3.0
    p = {k: v.clone().requires_grad_(True) for k, v in c["p"].items()}
    x = c["x"].clone().requires_grad_(True)
    out, attention = R.aten_composition(x, p)
    (out * c["dy"]).sum().backward()
    errs = {"out": R.normwise(out, c["ref"]["out"]), "attention": R.normwise(attention, c["ref"]["attention"]),
            "x": R.normwise(x.grad, c["grads"]["x"])}
    for k in R.NAMES:
        if name == "gamma0" and k != "gamma":
            assert float(c["grads"][k].abs().max()) == 0.0 and float(p[k].grad.abs().max()) == 0.0
            continue
        errs[k] = R.grad_err(k, p[k].grad, c["grads"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL_K, errs


def test_directed_inputs_do_what_they_claim():
    late = R.case("late_max")["ref"]["S"]
    N = late.shape[-1]
    assert bool((late.argmax(-1) >= N - 32).all()), "late_max: a row's largest score is not in the last key tile"
    tile_max = torch.stack([late[..., j:j + 32].max(-1).values for j in range(0, N, 32)], -1)
    assert bool((tile_max[..., 1:] > tile_max[..., :-1]).all()), "late_max: a key tile does not raise the maximum"
    mask = R.case("mask")["ref"]["S"]
    print(f"mask: scores in [{float(mask.min()):.2f}, {float(mask.max()):.2f}]")
    assert float(mask.max()) <= -7.0 and float(mask.min()) >= -13.0


def test_state_dict_matches_reference():
    m = _manifest()
    for name, C in (("attn16", 16), ("attn64", 64)):
        mod = F.Self_Attn(C, "relu")
        sd = mod.state_dict()
        assert list(sd) == m["state_dict_keys"][name]
        assert {k: list(v.shape) for k, v in sd.items()} == m["state_dict_shapes"][name]
        assert mod.chanel_in == C and mod.activation == "relu" and mod.need_attention is True
        assert float(mod.gamma) == 0.0 and isinstance(mod.softmax, torch.nn.Softmax)
    assert "Self_Attn" in F.__all__


def test_attn_supported_answers_without_a_gpu():
    L = _lib.load()
    assert L.ffc_attn_supported(64, 64, 64) == 1
    assert L.ffc_attn_supported(16, 6, 6) == 1
    assert L.ffc_attn_supported(8, 1, 1) == 1
    assert L.ffc_attn_supported(12, 8, 8) == 0
    assert L.ffc_attn_supported(128, 8, 8) == 0
    assert L.ffc_attn_supported(64, 0, 8) == 0
    assert L.ffc_attn_ws_floats(2, 64, 8, 8) == 2 * 64 + 2
    assert L.ffc_attn_ws_floats(2, 12, 8, 8) == 0


@pytest.mark.parametrize("C", [12, 128])
def test_unsupported_shape_is_refused_before_a_launch(C):
    L = _lib.load()
    null = ctypes.c_void_p(None)
    calls = {
        "ffc_attn_forward": lambda: L.ffc_attn_forward(null, null, null, 0, null, null, null, null, null, 2, C, 8, 8,
                                                       null),
        "ffc_attn_matrix": lambda: L.ffc_attn_matrix(null, null, 0, null, null, 2, C, 8, 8, null),
        "ffc_attn_backward": lambda: L.ffc_attn_backward(null, null, null, null, 0, null, null, null, null, null,
                                                         null, 0, null, null, 2, C, 8, 8, null),
    }
    for name, call in calls.items():
        assert call() == -1
        msg = L.ffc_last_error().decode()
        print(msg)
        assert "unsupported" in msg and name in msg and f", {C}, 8, 8)" in msg


def test_cpu_tensor_is_refused():
    mod = F.Self_Attn(16, "relu")
    with pytest.raises(_lib.FFCError, match="no CPU fallback"):
        mod(torch.zeros(1, 16, 4, 4))
