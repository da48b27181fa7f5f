"""The wide Self_Attn kernels (ffc_attnw_*, 72 <= C <= 256) without a GPU: on every input of
tests/test_gpu_attn_wide.py the formulas in plain float32 against the float64 references of tests/attn_refs.py,
the bounds that follow from it (tests/attn_wide_cases.py), four planted defects against those bounds, the
directed inputs, the shape queries, and the refusals of the entry points.

A bound is TOL_K = 1e-5 normwise where plain float32 stays under a quarter of it, and four times the float32
error on that input where it does not; every test prints what it measured.  Plain float32 itself has to stay
inside TOL_K on every input: an input that misses it is changed, never the bound.
"""
import ctypes

import pytest
import torch

import attn_refs as R
import attn_wide_cases as W
from fastfourierconvolution_amd import _lib


def _show(name, errs, bounds):
    print(name, {k: f"{e:.2e}" + ("" if bounds[k] == W.TOL_K else f" (bound {bounds[k]:.2e})") for k, e in errs.items()})


@pytest.mark.parametrize("name", list(W.SHAPES))
def test_layer_inputs_in_float32(name):
    errs, bounds = W.layer_fp32_errors(name), W.layer_bounds(name)
    _show(name, errs, bounds)
    assert set(errs) == set(W.LAYER_OUTPUTS)
    assert max(errs.values()) <= W.TOL_K, errs
    S = W.case(name)["ref"]["S"]
    assert float(S.abs().max()) <= 12.0


@pytest.mark.parametrize("name", W.CORE_ALL)
def test_core_inputs_in_float32(name):
    errs, bounds = W.core_fp32_errors(name), W.core_bounds(name)
    _show(name, errs, bounds)
    assert set(errs) == set(W.CORE_OUTPUTS)
    assert max(errs.values()) <= W.TOL_K, errs


def test_float32_scores_of_the_directed_inputs_are_exact():
    for name in ("offset", "neg_offset", "early_max", "late_max"):
        c = W.core_case(name)
        S32 = c["q"].transpose(1, 2) @ c["k"]
        assert torch.equal(S32.double(), c["fwd"]["S"]), name
    for name, sign in (("offset", 1.0), ("neg_offset", -1.0)):
        S = W.core_case(name)["fwd"]["S"]
        assert float((S - sign * 100.0).abs().max()) <= 4.0
    N = 160
    early, late = W.core_case("early_max")["fwd"]["S"], W.core_case("late_max")["fwd"]["S"]
    assert bool((early.argmax(-1) == 0).all()) and bool((late.argmax(-1) == N - 1).all())
    tiles = torch.stack([late[..., j:j + 32].max(-1).values for j in range(0, N, 32)], -1)
    assert bool((tiles[..., 1:] > tiles[..., :-1]).all()), "late_max: a key tile does not raise the maximum"


@pytest.mark.parametrize("defect", list(W.DEFECTS))
def test_planted_defects_exceed_the_bounds(defect):
    name, outputs = W.DEFECTS[defect]
    c, bounds = W.core_case(name), W.core_bounds(name)
    errs = W.core_errors(c, {k: v for k, v in W.fp32_core_case(c, defect).items() if k in outputs})
    print(defect, name, {k: f"{e:.2e} / {bounds[k]:.2e}" for k, e in errs.items()})
    for k in outputs:
        assert errs[k] > 10.0 * bounds[k], (defect, k, errs[k], bounds[k])


def test_layer_defect_shows_through_the_gradients():
    """the same mistakes planted in the layer's restatement move its outputs and parameter gradients"""
    name = "b3_c256_10x16"
    c, bounds = W.case(name), W.layer_bounds(name)
    errs = W.layer_errors(c, W.fp32_layer(c, "dP_over_64_channels"))
    print({k: f"{e:.2e}" for k, e in errs.items()})
    for k in ("query_conv.weight", "key_conv.weight", "query_conv.bias", "x"):
        assert errs[k] > 10.0 * bounds[k], k


def test_attnw_supported_answers_without_a_gpu():
    L = _lib.load()
    for shape in ((72, 1, 1), (256, 4, 4), (136, 3, 11)):
        assert L.ffc_attnw_supported(*shape) == 1, shape
        assert L.ffc_attnw_ws_floats(2, *shape) > 0, shape
    for shape in ((64, 8, 8), (264, 8, 8), (100, 4, 4), (256, 0, 4), (256, 257, 256)):
        assert L.ffc_attnw_supported(*shape) == 0, shape
        assert L.ffc_attnw_ws_floats(2, *shape) == 0, shape
    assert L.ffc_attnw_ws_floats(2, 256, 10, 16) == 2 * 160 + 2
    assert L.ffc_attnw_ws_floats(0, 256, 4, 4) == 0 and L.ffc_attnw_ws_floats(65536, 256, 4, 4) == 0
    # the narrow entry points keep their range
    assert L.ffc_attn_supported(64, 8, 8) == 1 and L.ffc_attn_supported(72, 8, 8) == 0


@pytest.mark.parametrize("C", [64, 100, 264])
def test_unsupported_shape_is_refused_before_a_launch(C):
    L = _lib.load()
    null = ctypes.c_void_p(None)
    calls = {
        "ffc_attnw_forward": lambda: L.ffc_attnw_forward(null, null, null, 0, null, null, null, null, null, 2, C, 8, 8,
                                                         null),
        "ffc_attnw_matrix": lambda: L.ffc_attnw_matrix(null, null, 0, null, null, 2, C, 8, 8, null),
        "ffc_attnw_backward": lambda: L.ffc_attnw_backward(null, null, null, null, 0, null, null, null, null, null,
                                                           null, 0, null, null, 2, C, 8, 8, null),
    }
    for name, call in calls.items():
        assert call() == -1
        msg = L.ffc_last_error().decode()
        print(msg)
        assert "unsupported" in msg and name in msg and f", {C}, 8, 8)" in msg


def test_reference_measures_agree_with_attn_refs():
    """core_errors is the normwise measure of attn_refs on the same references"""
    c = W.core_case("3x136x4x4")
    got = W.fp32_core_case(c)
    assert W.core_errors(c, {"o": got["o"]})["o"] == R.normwise(got["o"], c["fwd"]["o"])
