"""CPU checks of the ResNet SNGAN family: the fp64 restatements of tests/resnet_refs.py against F.interpolate /
avg_pool2d / autograd, the tolerance rule of the GPU kernel file, the planted defects, the block formulas against
the reference's own fp64 fixtures (tests/golden/gen_golden_resnet.py) and the state_dict key lists."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_refs as R
from conftest import GOLDEN
from fixture_weights import input_array

torch.set_num_threads(2)


def _manifest():
    with open(os.path.join(GOLDEN, "manifest_resnet.json")) as f:
        return json.load(f)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("h,w", R.CPU_PLANES)
def test_up2b_is_interpolate_and_its_adjoint_is_autograds(h, w):
    x = _rand(2, 3, h, w, seed=h * 10 + w).requires_grad_(True)
    ref = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    y, _ = R.act_up2b(x.detach())
    assert float((y - ref.detach()).abs().max()) <= 1e-14
    g = _rand(2, 3, 2 * h, 2 * w, seed=5)
    (gx,) = torch.autograd.grad(ref, x, g)
    dx, _ = R.up2b_adjoint(g)
    assert float((dx - gx).abs().max()) <= 1e-14
    # <up(x), g> = <x, up^T(g)>
    assert abs(float((y * g).sum() - (x.detach() * dx).sum())) <= 1e-12 * float((y.abs() * g.abs()).sum())
    # activation at the low resolution, with both affine forms
    sc, sh = _rand(3, seed=6), _rand(3, seed=7)
    y2, _ = R.act_up2b(x.detach(), sc, sh, act=1)
    ref2 = F.interpolate(torch.relu(sc.view(1, 3, 1, 1) * x.detach() + sh.view(1, 3, 1, 1)), scale_factor=2,
                         mode="bilinear", align_corners=False)
    assert float((y2 - ref2).abs().max()) <= 1e-14
    scb, shb = _rand(2, 3, seed=8), _rand(2, 3, seed=9)
    y3, _ = R.act_up2b(x.detach(), scb, shb, act=1)
    ref3 = F.interpolate(torch.relu(scb[:, :, None, None] * x.detach() + shb[:, :, None, None]), scale_factor=2,
                         mode="bilinear", align_corners=False)
    assert float((y3 - ref3).abs().max()) <= 1e-14


@pytest.mark.parametrize("h,w", R.CPU_PLANES)
def test_pool_and_sum_pool_are_atens(h, w):
    x = _rand(2, 3, 2 * h, 2 * w, seed=3).requires_grad_(True)
    ref = torch.relu(F.avg_pool2d(x, 2))
    y, _ = R.pool2_act(x.detach(), act=1)
    assert float((y - ref).abs().max()) <= 1e-15
    g = _rand(2, 3, h, w, seed=4)
    (gx,) = torch.autograd.grad(ref, x, g)
    assert float((R.pool2_act_bwd(y, g, act=1)[0] - gx).abs().max()) <= 1e-15
    x = _rand(2, 3, h, w, seed=11).requires_grad_(True)
    ref = torch.sum(torch.relu(x), (2, 3))
    assert float((R.relu_sum_pool(x.detach())[0] - ref).abs().max()) <= 1e-14
    go = _rand(2, 3, seed=12)
    (gx,) = torch.autograd.grad(ref, x, go)
    assert torch.equal(R.relu_sum_pool_bwd(x.detach(), go)[0], gx)


def _kernel_quantities(d, dtype, **defect):
    """every (name, value, scale) the GPU file compares, computed at ``dtype``"""
    out = []
    for form in R.SCALE_FORMS:
        sc, sh = R.scale_shift(d, form)
        for act in R.ACTS:
            out.append((f"up2b/{form}/{act}",) + R.act_up2b(d["x"], sc, sh, act, dtype=dtype, **defect))
    out.append(("adjoint",) + R.up2b_adjoint(d["dy"], dtype=dtype))
    for act in R.ACTS:
        out.append((f"pool2_act/{act}",) + R.pool2_act(d["dy"], act, dtype=dtype))
    out.append(("relu_sum",) + R.relu_sum_pool(d["x"], dtype=dtype))
    return out


def _worst_f32_share(tol):
    worst = 0.0
    for h, w in R.PLANES:
        for B, C in R.BCS:
            d = R.inputs(h, w, B, C)
            for (name, ref, scale), (_, got, _) in zip(_kernel_quantities(d, torch.float64),
                                                       _kernel_quantities(d, torch.float32)):
                worst = max(worst, R.share(got, ref, scale, tol))
    return worst


def test_tol_rule():
    """TOL is the smallest power of ten at which the plain fp32 restatement stays under a quarter of every bound"""
    at, tenth = _worst_f32_share(R.TOL), _worst_f32_share(R.TOL / 10)
    print(f"OBS worst fp32 share at TOL = {R.TOL:g}: {at:.3f}; at TOL / 10: {tenth:.3f}")
    assert at < 0.25
    assert tenth >= 0.25, "TOL is not the smallest power of ten"


DEFECTS = {"weights swapped": dict(near=0.25, far=0.75), "edge wrapped": dict(wrap=True),
           "activation after interpolation": dict(act_after=True)}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_forward_defects_exceed_the_bound(name):
    d = R.inputs(7, 9, 1, 3)
    sc, sh = R.scale_shift(d, "channel")
    ref, scale = R.act_up2b(d["x"], sc, sh, act=1)
    bad, _ = R.act_up2b(d["x"], sc, sh, act=1, **DEFECTS[name])
    assert R.share(bad, ref, scale) > 1.0
    if name != "edge wrapped":   # a 1-pixel axis has no neighbour to wrap to
        d1 = R.inputs(1, 5, 1, 3)
        ref, scale = R.act_up2b(d1["x"], *R.scale_shift(d1, "channel"), act=1)
        bad, _ = R.act_up2b(d1["x"], *R.scale_shift(d1, "channel"), act=1, **DEFECTS[name])
        assert R.share(bad, ref, scale) > 1.0


def test_planted_adjoint_and_sum_defects_exceed_the_bound():
    for h, w in ((7, 9), (1, 1), (2, 3)):
        d = R.inputs(h, w, 1, 3)
        ref, scale = R.up2b_adjoint(d["dy"])
        bad, _ = R.up2b_adjoint(d["dy"], edges=False)      # the clamped taps' weights dropped at the edges
        assert R.share(bad, ref, scale) > 1.0
        ref, scale = R.relu_sum_pool(d["x"])
        bad, _ = R.relu_sum_pool(d["x"], relu=False)        # a plain sum
        assert R.share(bad, ref, scale) > 1.0


def _block_case(name):
    c = {c["name"]: c for c in _manifest()["cases"]}[name]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    from fixture_weights import make_state
    st = make_state(c["seed"], c["specs"])
    P = {k[len("eff."):]: torch.from_numpy(data[k]).double() for k in data.files if k.startswith("eff.")}
    P.update({k: torch.from_numpy(v).double() for k, v in st.items() if k.endswith(".bias")})
    x = torch.from_numpy(input_array(c["seed"], "x", c["inputs"]["x"])).double()
    return c, data, P, x


@pytest.mark.parametrize("name,down", [("dblock_same_train", False), ("dblock_down_train", True),
                                       ("dblock_same_eval", False), ("dblock_down_eval", True)])
def test_dblock_shortcut_sees_relu_x(name, down):
    """the reference's in-place ReLU: its fp64 output is the formula with the shortcut on relu(x), in the fused
    form (one pooling of the sum) that resnet.py runs; the shortcut on x itself is off by far more than fp32"""
    c, data, P, x = _block_case(name)
    ref = torch.from_numpy(data["ref.out"]).double()
    n = float(ref.norm())
    for fused in (True, False):
        assert float((R.dblock(x, P, down, fused=fused) - ref).norm()) / n <= 2e-7   # stored as float32
    assert float((R.dblock(x, P, down, shortcut_relu=False) - ref).norm()) / n > 1e-2


def test_pointwise_conv_commutes_with_the_upsample():
    x, w, b = _rand(2, 5, 3, 4, seed=1), _rand(7, 5, 1, 1, seed=2), _rand(7, seed=3)
    lo = R.up(R.conv(x, w, b, 0))
    hi = R.conv(R.up(x), w, b, 0)
    assert float((lo - hi).abs().max()) <= 1e-13
    w2 = _rand(5, 7, 1, 1, seed=4)   # and with the pooling: c_sc(pool(x)) = pool(c_sc(x))
    assert float((R.pool(R.conv(hi, w2, None, 0)) - R.conv(R.pool(hi), w2, None, 0)).abs().max()) <= 1e-13


def test_state_dict_keys_are_the_references():
    import fastfourierconvolution_amd as ffc
    man = _manifest()
    seen = {}
    for c in man["cases"]:
        tag = c["kind"] + ":" + ",".join(f"{k}={v}" for k, v in c["ctor"].items())
        mod = getattr(ffc, c["kind"])(**c["ctor"])
        sd = mod.state_dict()
        assert list(sd) == man["state_dict_keys"][tag], tag
        assert {k: list(v.shape) for k, v in sd.items()} == man["state_dict_shapes"][tag], tag
        seen[c["kind"]] = len(sd)
    assert seen["SNGANGenerator128"] == 119 and seen["SNGANDiscriminator128"] == 72
    for name in ("GBlock", "DBlock", "DBlockOptimized", "SNGANGenerator128", "SNGANDiscriminator128"):
        assert name in ffc.__all__
    G = ffc.SNGANGenerator128()
    assert (G.nz, G.ngf, G.bottom_width) == (128, 1024, 4) and G.l1.out_features == 16 * 1024
    assert any(k.endswith("c_sc.weight_u") for k in G.state_dict())


def test_initialisation_and_attributes():
    import fastfourierconvolution_amd as ffc
    torch.manual_seed(0)
    b = ffc.GBlock(8, 4, upsample=True)
    assert b.learnable_sc and b.hidden_channels == 4 and isinstance(b.b1, torch.nn.BatchNorm2d)
    # xavier_uniform_ bounds: gain * sqrt(6 / (fan_in + fan_out))
    for conv, gain in ((b.c1, 2 ** 0.5), (b.c2, 2 ** 0.5), (b.c_sc, 1.0)):
        w = conv.weight_orig
        k = w.shape[2] * w.shape[3]
        lim = gain * (6.0 / (w.shape[1] * k + w.shape[0] * k)) ** 0.5
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.8 * lim
    d = ffc.DBlock(4, 4)
    assert not d.learnable_sc and not hasattr(d, "c_sc") and d.hidden_channels == 4
    assert isinstance(ffc.GBlock(8, 4, num_classes=5).b1, ffc.ConditionalBatchNorm2d)


def test_refusals_without_a_gpu():
    import fastfourierconvolution_amd as ffc
    from fastfourierconvolution_amd._lib import FFCError
    with pytest.raises(FFCError, match="no CPU fallback"):
        ffc.SNGANDiscriminator128(ndf=32)(torch.randn(1, 3, 32, 32))
    with pytest.raises(FFCError, match="no CPU fallback"):
        ffc.SNGANGenerator128(nz=8, ngf=32, bottom_width=1)(torch.randn(1, 8))


def test_argument_rejections_without_a_gpu():
    """every entry point refuses bad arguments before any launch (no device is touched)"""
    import ctypes
    from fastfourierconvolution_amd import _lib
    L = _lib.load()
    p = ctypes.c_void_p(64)   # never dereferenced
    E = -1
    assert L.ffc_act_up2b(None, None, None, 0, 1, 1, 2, 2, 0, 0.0, p, None) == E
    assert L.ffc_act_up2b(p, p, None, 0, 1, 1, 2, 2, 0, 0.0, p, None) == E and b"go together" in L.ffc_last_error()
    assert L.ffc_act_up2b(p, None, None, 0, 1, 1, 0, 2, 0, 0.0, p, None) == E
    assert L.ffc_act_up2b(p, None, None, 0, 1 << 15, 1 << 15, 1, 1, 0, 0.0, p, None) == E
    assert b"32-bit" in L.ffc_last_error()
    assert L.ffc_up2b_adjoint(p, 1, 2, -1, p, None) == E and L.ffc_up2b_adjoint(p, 1, 2, 2, None, None) == E
    assert L.ffc_up2b_adjoint(p, 1 << 20, 1 << 10, 1 << 10, p, None) == E and b"32-bit" in L.ffc_last_error()
    assert L.ffc_pool2_act(p, 1, 3, 2, 1, 0.0, p, None) == E and b"odd" in L.ffc_last_error()
    assert L.ffc_pool2_act(p, 1, 2, 5, 1, 0.0, p, None) == E and b"odd" in L.ffc_last_error()
    assert L.ffc_pool2_act(p, 1, 2, 2, 5, 0.0, p, None) == E and b"activation" in L.ffc_last_error()
    assert L.ffc_pool2_act(None, 1, 2, 2, 1, 0.0, p, None) == E
    assert L.ffc_pool2_act_bwd(p, None, 1, 2, 2, 1, 0.0, p, None) == E
    assert L.ffc_pool2_act_bwd(p, p, 0, 2, 2, 1, 0.0, p, None) == E
    assert L.ffc_relu_sum_pool(p, 1, 0, p, None) == E and L.ffc_relu_sum_pool(p, 1, 4, None, None) == E
    assert L.ffc_relu_sum_pool(p, 1 << 31, 2, p, None) == E and b"32-bit" in L.ffc_last_error()
    assert L.ffc_relu_sum_pool_bwd(p, p, 1, 4, None, None) == E and L.ffc_relu_sum_pool_bwd(p, p, 1, -4, p, None) == E


def test_head_stays_on_the_implicit_gemm_route():
    """the Conv2d(ngf / 16, 3, 3, 1, 1) + tanh head has no direct training route yet: conv_route answers None (the
    implicit-GEMM kernels) for it, as for every Conv2d 3x3 job of the training path"""
    from fastfourierconvolution_amd import _plan, _runtime as rt
    w = rt.ConvWeight(torch.empty(3, 64, 3, 3), 0, 3, 3, torch.empty(3))
    assert rt.conv_route((_plan.Seg("conv", 64, 128, 128, 3, 1, 1),), [w], 3, False, False, rt.TRAIN_ROUTES,
                         training=True) is None
    assert rt.TRAIN_ROUTES == frozenset(("convT", "full", "dense", "convT3"))
