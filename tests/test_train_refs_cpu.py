"""The float64 references of tests/train_refs.py are the operations themselves, not a restatement of
the kernels they judge in test_gpu_train_kernels.py: each is checked here, on the CPU, against an
independent statement of the same operation (float64 throughout; bounds are float64 round-off)."""
import math

import pytest
import torch
import torch.nn as nn

import train_refs as tr


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


# --------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("name", [n for n in tr.WGRAD_CASES if n != "h"])
def test_wgrad_formula_is_conv_and_convT_autograd(name):
    """the U/V formula (unfold + contraction, and explicit loops on the smallest cases) equals autograd of
    conv2d with (dy, x) = (U, V) and of conv_transpose2d with (x, dy) = (U, V)"""
    U, V = tr.wgrad_inputs(name)
    _, _, k, s, p, d, _, _ = tr.WGRAD_CASES[name]
    f = tr.wgrad_formula(U, V, k, s, p, d)
    assert _rel(tr.wgrad_ref_conv(U, V, k, s, p, d), f) <= 1e-13
    assert _rel(tr.wgrad_ref_convT(U, V, k, s, p, d), f) <= 1e-13
    assert _rel(tr.wgrad_ref(name)[2], f) <= 1e-13
    if U.numel() * V.shape[1] * k * k <= 40000:   # cases d, e, f, g: the definition as written, term by term
        B, Mu, PH, PW = U.shape
        _, Nv, VH, VW = V.shape
        Ud, Vd = U.double(), V.double()
        loops = torch.zeros(Mu, Nv, k, k, dtype=torch.float64)
        for kh in range(k):
            for kw in range(k):
                for qy in range(PH):
                    for qx in range(PW):
                        iy, ix = qy * s - p + kh * d, qx * s - p + kw * d
                        if 0 <= iy < VH and 0 <= ix < VW:
                            loops[:, :, kh, kw] += Ud[:, :, qy, qx].t() @ Vd[:, :, iy, ix]
        assert _rel(loops, f) <= 1e-13


def test_wgrad_case_table_is_the_issue_table():
    """the properties each case is there for (what the kernel branches on)"""
    P = {n: c[0][2] * c[0][3] for n, c in tr.WGRAD_CASES.items()}
    K = {n: c[0][0] * P[n] for n, c in tr.WGRAD_CASES.items()}
    NT = {n: c[1][1] * c[2] ** 2 for n, c in tr.WGRAD_CASES.items()}
    assert P["a"] % 8 == 0 and K["a"] // 8 == 16 and 17 in tr.WGRAD_CASES["a"][7]        # one empty split
    assert P["b"] == 25 and P["d"] == 36 and P["e"] == 12 and P["f"] == P["g"] == 1       # scalar gather
    assert tr.WGRAD_CASES["c"][0][1] >= 128 and NT["c"] >= 128 and NT["c"] % 128 and tr.WGRAD_CASES["c"][0][1] % 128
    assert NT["a"] == 144 and tr.WGRAD_CASES["a"][0][1] % 64 and K["f"] == 3 < 8
    assert tr.WGRAD_CASES["h"][0][1] * NT["h"] < 65536 and tr.WGRAD_CASES["h"][7] == (32, 31)
    for n, c in tr.WGRAD_CASES.items():
        assert max(c[7]) <= K[n], n                                                      # the ABI's S <= B*P


# --------------------------------------------------------------------------- DFTs
def _dft_matrix(N):
    j = torch.arange(N, dtype=torch.float64)
    return torch.exp(-2j * math.pi * torch.outer(j, j) / N)


@pytest.mark.parametrize("shape", tr.DFT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dft_refs_are_the_dft_and_adjoint(shape):
    P, H, W = shape
    x, Z, r = tr.dft_inputs(P, H, W)
    if P > 3:
        x, Z, r = x[:3], Z[:3], r[:3]
    Wp = W // 2 + 1
    FH, FW = _dft_matrix(H), _dft_matrix(W)
    # forward: the DFT sums, kept to the half spectrum
    full = (FH @ x.double().to(torch.complex128) @ FW) / math.sqrt(H * W)
    for s in (1.0, 2.0):
        want = torch.where(tr.mirror_mask(W), full[..., :Wp] * s, full[..., :Wp])
        got = tr.rfft2_ref(x, s)
        assert _rel(torch.view_as_real(torch.complex(got[:, 0], got[:, 1])), torch.view_as_real(want)) <= 1e-12
    # inverse of unconstrained planes: complex inverse DFT down the columns, then the real part of the
    # half-spectrum row sum with the mirrored bins counted twice
    z = torch.complex(Z[:, 0].double(), Z[:, 1].double())
    cols = FH.conj() @ z
    wgt = torch.where(tr.mirror_mask(W), 2.0, 1.0)
    for s in (1.0, 0.5):
        sc = torch.where(tr.mirror_mask(W), s, 1.0)
        want = ((cols * (wgt * sc)) @ FW.conj()[:Wp]).real / math.sqrt(H * W)
        assert _rel(tr.irfft2_ref(Z, H, W, s), want) <= 1e-12
        assert _rel(tr.irfft2_ref(Z, H, W, s, r), want + r.double()) <= 1e-12
    # the adjoint identities the ops' backward passes rest on (odd W included)
    y = r
    assert tr.adjoint_gap(tr.rfft2_ref(x, 1.0), Z, x, tr.irfft2_ref(Z, H, W, 0.5)) <= 1e-13
    assert tr.adjoint_gap(tr.irfft2_ref(Z, H, W, 1.0), y, Z, tr.rfft2_ref(y, 2.0)) <= 1e-13
    if tr.mirror_mask(W).any():   # the scales the other way round are not adjoint, by >= 10x the GPU test's bound
        assert tr.adjoint_gap(tr.rfft2_ref(x, 1.0), Z, x, tr.irfft2_ref(Z, H, W, 2.0)) > 1e-4
        assert tr.adjoint_gap(tr.irfft2_ref(Z, H, W, 1.0), y, Z, tr.rfft2_ref(y, 0.5)) > 1e-4


# --------------------------------------------------------------------------- BatchNorm
def _bn_cases():
    for shape in tr.BN_SHAPES:
        for train in (True, False):
            yield shape, train, False
    yield (2, 16, 64), True, True


@pytest.mark.parametrize("shape,train,offset", list(_bn_cases()))
def test_bn_builder_is_kink_free_and_ref_is_batchnorm2d(shape, train, offset):
    for with_gamma in (True, False):
        inp = tr.bn_inputs(shape, train, offset, with_gamma)
        pre = tr.bn_pre(inp["x"], inp["gamma"], inp["beta"], train, inp["rmean"], inp["rvar"])
        assert pre.abs().min().item() >= tr.KINK           # every element, none left out
        assert inp["x"].dtype == torch.float32
        B, C, HW = shape
        bn = nn.BatchNorm2d(C, eps=tr.BN_EPS, affine=True).double().train(train)
        with torch.no_grad():
            bn.weight.copy_(inp["gamma"].double() if with_gamma else torch.ones(C, dtype=torch.float64))
            bn.bias.copy_(inp["beta"].double())
            bn.running_mean.copy_(inp["rmean"].double())
            bn.running_var.copy_(inp["rvar"].double())
        for act in tr.ACTS:
            x = inp["x"].double().reshape(B, C, HW, 1).requires_grad_(True)
            bn.zero_grad()
            y = tr.act64(bn(x), act)
            assert _rel(y.detach().reshape(B, C, HW), tr.act64(pre, act)) <= 1e-12
            y.backward(inp["dy"].double().reshape(B, C, HW, 1))
            dx, dg, db = tr.bn_ref(inp, act, train)
            # dx of train-mode BN is a difference of O(1) terms: its round-off is relative to |g|, not |dx|
            gmax = max(1.0, (inp["dy"].double().abs().max() / dx.abs().max().clamp_min(1e-300)).item())
            assert _rel(dx, x.grad.reshape(B, C, HW)) <= 1e-12 * gmax
            assert _rel(db, bn.bias.grad) <= 1e-12
            assert _rel(dg, bn.weight.grad) <= 1e-12     # without gamma: the gradient at gamma = 1
            if not train:
                assert _rel(tr.bn_ref_eval_dx(inp, act), dx) <= 1e-12
        scale, shift, moments = tr.bn_forward_consts(inp, train)
        z32 = inp["x"].double() * scale.double()[None, :, None] + shift.double()[None, :, None]
        assert (z32 - pre).abs().max().item() <= 1e-4     # float32 scale/shift: far inside the KINK margin
        assert (moments is not None) == train


# --------------------------------------------------------------------------- SE, small ops
@pytest.mark.parametrize("case", tr.SE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_se_builder_is_kink_free(case):
    x, dy, w1, w2 = tr.se_inputs(case)
    pre = tr.se_hidden_pre(x, w1)
    assert pre.numel() == case[0] * case[4]
    if pre.numel():
        assert pre.abs().min().item() >= tr.KINK
    y, dx, dw1, dw2 = tr.se_ref(x, dy, w1, w2)
    assert dx.shape == x.shape and dw1.shape == w1.shape and dw2.shape == w2.shape
    if case[4] == 0:
        assert _rel(y, 0.5 * x.double()) <= 1e-15 and _rel(dx, 0.5 * dy.double()) <= 1e-15


@pytest.mark.parametrize("act", tr.ACTS)
def test_act_bwd_builder_is_kink_free(act):
    pre, dy, t = tr.act_bwd_inputs(8192 * 256 + 3, act)
    assert pre.abs().min().item() >= tr.KINK
    assert torch.equal(t, pre) if act == 5 else t.dtype == torch.float32
    if act == 2:
        ref = tr.act_bwd_ref(pre, dy, act)
        assert torch.equal(ref, torch.where(pre > 0, dy.double(), tr.SLOPE * dy.double()))


def test_pool_up_refs_are_adjoint():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(5, 1, 6, 10, generator=gen)
    y = torch.randn(5, 1, 3, 5, generator=gen)
    for s in (0.25, 1.0, 0.3):
        assert tr.adjoint_gap(tr.pool2_ref(x, s), y, x, tr.up2_ref(y, s)) <= 1e-14
