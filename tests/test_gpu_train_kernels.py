"""Kernel-level parity of the training-path primitives (csrc/train_kernels.hip) on the GPU, each
against a float64 CPU reference of the same operation (tests/train_refs.py, itself checked in
test_train_refs_cpu.py), at the shapes where the kernels change path.  Metric: normwise error
(oracle.ffc_oracle.normwise_err) per returned tensor, bound 1e-5 for every family (exact-fp32 /
fp64-accumulating kernels and the fp32-accurate split-bf16 weight gradient); outputs are prefilled
with NaN so an element nobody wrote fails.

Observed maxima per family on the first MI355X run (normwise error; bound 1e-5 each):
  wgrad 2.8e-07   wgrad (FFC_WGRAD_KERNEL=old) 3.4e-07   DFTs 4.7e-07   DFT adjoint gap 9.8e-09
  bn_bwd 2.7e-06 (dgamma, offset data, Tanh; 9.5e-08 on dx in eval)   moments 2.2e-16 (relative)
  se 1.2e-06   act_bwd 1.1e-07   pool / up 8.2e-08   conv_full_smallm 6.9e-07

Case -> branch of train_kernels.hip it is there for
  wgrad a   S=1,3,16,17  wgradq vector gather (P=64), 64 tile with ragged Mu=24 / NT=144, K8=16 so S=17
                         leaves one split empty; S>1 -> split_sum_kernel (S < 32)
  wgrad b   S=1,2,5      wgradq scalar gather (P=25), K tail of the last chunk (K=75), stride 2, pad taps
  wgrad c   S=1,2,4      128 tile, Mu=130 and NT=144 ragged (second tile row / column nearly empty)
  wgrad d   S=1,4        dilation 2 with pad 2 (taps out of range), P=36 scalar
  wgrad e   S=1,3        stride 2 on an odd non-square plane (9x7 -> 4x3), P=12
  wgrad f   S=1          P=1, K=3 < one 8-k group (SE fc.0 / fc.2), both operand orders
  wgrad g   S=1,5        P=1 with a 4x4 V plane (the critic's full-plane conv), one sample per split
  wgrad h   S=32 / 31    split_sum_grouped_kernel (S >= 32, n=3456 < 65536) against split_sum_kernel
  accumulate             a, b at S=1 (workspace + split sum with S=1) and S=3: dW += sum
  FFC_WGRAD_KERNEL=old   wgrad_kernel<64,64,true> (a, b, d, e) and <128,32,true> (c), every S
  conv_wgrad a-c         wgrad_splits' own S through the ABI's S <= B*P check
  dft (5,4,4) .. (3,5,7) rfft2_kernel / irfft2_kernel: non-square, non-power-of-two, odd W, H=1
  dft (70,4,4)           NPW=64: second workgroup has np=6 < NPW
  dft 64x48, 48x64       NPW=1, direct DFT at its largest non-square planes
  dft (3,8,8)            forward on the line FFT (H >= 8), inverse on the direct DFT (H < 16)
  dft 16..128 square     line FFTs both ways
  scales 2.0 / 0.5, addend   the backward passes' options; the adjoint test pins ops.py's choice
  bn (3,5,7) (6,8,1)     odd sizes, HW=1; S in {1, 3, ffc_reduce_splits}
  bn (4,3,1024)          ffc_reduce_splits > 1
  bn (1,300,9)           C > 256: second workgroup of the coeff / final / sums kernels
  bn eval                running statistics, k1 = k2 = 0; gamma / dx nullptr; activation codes 0..5
  bn offset              mean / sigma = 20: cancellation in k1 * x + k2
  bn syncbn              _sums -> _coeff -> _apply bit-identical to the fused call
  se cases               float4 / scalar planes, P % 4 != 0, C > 256, hidden 0 / 32, odd H with HW % 4 == 0
  act_bwd n              1, 255, 257 (one ragged workgroup), 8192*256+3 (grid-stride tail)
  full_smallm            K % 4 != 0 scalar path, two segments (float4 + scalar), M = 1..4, bias, act
"""
import functools
import math
import os

import pytest
import torch

import train_refs as tr
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-5
NAN = float("nan")

def _lib():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    from fastfourierconvolution_amd._lib import check
    check(status, what)


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _err(family, what, out, ref):
    """print, then return, the normwise error of a returned tensor (which must hold no NaN)"""
    assert not torch.isnan(out).any(), f"{what}: unwritten (NaN) elements"
    e = normwise_err(out.detach().cpu().double().reshape(ref.shape), ref)
    print(f"OBS {family} {what} {e:.3e}")
    return e


# --------------------------------------------------------------------------- weight gradient
_wgrad_ref = functools.lru_cache(maxsize=None)(tr.wgrad_ref)


def _wgrad_abi(name, S, accumulate=0, prefill=None, old=False):
    U, V, _ = _wgrad_ref(name)
    _, _, k, s, p, d, _, _ = tr.WGRAD_CASES[name]
    B, Mu, PH, PW = U.shape
    _, Nv, VH, VW = V.shape
    Ud, Vd = U.to(DEV), V.to(DEV)
    ws = _nan((S * Mu * Nv * k * k,))
    dW = prefill.to(DEV).clone() if accumulate else _nan((Mu, Nv, k, k))
    L = _lib()
    prev = os.environ.get("FFC_WGRAD_KERNEL")
    if old:
        os.environ["FFC_WGRAD_KERNEL"] = "old"
    else:
        os.environ.pop("FFC_WGRAD_KERNEL", None)
    try:
        rc = L.ffc_conv_wgrad(_ptr(Ud), Mu, PH, PW, _ptr(Vd), Nv, VH, VW, B, k, s, p, d, S, _ptr(ws), _ptr(dW),
                              accumulate, _stream())
    finally:
        if prev is None:
            os.environ.pop("FFC_WGRAD_KERNEL", None)
        else:
            os.environ["FFC_WGRAD_KERNEL"] = prev
    _ok(rc, "ffc_conv_wgrad")
    torch.cuda.synchronize()
    return dW


_WGRAD_RUNS = [(n, S) for n, c in tr.WGRAD_CASES.items() for S in c[7]]


@pytest.mark.parametrize("name,S", _WGRAD_RUNS, ids=[f"{n}-S{S}" for n, S in _WGRAD_RUNS])
def test_wgrad_matches_fp64(name, S):
    ref = _wgrad_ref(name)[2]
    assert _err("wgrad", f"{name} S={S}", _wgrad_abi(name, S), ref) <= TOL


def test_wgrad_split_sum_kernels_agree():
    """case h: S=32 sums on split_sum_grouped_kernel, S=31 on split_sum_kernel"""
    c = tr.WGRAD_CASES["h"]
    assert c[0][1] * c[1][1] * c[2] ** 2 < 65536
    d32, d31 = _wgrad_abi("h", 32), _wgrad_abi("h", 31)
    assert _err("wgrad", "h S=32 against S=31", d32, d31.cpu().double()) <= TOL


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("S", [1, 3])
def test_wgrad_accumulate(name, S):
    ref = _wgrad_ref(name)[2]
    pre = torch.randn(ref.shape, generator=torch.Generator().manual_seed(77 + S))
    out = _wgrad_abi(name, S, accumulate=1, prefill=pre)
    assert _err("wgrad", f"{name} S={S} accumulate", out, pre.double() + ref) <= TOL


_OLD_RUNS = [(n, S) for n in "abcde" for S in tr.WGRAD_CASES[n][7]]


@pytest.mark.parametrize("name,S", _OLD_RUNS, ids=[f"{n}-S{S}" for n, S in _OLD_RUNS])
def test_wgrad_old_kernel_matches_fp64(name, S):
    """FFC_WGRAD_KERNEL=old (read on every call): the split-per-use wgrad_kernel variants"""
    ref = _wgrad_ref(name)[2]
    assert _err("wgrad_old", f"{name} S={S}", _wgrad_abi(name, S, old=True), ref) <= TOL


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_wgrad_wrapper_split_choice(name):
    """_autograd.conv_wgrad: the split count wgrad_splits picks is accepted by the ABI, same answer"""
    from fastfourierconvolution_amd import _autograd as ag
    U, V, ref = _wgrad_ref(name)
    _, _, k, s, p, d, _, _ = tr.WGRAD_CASES[name]
    out = ag.conv_wgrad(U.to(DEV), V.to(DEV), k, s, p, d, tuple(ref.shape))
    torch.cuda.synchronize()
    assert _err("wgrad", f"{name} conv_wgrad", out, ref) <= TOL


def test_wgrad_repeatable():
    """fixed-order split sum: a second launch is bit-identical"""
    assert torch.equal(_wgrad_abi("a", 3), _wgrad_abi("a", 3))


# --------------------------------------------------------------------------- planar DFTs
_dft_inputs = functools.lru_cache(maxsize=None)(tr.dft_inputs)


@functools.lru_cache(maxsize=None)
def _rfft(shape, scale):
    P, H, W = shape
    x = _dft_inputs(*shape)[0].to(DEV)
    Z = _nan((P, 2, H, W // 2 + 1))
    _ok(_lib().ffc_rfft2_planes(_ptr(x), P, H, W, scale, _ptr(Z), _stream()), "ffc_rfft2_planes")
    torch.cuda.synchronize()
    return Z.cpu()


@functools.lru_cache(maxsize=None)
def _irfft(shape, scale, with_addend):
    """irfft of the case's Z planes (the addend is the case's r)"""
    P, H, W = shape
    _, Z, r = _dft_inputs(*shape)
    Zd = Z.to(DEV)
    rd = r.to(DEV) if with_addend else None
    y = _nan((P, H, W))
    _ok(_lib().ffc_irfft2_planes(_ptr(Zd), P, H, W, scale, _ptr(rd), _ptr(y), _stream()), "ffc_irfft2_planes")
    torch.cuda.synchronize()
    return y.cpu()


def _rfft_of(t, shape, scale):
    P, H, W = shape
    td = t.to(DEV)
    Z = _nan((P, 2, H, W // 2 + 1))
    _ok(_lib().ffc_rfft2_planes(_ptr(td), P, H, W, scale, _ptr(Z), _stream()), "ffc_rfft2_planes")
    torch.cuda.synchronize()
    return Z.cpu()


_DFT_IDS = ["x".join(map(str, s)) for s in tr.DFT_SHAPES]


@pytest.mark.parametrize("shape", tr.DFT_SHAPES, ids=_DFT_IDS)
@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_rfft2_matches_fp64(shape, scale):
    x = _dft_inputs(*shape)[0]
    assert _err("dft", f"rfft {shape} x{scale}", _rfft(shape, scale), tr.rfft2_ref(x, scale)) <= TOL


@pytest.mark.parametrize("shape", tr.DFT_SHAPES, ids=_DFT_IDS)
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("with_addend", [False, True])
def test_irfft2_matches_fp64(shape, scale, with_addend):
    P, H, W = shape
    _, Z, r = _dft_inputs(*shape)
    ref = tr.irfft2_ref(Z, H, W, scale, r if with_addend else None)
    assert _err("dft", f"irfft {shape} x{scale} addend={with_addend}", _irfft(shape, scale, with_addend),
                ref) <= TOL


@pytest.mark.parametrize("shape", tr.DFT_SHAPES, ids=_DFT_IDS)
def test_dft_adjoint_identity(shape):
    """<rfft2(x, 1), Z> = <x, irfft2(Z, 0.5)> and <irfft2(Z, 1), y> = <Z, rfft2(y, 2)>: the mirror scales
    ops.py hands the backward passes (irfft2 at 0.5 is the adjoint of rfft2, rfft2 at 2 that of irfft2).
    Bound: train_refs.adjoint_gap with the kernels' 1e-5 (see its docstring)."""
    P, H, W = shape
    x, Z, y = _dft_inputs(*shape)
    g1 = tr.adjoint_gap(_rfft(shape, 1.0), Z, x, _irfft(shape, 0.5, False))
    g2 = tr.adjoint_gap(_irfft(shape, 1.0, False), y, Z, _rfft_of(y, shape, 2.0))
    print(f"OBS dft_adjoint {shape} {g1:.3e} {g2:.3e}")
    assert g1 <= TOL and g2 <= TOL


@pytest.mark.parametrize("shape", [(3, 6, 10), (3, 8, 8), (2, 16, 16)], ids=["3x6x10", "3x8x8", "2x16x16"])
def test_dft_ops_backward_is_the_adjoint(shape):
    """torch.ops.ffc.rfft2 / irfft2 backward (ops.py's scales) against the float64 adjoints"""
    _lib()
    P, H, W = shape
    x, Z, y = _dft_inputs(*shape)
    xd = x.to(DEV).reshape(1, P, H, W).requires_grad_(True)
    torch.ops.ffc.rfft2(xd, 1.0).backward(Z.to(DEV).reshape(1, 2 * P, H, W // 2 + 1))
    assert _err("dft", f"rfft2 backward {shape}", xd.grad, tr.irfft2_ref(Z, H, W, 0.5).reshape(1, P, H, W)) <= TOL
    Zd = Z.to(DEV).reshape(1, 2 * P, H, W // 2 + 1).requires_grad_(True)
    rd = y.to(DEV).reshape(1, P, H, W).requires_grad_(True)
    dy = x.to(DEV).reshape(1, P, H, W)
    torch.ops.ffc.irfft2(Zd, H, W, 1.0, rd).backward(dy)
    assert _err("dft", f"irfft2 backward {shape}", Zd.grad,
                tr.rfft2_ref(x, 2.0).reshape(1, 2 * P, H, W // 2 + 1)) <= TOL
    assert torch.equal(rd.grad, dy)


def test_dft_rejections():
    from fastfourierconvolution_amd import _autograd as ag
    from fastfourierconvolution_amd._lib import FFCError
    L = _lib()
    for H, W in ((128, 96), (65, 65)):
        with pytest.raises(FFCError):
            ag.rfft2_impl(torch.zeros(1, 1, H, W, device=DEV), 1.0)
        with pytest.raises(FFCError):
            ag.irfft2_impl(torch.zeros(1, 2, H, W // 2 + 1, device=DEV), H, W, 1.0, None)
    x, Z = torch.zeros(4, device=DEV), torch.zeros(8, device=DEV)
    assert L.ffc_rfft2_planes(_ptr(x), 1, 4, 1, 1.0, _ptr(Z), _stream()) != 0
    assert L.ffc_irfft2_planes(_ptr(Z), 1, 4, 1, 1.0, None, _ptr(x), _stream()) != 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- BatchNorm backward, moments
def _splits(shape):
    B, C, HW = shape
    return sorted({1, 3, _lib().ffc_reduce_splits(B, C, HW)})


def _bn_bufs(C, S, x, want_dx):
    return dict(ws=_nan((S * C * 2,), torch.float64), coef=_nan((3 * C,)), dgamma=_nan((C,)), dbeta=_nan((C,)),
                dx=_nan(tuple(x.shape)) if want_dx else None)


def _bn_dev(inp, train):
    scale, shift, moments = tr.bn_forward_consts(inp, train)
    d = {k: (v.to(DEV) if v is not None else None) for k, v in inp.items()}
    d.update(scale=scale.to(DEV), shift=shift.to(DEV), moments=moments.to(DEV) if moments is not None else None)
    return d


def _bn_fused(d, act, train, S, want_dx=True):
    B, C, HW = d["x"].shape
    o = _bn_bufs(C, S, d["x"], want_dx)
    rc = _lib().ffc_bn_bwd(_ptr(d["x"]), _ptr(d["dy"]), B, C, HW, _ptr(d["scale"]), _ptr(d["shift"]), act, tr.SLOPE,
                           _ptr(d["moments"]) if train else None, None if train else _ptr(d["rmean"]),
                           None if train else _ptr(d["rvar"]), tr.BN_EPS, _ptr(d["gamma"]), _ptr(o["ws"]), S,
                           _ptr(o["coef"]), _ptr(o["dgamma"]), _ptr(o["dbeta"]), _ptr(o["dx"]), _stream())
    _ok(rc, "ffc_bn_bwd")
    torch.cuda.synchronize()
    return o


def _bn_check(shape, train, offset=False, acts=tr.ACTS):
    worst = 0.0
    for with_gamma in (True, False):
        inp = tr.bn_inputs(shape, train, offset, with_gamma)
        d = _bn_dev(inp, train)
        for act in acts:
            dx, dg, db = tr.bn_ref(inp, act, train)
            if not train:
                assert normwise_err(tr.bn_ref_eval_dx(inp, act), dx) <= 1e-12
            tag = f"{shape} train={train} offset={offset} gamma={with_gamma} act={act}"
            first = None
            for S in _splits(shape):
                o = _bn_fused(d, act, train, S)
                errs = (_err("bn_bwd", f"dx {tag} S={S}", o["dx"], dx),
                        _err("bn_bwd", f"dgamma {tag} S={S}", o["dgamma"], dg),
                        _err("bn_bwd", f"dbeta {tag} S={S}", o["dbeta"], db))
                worst = max(worst, *errs)
                assert not torch.isnan(o["coef"]).any()
                if not train:
                    assert (o["coef"].reshape(-1, 3)[:, 1:] == 0).all()
                first = first or o
            nodx = _bn_fused(d, act, train, 1, want_dx=False)     # dx = nullptr: the sums alone, same bits
            assert torch.equal(nodx["dgamma"], first["dgamma"]) and torch.equal(nodx["dbeta"], first["dbeta"])
            assert torch.equal(nodx["coef"], first["coef"])
    return worst


@pytest.mark.parametrize("shape", tr.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("train", [True, False], ids=["batch", "running"])
def test_bn_bwd_matches_fp64(shape, train):
    assert _bn_check(shape, train) <= TOL


def test_bn_bwd_offset_data():
    """x = 20 + randn per channel (mean / sigma = 20): where dx = k0 g + (k1 x + k2) cancels"""
    assert _bn_check((2, 16, 64), True, offset=True) <= TOL


@pytest.mark.parametrize("shape", tr.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_bwd_syncbn_form_is_bit_identical(shape):
    """_sums -> _coeff -> _apply on one rank's own sums against the fused call at the same S"""
    L = _lib()
    B, C, HW = shape
    inp = tr.bn_inputs(shape, True)
    d = _bn_dev(inp, True)
    for act in (2, 5):
        for S in _splits(shape):
            f = _bn_fused(d, act, True, S)
            o = _bn_bufs(C, S, d["x"], True)
            sums = _nan((C, 2), torch.float64)
            _ok(L.ffc_bn_bwd_sums(_ptr(d["x"]), _ptr(d["dy"]), B, C, HW, _ptr(d["scale"]), _ptr(d["shift"]), act,
                                  tr.SLOPE, _ptr(o["ws"]), S, _ptr(sums), _stream()), "ffc_bn_bwd_sums")
            _ok(L.ffc_bn_bwd_coeff(_ptr(sums), C, _ptr(d["moments"]), tr.BN_EPS, _ptr(d["gamma"]), _ptr(o["coef"]),
                                   _ptr(o["dgamma"]), _ptr(o["dbeta"]), _stream()), "ffc_bn_bwd_coeff")
            _ok(L.ffc_bn_bwd_apply(_ptr(d["x"]), _ptr(d["dy"]), B, C, HW, _ptr(d["scale"]), _ptr(d["shift"]), act,
                                   tr.SLOPE, _ptr(o["coef"]), _ptr(o["dx"]), _stream()), "ffc_bn_bwd_apply")
            torch.cuda.synchronize()
            for k in ("coef", "dgamma", "dbeta", "dx"):
                assert not torch.isnan(o[k]).any(), k
                assert torch.equal(o[k], f[k]), (k, act, S)


@pytest.mark.parametrize("shape", tr.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_channel_moments_match_fp64(shape):
    """count exact; sum x and sum x^2 against the correctly rounded float64 sums (math.fsum) of the float32
    input (x * x is exact in float64), rtol 1e-12"""
    L = _lib()
    B, C, HW = shape
    x = tr.bn_inputs(shape, True)["x"]
    xd = x.to(DEV)
    cols = x.double().permute(1, 0, 2).reshape(C, -1)
    ref = torch.tensor([[float(B * HW), math.fsum(c.tolist()), math.fsum((c * c).tolist())] for c in cols],
                       dtype=torch.float64)
    for S in sorted({1, L.ffc_reduce_splits(B, C, HW)}):
        ws, mom = _nan((S * C * 2,), torch.float64), _nan((C, 3), torch.float64)
        _ok(L.ffc_channel_moments(_ptr(xd), B, C, HW, _ptr(ws), S, _ptr(mom), _stream()), "ffc_channel_moments")
        torch.cuda.synchronize()
        mom = mom.cpu()
        assert not torch.isnan(mom).any()
        rel = ((mom - ref).abs() / ref.abs()).max().item()
        print(f"OBS moments {shape} S={S} max rel {rel:.3e}")
        assert torch.equal(mom[:, 0], ref[:, 0])
        torch.testing.assert_close(mom[:, 1:], ref[:, 1:], rtol=1e-12, atol=0.0)


# --------------------------------------------------------------------------- SE backward
@pytest.mark.parametrize("case", tr.SE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_se_scale_and_backward_match_fp64(case):
    _lib()
    x, dy, w1, w2 = tr.se_inputs(case)
    y, dx, dw1, dw2 = tr.se_ref(x, dy, w1, w2)
    xd, a, b = (t.to(DEV).requires_grad_(True) for t in (x, w1, w2))
    out = torch.ops.ffc.se_scale(xd, a, b)
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    errs = [_err("se", f"{n} {case}", t, r) for n, t, r in
            (("y", out, y), ("dx", xd.grad, dx), ("dw1", a.grad, dw1), ("dw2", b.grad, dw2))]
    assert a.grad.shape == w1.shape and b.grad.shape == w2.shape
    assert max(errs) <= TOL, errs


# --------------------------------------------------------------------------- small ops
@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 3])
@pytest.mark.parametrize("act", [1, 2, 3, 4, 5])
def test_act_bwd_matches_fp64(n, act):
    pre, dy, t = tr.act_bwd_inputs(n, act)
    td, dyd, dx = t.to(DEV), dy.to(DEV), _nan((n,))
    _ok(_lib().ffc_act_bwd(_ptr(td), _ptr(dyd), _ptr(dx), n, act, tr.SLOPE, _stream()), "ffc_act_bwd")
    torch.cuda.synchronize()
    assert _err("act_bwd", f"n={n} act={act}", dx, tr.act_bwd_ref(pre, dy, act)) <= TOL


@pytest.mark.parametrize("P,H,W", [(3, 2, 2), (5, 6, 10), (2, 64, 2)])
@pytest.mark.parametrize("scale", [0.25, 1.0, 0.3])
def test_pool2_up2_match_fp64_and_are_adjoint(P, H, W, scale):
    L = _lib()
    gen = torch.Generator().manual_seed(6000 + P + H * W)
    x = torch.randn(P, 1, H, W, generator=gen)
    xd = x.to(DEV)
    pooled = _nan((P, 1, H // 2, W // 2))
    _ok(L.ffc_pool2(_ptr(xd), P, H, W, scale, _ptr(pooled), _stream()), "ffc_pool2")
    up = _nan((P, 1, 2 * H, 2 * W))
    _ok(L.ffc_up2(_ptr(xd), P, H, W, scale, _ptr(up), _stream()), "ffc_up2")
    y = torch.randn(P, 1, H // 2, W // 2, generator=gen)
    yd = y.to(DEV)
    upy = _nan((P, 1, H, W))
    _ok(L.ffc_up2(_ptr(yd), P, H // 2, W // 2, scale, _ptr(upy), _stream()), "ffc_up2")
    torch.cuda.synchronize()
    assert _err("pool_up", f"pool2 {(P, H, W)} x{scale}", pooled, tr.pool2_ref(x, scale)) <= TOL
    assert _err("pool_up", f"up2 {(P, H, W)} x{scale}", up, tr.up2_ref(x, scale)) <= TOL
    gap = tr.adjoint_gap(pooled.cpu(), y, x, upy.cpu())
    print(f"OBS pool_up adjoint {(P, H, W)} x{scale} {gap:.3e}")
    assert gap <= TOL


@pytest.mark.parametrize("K0", [48, 50, 8192])
def test_conv_full_smallm_matches_fp64(K0):
    L = _lib()
    B = 3
    gen = torch.Generator().manual_seed(7000 + K0)
    x0 = torch.randn(B, K0, generator=gen)
    worst = 0.0
    for M in (1, 2, 3, 4):
        w0 = torch.randn(M, K0, generator=gen) / K0 ** 0.5
        bias = torch.randn(M, generator=gen)
        for K1 in (0, 20, 18):
            x1 = torch.randn(B, K1, generator=gen) if K1 else None
            w1 = torch.randn(M, K1, generator=gen) / K1 ** 0.5 if K1 else None
            dev = [t.to(DEV) if t is not None else None for t in (x0, w0, x1, w1, bias)]
            for use_bias in (False, True):
                for act in (0, 2, 4):
                    out = _nan((B, M))
                    _ok(L.ffc_conv_full_smallm(_ptr(dev[0]), K0, _ptr(dev[1]), _ptr(dev[2]), K1, _ptr(dev[3]),
                                               _ptr(dev[4]) if use_bias else None, B, M, _ptr(out), act, tr.SLOPE,
                                               _stream()), "ffc_conv_full_smallm")
                    torch.cuda.synchronize()
                    ref = tr.full_smallm_ref(x0, w0, x1, w1, bias if use_bias else None, act)
                    worst = max(worst, _err("full_smallm", f"K0={K0} M={M} K1={K1} bias={use_bias} act={act}",
                                            out, ref))
    assert worst <= TOL
