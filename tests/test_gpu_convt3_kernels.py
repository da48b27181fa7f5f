"""Kernel-level parity of csrc/convt3_smallm.hip -- ffc_convt3x3_smallm (the small-M ConvTranspose2d k3 s1 p1
head) and ffc_convt3x3_smallm_dgrad (its data gradient) -- each called through the C ABI against the float64
references of baseline_refs.py, element by element under the project's kernel bound
|got - ref| <= 1e-5 (|ref| + rms(ref)).  test_baseline_cpu.py pins the references against float64 autograd
and shows PyTorch's fp32 result under a quarter of the bound on every input used here.

Outputs live inside NaN-filled allocations with guard floats on both sides: every element in range must be
written and nothing outside it.  Also: bit-equality of two runs, the scalar path taken for misaligned
pointers at W % 4 == 0, agreement with the implicit-GEMM route on the same job (USE_SMALLM off) under the
same bound, and every rejection of the argument checks (nothing is launched: the outputs stay NaN).
"""
import pytest
import torch
import torch.nn as nn

import baseline_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN = float("nan")
GUARD = 64
E_INVALID = -1


def _L():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    from fastfourierconvolution_amd._lib import check
    check(status, what)


@pytest.fixture(autouse=True)
def _sync_after():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is launched from this file
        pytest.exit(f"HIP error after a kernel of this file: {e}", returncode=3)


class _Buf:
    """n floats inside a NaN-filled allocation: GUARD floats in front (one more with ``mis``: the data then
    starts one float off 16-byte alignment) and GUARD behind"""

    def __init__(self, n, mis=False, fill=None):
        self.n, self.off = n, GUARD + (1 if mis else 0)
        self.buf = torch.full((self.off + n + GUARD,), NAN, device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        if fill is not None:
            self.buf[self.off:self.off + n] = fill.to(DEV).reshape(-1).float()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def get(self, what, shape):
        torch.cuda.synchronize()
        data = self.buf.cpu()
        inside = data[self.off:self.off + self.n]
        assert bool(torch.isfinite(inside).all()), f"{what}: unwritten or non-finite elements in range"
        assert int(torch.isnan(data).sum()) == data.numel() - self.n, f"{what}: wrote outside its range"
        return inside.reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())


_REFS = {}


def _case(name):
    """inputs and float64 references of a case, computed once"""
    if name not in _REFS:
        B, C, M, H, W, _, act, _ = R.CASES[name]
        x, w, bias, dpre = R.inputs(name)
        _REFS[name] = dict(x=x, w=w, bias=bias, dpre=dpre, act=act, dims=(B, C, M, H, W),
                           ref=R.head_ref(x, w, bias, act), dref=R.dgrad_ref(dpre, w))
    return _REFS[name]


def _forward(c, mis=False, act=None):
    B, C, M, H, W = c["dims"]
    x, w = _Buf(c["x"].numel(), mis, c["x"]), _Buf(c["w"].numel(), fill=c["w"])
    bias = _Buf(M, fill=c["bias"]) if c["bias"] is not None else None
    out = _Buf(B * M * H * W, mis)
    _ok(_L().ffc_convt3x3_smallm(x.ptr(), C, w.ptr(), bias.ptr() if bias else None, B, H, W, M, out.ptr(),
                                 c["act"] if act is None else act, 0.0, _stream()), "ffc_convt3x3_smallm")
    return out.get("out", (B, M, H, W))


def _dgrad(c, mis=False):
    B, C, M, H, W = c["dims"]
    g, w = _Buf(c["dpre"].numel(), mis, c["dpre"]), _Buf(c["w"].numel(), fill=c["w"])
    dx = _Buf(B * C * H * W, mis)
    _ok(_L().ffc_convt3x3_smallm_dgrad(g.ptr(), w.ptr(), B, C, H, W, M, dx.ptr(), _stream()),
        "ffc_convt3x3_smallm_dgrad")
    return dx.get("dx", (B, C, H, W))


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_against_float64(name):
    c = _case(name)
    got = _forward(c)
    share = R.worst(got, c["ref"])
    print(f"{name}: forward worst share of the bound {share:.3f}")
    assert share <= 1.0
    assert torch.equal(got, _forward(c)), "two runs differ"


@pytest.mark.parametrize("name", list(R.CASES))
def test_dgrad_against_float64(name):
    c = _case(name)
    got = _dgrad(c)
    share = R.worst(got, c["dref"])
    print(f"{name}: dgrad worst share of the bound {share:.3f}")
    assert share <= 1.0
    assert torch.equal(got, _dgrad(c)), "two runs differ"


@pytest.mark.parametrize("name", ["c64_m3_8x8", "c64_m4_24x24_b3", "c3_m1_5x72_b3"])
def test_misaligned_pointers_take_the_scalar_path(name):
    """W % 4 == 0 with x / out (dpre / dx) one float off 16-byte alignment: same bound, no float4 access"""
    c = _case(name)
    assert R.worst(_forward(c, mis=True), c["ref"]) <= 1.0
    assert R.worst(_dgrad(c, mis=True), c["dref"]) <= 1.0


@pytest.mark.parametrize("act", [R.IDENT, R.TANH])
@pytest.mark.parametrize("with_bias", [True, False])
def test_bias_and_activation_combinations(act, with_bias):
    c = dict(_case("c64_m3_8x8"))
    if not with_bias:
        c["bias"] = None
    ref = R.head_ref(c["x"], c["w"], c["bias"], act)
    assert R.worst(_forward(c, act=act), ref) <= 1.0


@pytest.mark.parametrize("name", ["c64_m3_8x8", "c64_m4_24x24_b3", "cap_m3_33x7"])
def test_matches_the_implicit_gemm_route(name, monkeypatch):
    """the same ffc::conv_layer job forward and backward with USE_SMALLM on (the direct kernels) and off (the
    implicit-GEMM kernels): both under the bound against float64, so within twice the bound of each other"""
    from fastfourierconvolution_amd import _autograd as ag
    from fastfourierconvolution_amd import _runtime as rt
    c = _case(name)
    B, C, M, H, W = c["dims"]
    conv = nn.ConvTranspose2d(C, M, 3, stride=1, padding=1, bias=c["bias"] is not None).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
        if c["bias"] is not None:
            conv.bias.copy_(c["bias"])
    res = {}
    for on in (True, False):
        monkeypatch.setattr(rt, "USE_SMALLM", on)
        x = c["x"].to(DEV).requires_grad_(True)
        sg = rt.conv_seg(conv, x)
        w = [rt.conv_weight(conv)]
        assert rt.conv_route([sg], w, M, False, False, rt.TRAIN_ROUTES, training=True) == ("convT3" if on else None)
        (y,) = ag.conv_layer(B, [(M, 0, 0.0)], [(0, 0, sg, conv)], [x])
        (gx,) = torch.autograd.grad(y, x, c["dpre"].to(DEV))
        res[on] = (y.detach().cpu(), gx.cpu())
    ref = R.head_ref(c["x"], c["w"], c["bias"], R.IDENT)
    for on in (True, False):
        sy, sg_ = R.worst(res[on][0], ref), R.worst(res[on][1], c["dref"])
        print(f"{name} USE_SMALLM={on}: forward {sy:.3f} dgrad {sg_:.3f} of the bound")
        assert sy <= 1.0 and sg_ <= 1.0


def test_rejections_launch_nothing():
    """M > 4, M < 1, C over the cap, null pointers, B = 0 (and non-positive C, H, W): FFC_E_INVALID with a
    message, outputs untouched"""
    L = _L()
    x, w, b = _Buf(4 * 64, fill=torch.zeros(256)), _Buf(9 * 260 * 5, fill=torch.zeros(9 * 260 * 5)), _Buf(8, fill=torch.zeros(8))
    out = _Buf(4096)
    s = _stream()
    fwd = lambda xp, C, wp, B, H, W, M, op: L.ffc_convt3x3_smallm(xp, C, wp, b.ptr(), B, H, W, M, op, 0, 0.0, s)  # noqa: E731
    bwd = lambda gp, wp, B, C, H, W, M, dp: L.ffc_convt3x3_smallm_dgrad(gp, wp, B, C, H, W, M, dp, s)  # noqa: E731
    bad = [
        ("1 <= M <= 4", fwd(x.ptr(), 4, w.ptr(), 1, 4, 4, 5, out.ptr())),
        ("1 <= M <= 4", fwd(x.ptr(), 4, w.ptr(), 1, 4, 4, 0, out.ptr())),
        ("at most 256", fwd(x.ptr(), 257, w.ptr(), 1, 1, 1, 3, out.ptr())),
        ("null pointer", fwd(None, 4, w.ptr(), 1, 4, 4, 3, out.ptr())),
        ("null pointer", fwd(x.ptr(), 4, None, 1, 4, 4, 3, out.ptr())),
        ("null pointer", fwd(x.ptr(), 4, w.ptr(), 1, 4, 4, 3, None)),
        ("must be positive", fwd(x.ptr(), 4, w.ptr(), 0, 4, 4, 3, out.ptr())),
        ("must be positive", fwd(x.ptr(), 0, w.ptr(), 1, 4, 4, 3, out.ptr())),
        ("must be positive", fwd(x.ptr(), 4, w.ptr(), 1, 0, 4, 3, out.ptr())),
        ("must be positive", fwd(x.ptr(), 4, w.ptr(), 1, 4, -1, 3, out.ptr())),
        ("1 <= M <= 4", bwd(x.ptr(), w.ptr(), 1, 4, 4, 4, 5, out.ptr())),
        ("at most 256", bwd(x.ptr(), w.ptr(), 1, 257, 1, 1, 3, out.ptr())),
        ("null pointer", bwd(None, w.ptr(), 1, 4, 4, 4, 3, out.ptr())),
        ("null pointer", bwd(x.ptr(), None, 1, 4, 4, 4, 3, out.ptr())),
        ("null pointer", bwd(x.ptr(), w.ptr(), 1, 4, 4, 4, 3, None)),
        ("must be positive", bwd(x.ptr(), w.ptr(), 0, 4, 4, 4, 3, out.ptr())),
    ]
    for want, status in bad:
        assert status == E_INVALID, want
    # the message of the last refusal names the entry point and the reason
    assert L.ffc_convt3x3_smallm(x.ptr(), 4, w.ptr(), None, 1, 4, 4, 5, out.ptr(), 0, 0.0, s) == E_INVALID
    msg = L.ffc_last_error().decode()
    assert "ffc_convt3x3_smallm" in msg and "1 <= M <= 4" in msg
    assert L.ffc_convt3x3_smallm_dgrad(x.ptr(), w.ptr(), 1, 300, 4, 4, 3, out.ptr(), s) == E_INVALID
    msg = L.ffc_last_error().decode()
    assert "ffc_convt3x3_smallm_dgrad" in msg and "at most 256" in msg
    assert out.untouched()
