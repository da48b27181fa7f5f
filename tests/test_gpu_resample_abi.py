"""The resampling kernels through the C ABI (include/ffc_amd.h: ffc_act_up2b, ffc_up2b_adjoint, ffc_pool2_act,
ffc_relu_sum_pool and the two backwards) with raw pointers into the NaN-guarded buffers of tests/abi_bufs.py,
compared elementwise with the fp64 restatements of tests/resnet_refs.py.

Bound: |got - ref| <= TOL * (the fp64 sum of the element's absolute terms), TOL = 1e-6 fixed by
tests/test_resnet_cpu.py::test_tol_rule on the CPU (the plain fp32 restatement's worst share is 0.198; every planted
defect exceeds 1).  Every test prints its largest share.  Buffers come both 16-byte aligned and one float off."""
import pytest
import torch

import abi_bufs as A
import resnet_refs as R
from abi_bufs import Buf

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _end():
    yield
    A.end_of_test()


def _check(name, got, ref, scale, worst):
    s = R.share(got.reshape(ref.shape), ref, scale)
    worst[0] = max(worst[0], s)
    assert s <= 1.0, (name, s)


@pytest.mark.parametrize("B,C", R.BCS)
@pytest.mark.parametrize("h,w", R.PLANES)
def test_act_up2b(h, w, B, C):
    L, st = A.lib(), A.stream()
    d = R.inputs(h, w, B, C)
    worst = [0.0]
    for mis in (False, True):
        x = Buf(d["x"].numel(), mis, d["x"])
        for form in R.SCALE_FORMS:
            sc, sh = R.scale_shift(d, form)
            bs = Buf(sc.numel(), mis, sc) if sc is not None else None
            bt = Buf(sh.numel(), mis, sh) if sh is not None else None
            for act in R.ACTS:
                y = Buf(4 * d["x"].numel(), mis)
                A.ok(L.ffc_act_up2b(x.ptr(), bs.ptr() if bs else None, bt.ptr() if bt else None,
                                    1 if form == "sample" else 0, B, C, h, w, act, 0.0, y.ptr(), st), "ffc_act_up2b")
                ref, scale = R.act_up2b(d["x"], sc, sh, act)
                _check(f"{form}/{act}/mis={mis}", y.get("y"), ref, scale, worst)
    print(f"OBS act_up2b {h}x{w} B*C={B * C}: worst share {worst[0]:.3f}")


@pytest.mark.parametrize("B,C", R.BCS)
@pytest.mark.parametrize("h,w", R.PLANES)
def test_up2b_adjoint(h, w, B, C):
    """against the fp64 adjoint, and <up(x), g> = <x, up^T(g)> with the kernel's own forward"""
    L, st = A.lib(), A.stream()
    d = R.inputs(h, w, B, C, seed=1)
    worst = [0.0]
    for mis in (False, True):
        g = Buf(d["dy"].numel(), mis, d["dy"])
        dx = Buf(d["x"].numel(), mis)
        A.ok(L.ffc_up2b_adjoint(g.ptr(), B * C, h, w, dx.ptr(), st), "ffc_up2b_adjoint")
        ref, scale = R.up2b_adjoint(d["dy"])
        got = dx.get("dx")
        _check(f"adjoint/mis={mis}", got, ref, scale, worst)
        x = Buf(d["x"].numel(), mis, d["x"])
        y = Buf(d["dy"].numel(), mis)
        A.ok(L.ffc_act_up2b(x.ptr(), None, None, 0, B, C, h, w, 0, 0.0, y.ptr(), st), "ffc_act_up2b")
        lhs = float((y.get("y").double() * d["dy"].double().reshape(-1)).sum())
        rhs = float((d["x"].double().reshape(-1) * got.double()).sum())
        mag = float((R.act_up2b(d["x"].abs())[0] * d["dy"].abs().double()).sum())
        assert abs(lhs - rhs) <= 2 * R.TOL * mag, (lhs, rhs, mag)
    print(f"OBS up2b_adjoint {h}x{w} B*C={B * C}: worst share {worst[0]:.3f}")


@pytest.mark.parametrize("B,C", R.BCS)
@pytest.mark.parametrize("h,w", R.PLANES)
def test_pool2_act_and_backward(h, w, B, C):
    """on the (2h, 2w) plane; the backward is exact (a product with 0.25 and a 0 / 1 mask)"""
    L, st = A.lib(), A.stream()
    d = R.inputs(h, w, B, C, seed=2)
    worst = [0.0]
    for mis in (False, True):
        x = Buf(d["dy"].numel(), mis, d["dy"])
        for act in R.ACTS:
            y = Buf(d["x"].numel(), mis)
            A.ok(L.ffc_pool2_act(x.ptr(), B * C, 2 * h, 2 * w, act, 0.0, y.ptr(), st), "ffc_pool2_act")
            ref, scale = R.pool2_act(d["dy"], act)
            got = y.get("y")
            _check(f"pool2_act/{act}/mis={mis}", got, ref, scale, worst)
            g = Buf(d["dlow"].numel(), mis, d["dlow"])
            dx = Buf(d["dy"].numel(), mis)
            A.ok(L.ffc_pool2_act_bwd(y.ptr(), g.ptr(), B * C, h, w, act, 0.0, dx.ptr(), st), "ffc_pool2_act_bwd")
            bref, _ = R.pool2_act_bwd(got.reshape(d["x"].shape), d["dlow"], act)   # the mask of the kernel's own y
            assert torch.equal(dx.get("dx").double(), bref.reshape(-1))
    print(f"OBS pool2_act {2 * h}x{2 * w} B*C={B * C}: worst share {worst[0]:.3f}")


@pytest.mark.parametrize("B,C", R.BCS)
@pytest.mark.parametrize("h,w", R.PLANES)
def test_relu_sum_pool_and_backward(h, w, B, C):
    L, st = A.lib(), A.stream()
    d = R.inputs(h, w, B, C, seed=3)
    worst = [0.0]
    for mis in (False, True):
        for x0 in (d["x"], -d["x"].abs() - 0.5):   # the second: all-negative planes, exact 0
            x = Buf(x0.numel(), mis, x0)
            out = Buf(B * C, mis)
            A.ok(L.ffc_relu_sum_pool(x.ptr(), B * C, h * w, out.ptr(), st), "ffc_relu_sum_pool")
            ref, scale = R.relu_sum_pool(x0)
            got = out.get("out")
            _check(f"relu_sum/mis={mis}", got, ref, scale, worst)
            if x0 is not d["x"]:
                assert not bool(got.any())
            g = Buf(B * C, mis, d["dout"])
            dx = Buf(x0.numel(), mis)
            A.ok(L.ffc_relu_sum_pool_bwd(x.ptr(), g.ptr(), B * C, h * w, dx.ptr(), st), "ffc_relu_sum_pool_bwd")
            assert torch.equal(dx.get("dx").double(), R.relu_sum_pool_bwd(x0, d["dout"])[0].reshape(-1))
    print(f"OBS relu_sum_pool {h}x{w} B*C={B * C}: worst share {worst[0]:.3f}")


def test_two_runs_are_bit_equal():
    L, st = A.lib(), A.stream()
    d = R.inputs(16, 16, 2, 65, seed=4)
    runs = []
    for _ in range(2):
        x, g = Buf(d["x"].numel(), False, d["x"]), Buf(d["dy"].numel(), False, d["dy"])
        s, t = Buf(65, False, d["scale_c"]), Buf(65, False, d["shift_c"])
        y, dx, o = Buf(d["dy"].numel()), Buf(d["x"].numel()), Buf(130)
        A.ok(L.ffc_act_up2b(x.ptr(), s.ptr(), t.ptr(), 0, 2, 65, 16, 16, 1, 0.0, y.ptr(), st), "ffc_act_up2b")
        A.ok(L.ffc_up2b_adjoint(g.ptr(), 130, 16, 16, dx.ptr(), st), "ffc_up2b_adjoint")
        A.ok(L.ffc_relu_sum_pool(x.ptr(), 130, 256, o.ptr(), st), "ffc_relu_sum_pool")
        runs.append((y.get("y"), dx.get("dx"), o.get("out")))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_argument_rejections_launch_nothing():
    L, st = A.lib(), A.stream()
    x, y = Buf(16, False, torch.ones(16)), Buf(64)
    p, q = x.ptr(), y.ptr()
    cases = [
        (L.ffc_act_up2b(None, None, None, 0, 1, 1, 4, 4, 0, 0.0, q, st), "ffc_act_up2b", "null"),
        (L.ffc_act_up2b(p, None, None, 0, 1, 1, 4, 4, 0, 0.0, None, st), "ffc_act_up2b", "null"),
        (L.ffc_act_up2b(p, p, None, 0, 1, 1, 4, 4, 0, 0.0, q, st), "ffc_act_up2b", "together"),
        (L.ffc_act_up2b(p, None, None, 0, 1, 1, 0, 4, 0, 0.0, q, st), "ffc_act_up2b", "shape"),
        (L.ffc_act_up2b(p, None, None, 0, 1, 1, 4, -1, 0, 0.0, q, st), "ffc_act_up2b", "shape"),
        (L.ffc_act_up2b(p, None, None, 0, 1, 1, 4, 4, 9, 0.0, q, st), "ffc_act_up2b", "activation"),
        (L.ffc_act_up2b(p, None, None, 0, 1 << 15, 1 << 15, 1, 1, 0, 0.0, q, st), "ffc_act_up2b", "32-bit"),
        (L.ffc_up2b_adjoint(None, 1, 2, 2, p, st), "ffc_up2b_adjoint", "null"),
        (L.ffc_up2b_adjoint(q, 1, 2, 2, None, st), "ffc_up2b_adjoint", "null"),
        (L.ffc_up2b_adjoint(q, 0, 2, 2, p, st), "ffc_up2b_adjoint", "shape"),
        (L.ffc_up2b_adjoint(q, 1, 2, 0, p, st), "ffc_up2b_adjoint", "shape"),
        (L.ffc_up2b_adjoint(q, 1 << 20, 1 << 10, 1 << 10, p, st), "ffc_up2b_adjoint", "32-bit"),
        (L.ffc_pool2_act(None, 1, 4, 4, 1, 0.0, q, st), "ffc_pool2_act", "null"),
        (L.ffc_pool2_act(p, 1, 3, 4, 1, 0.0, q, st), "ffc_pool2_act", "odd"),
        (L.ffc_pool2_act(p, 1, 4, 3, 1, 0.0, q, st), "ffc_pool2_act", "odd"),
        (L.ffc_pool2_act(p, 1, 0, 4, 1, 0.0, q, st), "ffc_pool2_act", "shape"),
        (L.ffc_pool2_act(p, 1, 4, 4, 5, 0.0, q, st), "ffc_pool2_act", "activation"),
        (L.ffc_pool2_act(p, 1 << 31, 2, 2, 1, 0.0, q, st), "ffc_pool2_act", "32-bit"),
        (L.ffc_pool2_act_bwd(p, None, 1, 2, 2, 1, 0.0, q, st), "ffc_pool2_act_bwd", "null"),
        (L.ffc_pool2_act_bwd(p, p, 1, 2, -2, 1, 0.0, q, st), "ffc_pool2_act_bwd", "shape"),
        (L.ffc_pool2_act_bwd(p, p, 1, 2, 2, 5, 0.0, q, st), "ffc_pool2_act_bwd", "activation"),
        (L.ffc_relu_sum_pool(None, 1, 16, q, st), "ffc_relu_sum_pool", "null"),
        (L.ffc_relu_sum_pool(p, 1, 0, q, st), "ffc_relu_sum_pool", "shape"),
        (L.ffc_relu_sum_pool(p, 1 << 31, 2, q, st), "ffc_relu_sum_pool", "32-bit"),
        (L.ffc_relu_sum_pool_bwd(p, p, 1, 16, None, st), "ffc_relu_sum_pool_bwd", "null"),
        (L.ffc_relu_sum_pool_bwd(p, p, 0, 16, q, st), "ffc_relu_sum_pool_bwd", "shape"),
    ]
    assert all(status == A.E_INVALID for status, _, _ in cases)
    # the error text of the last call, and of one call made again for each word
    A.rejected(L.ffc_relu_sum_pool_bwd(p, p, 0, 16, q, st), "ffc_relu_sum_pool_bwd", "shape")
    A.rejected(L.ffc_pool2_act(p, 1, 3, 4, 1, 0.0, q, st), "ffc_pool2_act", "odd")
    A.rejected(L.ffc_act_up2b(p, None, None, 0, 1 << 15, 1 << 15, 1, 1, 0, 0.0, q, st), "ffc_act_up2b", "32-bit")
    A.rejected(L.ffc_act_up2b(None, None, None, 0, 1, 1, 4, 4, 0, 0.0, q, st), "ffc_act_up2b", "null")
    assert y.untouched()
