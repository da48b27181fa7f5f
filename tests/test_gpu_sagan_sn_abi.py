"""ffc_sn_job.flags bit 0 (FFC_SN_EPS_ADD, the SAGAN wrapper's x / (||x|| + 1e-12)) through the C ABI with guarded
buffers (tests/abi_bufs.py) against float64 (tests/sagan_refs.sn_refresh / sn_backward).

Shapes (M, K): (3, 5) the 4-byte path in one workgroup; (64, 48) the critic's l1; (100, 4096) the generator's l1 at
z = 100, two matvec column chunks; (65, 2049) ragged in both tilings.  Weights n / sqrt(K), u and v unit vectors.

Bounds, normwise (1e-5 where the float32 evaluation of the same formulas stays under 2.5e-6, four
times its error otherwise -- ``_check`` computes the float32 figure on the CPU for the case at hand and prints it):
u', v', sigma, W, dw_bar.  The tiny-norm case is decided by which float64 form the result is near: the two differ by
about a factor of two there.  flags = 0 must leave the bits the existing entry point gives, alone and in a mixed table."""
import numpy as np
import pytest
import torch

import abi_bufs as B
import sagan_refs as R
from abi_bufs import Buf

pytestmark = pytest.mark.gpu
SHAPES = ((3, 5), (64, 48), (100, 4096), (65, 2049))


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    B.end_of_test()


def _case(M, K, seed=0, scale=None, zero=False):
    rs = np.random.RandomState(seed + 7 * M + K)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    w, u, v, g = f(M, K) / K ** 0.5, f(M), f(K), f(M, K)
    u, v = (u.double() / u.double().norm()).float(), (v.double() / v.double().norm()).float()
    if scale is not None:      # ||Wm^T u|| = scale
        w = (w.double() * (scale / float(w.double().t().mv(u.double()).norm()))).float()
    if zero:
        w = torch.zeros(M, K)
    return dict(M=M, K=K, w=w, u=u, v=v, g=g)


class _Table:
    def __init__(self, cases, flags):
        from fastfourierconvolution_amd import _lib
        L = B.lib()
        self.cases, self.n = cases, len(cases)
        self.bufs, off = [], 0
        self.arr = (_lib.SnJob * self.n)()
        for a, c, fl in zip(self.arr, cases, flags):
            M, K = c["M"], c["K"]
            b = dict(w_orig=Buf(M * K, fill=c["w"]), u=Buf(M, fill=c["u"]), v=Buf(K, fill=c["v"]), w=Buf(M * K),
                     sigma=Buf(1), dw=Buf(M * K, fill=c["g"]), dwo=Buf(M * K))
            self.bufs.append(b)
            a.w_orig, a.u, a.v, a.w, a.sigma = (b[k].ptr() for k in ("w_orig", "u", "v", "w", "sigma"))
            a.dw, a.dw_orig = b["dw"].ptr(), b["dwo"].ptr()
            a.M, a.K, a.R, a.stride_m, a.stride_i, a.flags, a.ws_off = M, K, K, K, 0, fl, off
            off += L.ffc_sn_ws_bytes(M, K)
        self.ws_bytes = off
        self.ws = Buf(off // 4)

    def forward(self):
        B.ok(B.lib().ffc_sn_forward(self.arr, self.n, 1, self.ws.ptr(), self.ws_bytes, B.stream()), "ffc_sn_forward")
        return self

    def backward(self):
        B.ok(B.lib().ffc_sn_backward(self.arr, self.n, self.ws.ptr(), self.ws_bytes, B.stream()), "ffc_sn_backward")
        return self

    def read(self, i, finite=True):
        b, c = self.bufs[i], self.cases[i]
        get = (lambda k: b[k].get(k)) if finite else (lambda k: b[k].raw())
        return dict(u=get("u"), v=get("v"), sigma=get("sigma"), w=get("w").reshape(c["M"], c["K"]))


def _ref(c, dtype, normalize=R.l2n_add):
    w, u, v, s = R.sn_refresh(c["w"].to(dtype), c["u"].to(dtype), c["v"].to(dtype), normalize)
    return dict(w=w, u=u, v=v, sigma=s.reshape(1))


def _check(name, got, c):
    ref, f32 = _ref(c, torch.float64), _ref(c, torch.float32)
    for k in ("u", "v", "sigma", "w"):
        fig = R.nerr(f32[k], ref[k])
        e = R.nerr(got[k], ref[k])
        print(f"OBS {name} {k}: gpu {e:.3e} float32 {fig:.3e} bound {R.bound(fig):.3e}")
        assert e <= R.bound(fig), (name, k, e, fig)


@pytest.mark.parametrize("M,K", SHAPES)
def test_eps_add_matches_fp64_forward_and_backward(M, K):
    c = _case(M, K)
    t = _Table([c], [1]).forward()
    got = t.read(0)
    _check(f"{M}x{K}", got, c)
    t.backward()
    dwo = t.bufs[0]["dwo"].get("dw_orig").reshape(M, K)
    ref = _ref(c, torch.float64)
    want = R.sn_backward(c["g"].double(), c["w"].double(), ref["u"], ref["v"], ref["sigma"][0])
    r32 = _ref(c, torch.float32)
    fig = R.nerr(R.sn_backward(c["g"], c["w"], r32["u"], r32["v"], r32["sigma"][0]), want)
    e = R.nerr(dwo, want)
    print(f"OBS {M}x{K} dw_bar: gpu {e:.3e} float32 {fig:.3e} bound {R.bound(fig):.3e}")
    assert e <= R.bound(fig)
    again = _Table([c], [1]).forward().read(0)
    for k in got:
        assert torch.equal(again[k], got[k]), k


@pytest.mark.parametrize("M,K", ((3, 5), (64, 48)))
def test_tiny_norm_follows_the_eps_add_form(M, K):
    """||Wm^T u|| = 1e-12: v' = p / (||p|| + eps) has norm 1/2 where the hook's p / max(||p||, eps) has norm 1"""
    c = _case(M, K, scale=1e-12)
    add, mx = _ref(c, torch.float64, R.l2n_add), _ref(c, torch.float64, R.l2n_max)
    assert 0.4 < float(add["v"].norm()) < 0.6 and abs(float(mx["v"].norm()) - 1.0) < 1e-6
    got = _Table([c], [1]).forward().read(0)
    hook = _Table([c], [0]).forward().read(0)
    f32 = _ref(c, torch.float32, R.l2n_add)
    for k in ("u", "v", "sigma"):
        e_add, e_max, fig = R.nerr(got[k], add[k]), R.nerr(got[k], mx[k]), R.nerr(f32[k], add[k])
        print(f"OBS tiny {M}x{K} {k}: to the +eps form {e_add:.3e} (float32 {fig:.3e}), to the max form {e_max:.3e}")
        assert e_add <= R.bound(fig) and e_max > 0.1, k
    # flags = 0 keeps the hook's form: v' a unit vector
    assert abs(float(hook["v"].double().norm()) - 1.0) < 1e-5


@pytest.mark.parametrize("M,K", ((3, 5), (65, 2049)))
def test_all_zero_weight(M, K):
    c = _case(M, K, zero=True)
    got = _Table([c], [1]).forward().read(0, finite=False)
    ref = _ref(c, torch.float64)
    assert bool((got["u"] == 0).all()) and bool((got["v"] == 0).all())
    for k in ("u", "v", "sigma", "w"):
        assert torch.equal(torch.isnan(got[k]), torch.isnan(ref[k])), k
        assert torch.equal(torch.isinf(got[k]), torch.isinf(ref[k])), k


def test_flags_zero_keeps_the_bits_and_a_mixed_table_gives_each_layer_its_own():
    cases = [_case(M, K) for M, K in SHAPES]
    alone = {fl: [_Table([c], [fl]).forward().read(0) for c in cases] for fl in (0, 1)}
    # flags = 0 against the existing op, which never sets the field
    for c, a in zip(cases, alone[0]):
        dev = lambda t: t.clone().to(B.DEV)
        w_orig, u, v = dev(c["w"]), dev(c["u"]), dev(c["v"])
        w, sigma = torch.empty_like(w_orig), torch.empty(1, device=B.DEV)
        torch.ops.ffc.sn_weight([w_orig], [u], [v], [w], sigma, sigma.new_empty(0), [0], True)
        for k, t in (("u", u), ("v", v), ("sigma", sigma), ("w", w)):
            assert torch.equal(t.cpu(), a[k]), (c["M"], c["K"], k)
    for flags in ((0, 1, 0, 1), (1, 0, 1, 0)):
        t = _Table(cases, flags).forward()
        for i, fl in enumerate(flags):
            got = t.read(i)
            for k in got:
                assert torch.equal(got[k], alone[fl][i][k]), (flags, i, k)
    bad = _Table(cases[:1], [2])
    st = B.lib().ffc_sn_forward(bad.arr, 1, 1, bad.ws.ptr(), bad.ws_bytes, B.stream())
    B.rejected(st, "ffc_sn_forward", "flags")
    assert bad.ws.untouched() and bad.bufs[0]["w"].untouched()
