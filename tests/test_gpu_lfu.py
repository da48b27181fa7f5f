"""The local Fourier unit (LFU) of SpectralTransform on the GPU: the four data-movement kernels of
csrc/lfu_kernels.hip against torch indexing, the ffc::lfu_split / ffc::lfu_tile_add ops, and
SpectralTransform / FFCGenerator with run_lfu against the fp64 restatement of tests/lfu_refs.py
(the reference never executes this branch, so there is no reference golden).  Normwise 1e-4
 for the module outputs and gradients; the kernel bounds are stated per test."""
import contextlib
import io

import pytest
import torch

import lfu_refs as R
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
# (B, c, H, W, up): one channel per quadrant; non-square; upsampled source; a 2x2 quadrant (scalar
# tail: W/2 % 4 != 0); a plane wide enough for 16-byte rows in more than one workgroup
PLANES = [(2, 4, 8, 8, 1), (3, 8, 8, 16, 1), (2, 8, 8, 8, 2), (2, 12, 4, 4, 1), (1, 16, 32, 32, 1)]


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _lib():
    from fastfourierconvolution_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == 0, (what, rc, _lib().ffc_last_error())


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,c,H,W,up", PLANES)
def test_gather_against_indexing(B, c, H, W, up):
    L = _lib()
    t = _randn(B, c, H // up, W // up, seed=1)
    full = t.repeat_interleave(up, 2).repeat_interleave(up, 3) if up == 2 else t
    xs = torch.full((B, c, H // 2, W // 2), float("nan"), device=DEV)
    _ok(L.ffc_lfu_gather(t.data_ptr(), B, c, H // up, W // up, up, None, None, 0, xs.data_ptr(), _stream()), "gather")
    assert torch.equal(xs, R.lfu_split(full))   # identity transform: a permutation, bitwise
    sc, sh = 1.0 + 0.3 * _randn(c, seed=2), 0.3 * _randn(c, seed=3)
    ref = R.lfu_split(torch.relu(full.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]))
    xs.fill_(float("nan"))
    _ok(L.ffc_lfu_gather(t.data_ptr(), B, c, H // up, W // up, up, sc.data_ptr(), sh.data_ptr(), 1, xs.data_ptr(),
                         _stream()), "gather")
    err = normwise_err(xs.cpu(), ref.cpu())   # one fused multiply-add per element: <= 2^-24 relative
    assert err <= 1e-6, err
    # shift alone / no ReLU: the null scale reads as 1
    _ok(L.ffc_lfu_gather(t.data_ptr(), B, c, H // up, W // up, up, None, sh.data_ptr(), 0, xs.data_ptr(), _stream()),
        "gather")
    assert torch.equal(xs, R.lfu_split(full + sh[None, :, None, None]))


@pytest.mark.parametrize("B,c,H,W,up", PLANES)
def test_tile_add_bitwise(B, c, H, W, up):
    L = _lib()
    v, ys = _randn(B, c, H, W, seed=4), _randn(B, c, H // 2, W // 2, seed=5)
    ref = v + ys.repeat(1, 1, 2, 2)
    out = torch.full_like(v, float("nan"))
    _ok(L.ffc_lfu_tile_add(v.data_ptr(), ys.data_ptr(), B, c, H, W, out.data_ptr(), _stream()), "tile_add")
    assert torch.equal(out, ref)
    _ok(L.ffc_lfu_tile_add(v.data_ptr(), ys.data_ptr(), B, c, H, W, v.data_ptr(), _stream()), "tile_add in place")
    assert torch.equal(v, ref)


@pytest.mark.parametrize("B,c,H,W,up", PLANES)
def test_adjoints_against_fp64_autograd(B, c, H, W, up):
    L = _lib()
    dxs, dv = _randn(B, c, H // 2, W // 2, seed=6), _randn(B, c, H, W, seed=7)
    s = torch.zeros(B, c, H, W, dtype=torch.float64, device=DEV, requires_grad=True)
    (ds_ref,) = torch.autograd.grad(R.lfu_split(s), s, dxs.double())
    ds = torch.full((B, c, H, W), float("nan"), device=DEV)
    _ok(L.ffc_lfu_gather_bwd(dxs.data_ptr(), B, c, H, W, ds.data_ptr(), _stream()), "gather_bwd")
    assert torch.equal(ds.double(), ds_ref)   # a permutation plus zeros: bitwise
    ys = torch.zeros(B, c, H // 2, W // 2, dtype=torch.float64, device=DEV, requires_grad=True)
    (dys_ref,) = torch.autograd.grad(R.lfu_tile(ys), ys, dv.double())
    dys = torch.full((B, c, H // 2, W // 2), float("nan"), device=DEV)
    _ok(L.ffc_lfu_tile_bwd(dv.data_ptr(), B, c, H, W, dys.data_ptr(), _stream()), "tile_bwd")
    err = normwise_err(dys.cpu(), dys_ref.cpu())   # three fp32 adds per element
    assert err <= 1e-6, err
    again = torch.empty_like(dys)
    _ok(L.ffc_lfu_tile_bwd(dv.data_ptr(), B, c, H, W, again.data_ptr(), _stream()), "tile_bwd")
    assert torch.equal(again, dys)   # fixed summation order


def test_opcheck_lfu_ops():
    def opcheck(op, args):
        res = torch.library.opcheck(op, args, raise_exception=False)
        bad = {k: v for k, v in res.items() if v != "SUCCESS"}
        assert not bad, f"{op}: {bad}"
    for B, c, H, W in ((2, 8, 8, 8), (2, 12, 4, 4)):
        s = _randn(B, c, H, W, seed=8).requires_grad_()
        ys = _randn(B, c, H // 2, W // 2, seed=9).requires_grad_()
        opcheck(torch.ops.ffc.lfu_split.default, (s,))
        opcheck(torch.ops.ffc.lfu_tile_add.default, (s, ys))
        opcheck(torch.ops.ffc.lfu_split_backward.default, (ys,))
        opcheck(torch.ops.ffc.lfu_tile_backward.default, (s.detach(),))
    xs = torch.ops.ffc.lfu_split(s)
    assert torch.equal(xs, R.lfu_split(s))
    (g,) = torch.autograd.grad(torch.ops.ffc.lfu_tile_add(s, xs).sum(), s)
    assert torch.equal(g[:, :c // 4], torch.full_like(g[:, :c // 4], 5.0)) and torch.equal(
        g[:, c // 4:], torch.ones_like(g[:, c // 4:]))


# ------------------------------------------------------------------ SpectralTransform
# (cin, cout, stride, upsample, input H = W, B)
ST_CASES = {
    "s1_32_8x8": (32, 32, 1, False, 8, 3),          # LFU at c = 16, 4x4
    "up_32to16_4x4": (32, 16, 2, True, 4, 3),       # transposed: 4x4 -> 8x8, LFU at c = 8, 4x4
    "pool_16to32_16x16": (16, 32, 2, False, 16, 3),  # pooled: 16x16 -> 8x8
    "s1_64_32x32": (64, 64, 1, False, 32, 2),       # small batch: staged fu at 32x32, LFU at 16x16
}


def _st(case, seed, running):
    import fastfourierconvolution_amd as F
    cin, cout, stride, upsample, hw, B = ST_CASES[case]
    st = F.SpectralTransform(cin, cout, stride, enable_lfu=True, upsample=upsample)
    sd = R.random_state(st, seed, running)
    st.load_state_dict(sd)
    x = torch.randn(B, cin, hw, hw, generator=torch.Generator().manual_seed(seed + 100))
    return st.to(DEV), sd, x


@pytest.mark.parametrize("case", list(ST_CASES))
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_spectral_transform_lfu_vs_restatement(case, train):
    import fastfourierconvolution_amd as F
    _, _, stride, upsample, _, _ = ST_CASES[case]
    st, sd, x = _st(case, seed=21, running=not train)
    F.set_lfu(st).train(train)
    ref_sd = R.to_double(sd)
    steps = 2 if train else 1
    for _ in range(steps):   # two train-mode forwards: the running statistics move twice
        with torch.no_grad():
            out = st(x.to(DEV))
        ref = R.spectral_transform_lfu(x.double(), ref_sd, "", stride, upsample, train)
    err = normwise_err(out.cpu(), ref)
    assert err <= TOL, err
    got = st.state_dict()
    for bn in ("bn1", "fu.bn", "lfu.bn"):
        assert int(got[bn + ".num_batches_tracked"]) == int(ref_sd[bn + ".num_batches_tracked"]) == (steps if train
                                                                                                      else 0), bn
        for k in ("running_mean", "running_var"):
            torch.testing.assert_close(got[f"{bn}.{k}"].cpu().double(), ref_sd[f"{bn}.{k}"], rtol=1e-4, atol=1e-5,
                                       msg=f"{bn}.{k}")


@pytest.mark.parametrize("grad", [False, True], ids=["inference", "training"])
def test_refusals(grad):
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd._lib import FFCError
    odd = F.set_lfu(F.SpectralTransform(8, 12, enable_lfu=True).to(DEV))           # c = 6
    plane24 = F.set_lfu(F.SpectralTransform(32, 32, enable_lfu=True).to(DEV))      # 24x24 -> a 12x12 LFU plane
    for st, x, what in ((odd, torch.randn(2, 8, 8, 8, device=DEV), "c=6"),
                        (plane24, torch.randn(2, 32, 24, 24, device=DEV), "24x24")):
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match=what) as ei:
            st(x)
        assert not isinstance(ei.value, FFCError)
        assert int(st.lfu.bn.num_batches_tracked) == 0 and int(st.bn1.num_batches_tracked) == 0
    F.set_lfu(plane24, False)
    with torch.set_grad_enabled(grad):
        assert torch.isfinite(plane24(x)).all()   # the 24x24 plane itself runs: only its LFU has no kernel


def test_fp16_mix_with_lfu_raises():
    import fastfourierconvolution_amd as F
    st = F.set_mix_precision(F.set_lfu(F.SpectralTransform(64, 64, enable_lfu=True).to(DEV).eval()), "fp16")
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp32 only"):
        st(torch.randn(2, 64, 32, 32, device=DEV))


@pytest.mark.parametrize("case", ["s1_32_8x8", "up_32to16_4x4"])
def test_off_means_off(case):
    """run_lfu False: the lfu parameters do not reach the output, its BN never runs, it gets no gradient"""
    st, sd, x = _st(case, seed=31, running=False)
    st.train()
    x = x.to(DEV)
    assert st.run_lfu is False
    with torch.no_grad():
        a = st(x)
        for p in st.lfu.parameters():
            p.zero_()
        b = st(x)
    assert torch.equal(a, b)
    xg = x.clone().requires_grad_()
    st(xg).square().sum().backward()
    assert int(st.lfu.bn.num_batches_tracked) == 0
    assert torch.equal(st.lfu.bn.running_mean, torch.zeros_like(st.lfu.bn.running_mean))
    assert all(p.grad is None for p in st.lfu.parameters())
    assert xg.grad is not None and st.fu.conv_layer.weight.grad is not None
    # a block's fused layer op too: same launches, same bits, whatever the lfu weights hold
    import fastfourierconvolution_amd as F
    blk = _quiet(F.FFC_BN_ACT, 32, 32, 3, 0.5, 0.5, 1, 1).to(DEV).train()
    xl, xg2 = _randn(3, 16, 8, 8, seed=32), _randn(3, 16, 8, 8, seed=33)
    with torch.no_grad():
        a = blk((xl, xg2))
        for p in blk.ffc.convg2g.lfu.parameters():
            p.normal_()
        b = blk((xl, xg2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert int(blk.ffc.convg2g.lfu.bn.num_batches_tracked) == 0


@pytest.mark.parametrize("case", ["s1_32_8x8", "up_32to16_4x4"])
def test_gradients_vs_fp64_autograd(case):
    import fastfourierconvolution_amd as F
    _, cout, stride, upsample, hw, B = ST_CASES[case]
    st, sd, x = _st(case, seed=41, running=False)
    F.set_lfu(st).train()
    ho = 2 * hw if upsample else hw
    w = torch.randn(B, cout, ho, ho, generator=torch.Generator().manual_seed(42))   # the loss: <out, w>
    xg = x.to(DEV).requires_grad_()
    (st(xg) * w.to(DEV)).sum().backward()
    ref_sd = R.to_double(sd)
    names = [k for k, _ in st.named_parameters()]
    for k in names:
        ref_sd[k].requires_grad_()
    xr = x.double().requires_grad_()
    (R.spectral_transform_lfu(xr, ref_sd, "", stride, upsample, True, fft="torch") * w.double()).sum().backward()
    assert {"lfu.conv_layer.weight", "lfu.bn.weight", "lfu.bn.bias"} <= set(names)
    errs = {"x": normwise_err(xg.grad.cpu(), xr.grad)}
    for k, p in st.named_parameters():
        assert p.grad is not None, k
        errs[k] = normwise_err(p.grad.cpu(), ref_sd[k].grad)
    assert max(errs.values()) <= TOL, errs
    assert int(st.lfu.bn.num_batches_tracked) == 1


# ------------------------------------------------------------------ whole model
def test_generator_with_lfu():
    import fastfourierconvolution_amd as F
    g = _quiet(F.FFCGenerator, 100, 3, 64)
    g.load_state_dict(R.random_state(g, seed=51))
    g = g.to(DEV).train()
    z = _randn(4, 100, 1, 1, seed=52)
    with torch.no_grad():
        off = g(z)
    F.set_lfu(g)
    live = [m for m in g.modules() if isinstance(m, F.SpectralTransform)]
    assert len(live) == 3 and all(int(m.lfu.bn.num_batches_tracked) == 0 for m in live)
    with torch.no_grad():
        on = g(z)
    assert torch.isfinite(on).all()
    assert normwise_err(on.cpu(), off.cpu()) > 1e-3
    assert all(int(m.lfu.bn.num_batches_tracked) == 1 for m in live)
    for train in (True, False):
        g.train(train)
        with torch.no_grad():
            eager = g(z)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                g(z)
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = g(z)
            graph.replay()
            torch.cuda.synchronize()
        assert torch.equal(out, eager), train


def test_generator_with_lfu_vs_restatement():
    """the generator's three live LFUs (4x4, 8x8 and 16x16 planes behind the transposed layers) against
    the restatement chained through the oracle's layers"""
    import fastfourierconvolution_amd as F
    from oracle import ffc_oracle as O
    g = _quiet(F.FFCGenerator, 100, 3, 64)
    sd = R.random_state(g, seed=61)
    g.load_state_dict(sd)
    g = F.set_lfu(g.to(DEV).train())
    z = torch.randn(4, 100, 1, 1, generator=torch.Generator().manual_seed(62))
    with torch.no_grad():
        out = g(z.to(DEV))
    orig = O.spectral_transform
    O.spectral_transform = R.spectral_transform_lfu   # same signature; the oracle's layers call it by name
    try:
        ref = O.ffc_generator(z.double(), R.to_double(sd), 100, 3, 64, True)
    finally:
        O.spectral_transform = orig
    err = normwise_err(out.cpu(), ref)
    assert err <= TOL, err
