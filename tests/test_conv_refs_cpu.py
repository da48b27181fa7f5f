"""The float64 references of tests/conv_refs.py against torch.nn.functional in float64, to 1e-12, at
odd sizes: what test_gpu_conv_kernels.py compares the kernels with is itself checked here, without a
GPU.  The packer references are checked against the layouts they restate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as cr
from fastfourierconvolution_amd import _lib, _plan
from oracle import ffc_oracle as O

TOL = 1e-12
Seg = _plan.Seg


def _close(a, b, tol=TOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    e = O.normwise_err(a, b)
    assert e <= tol, e


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def test_act_codes_are_the_headers_and_the_bindings():
    assert cr.ACT == {"IDENTITY": 0, "RELU": 1, "LEAKY_RELU": 2, "TANH": 3, "SIGMOID": 4, "GELU": 5}
    assert {k.upper().replace("LEAKYRELU", "LEAKY_RELU"): v for k, v in _lib.ACT.items()} == cr.ACT


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4, 5])
def test_act64_matches_torch(code):
    z = torch.randn(257, generator=_gen(code)).double() * 3
    want = {0: lambda v: v, 1: F.relu, 2: lambda v: F.leaky_relu(v, 0.1), 3: torch.tanh, 4: torch.sigmoid,
            5: F.gelu}[code](z)
    _close(cr.act64(z, code, 0.1), want)


CONV = [  # (C, IH, IW, M, k, s, p, d)
    (7, 5, 7, 6, 3, 1, 1, 1), (5, 9, 7, 4, 4, 2, 1, 1), (3, 9, 11, 5, 3, 1, 2, 2), (2, 7, 5, 3, 3, 2, 0, 2),
    (4, 3, 3, 2, 1, 1, 0, 1)]


@pytest.mark.parametrize("C,IH,IW,M,k,s,p,d", CONV)
def test_conv_segment_matches_conv2d(C, IH, IW, M, k, s, p, d):
    g = _gen(C + IH)
    x, w = torch.randn(3, C, IH, IW, generator=g), torch.randn(M, C, k, k, generator=g)
    sg = Seg("conv", C, IH, IW, k, s, p, d)
    want = F.conv2d(x.double(), w.double(), stride=s, padding=p, dilation=d)
    assert tuple(want.shape[2:]) == _plan.seg_out(sg)
    _close(cr.seg_ref(sg, x, w, 0), want)
    # the same weight under the other layout (the adjoint segments of the training path)
    _close(cr.seg_ref(sg, x, w.transpose(0, 1).contiguous(), 1), want)


CONVT = [  # (C, IH, IW, M, k, s, p, d, op)
    (5, 4, 4, 6, 4, 2, 1, 1, 0), (3, 5, 7, 4, 3, 2, 1, 1, 1), (2, 5, 5, 3, 4, 1, 0, 2, 0), (10, 1, 1, 7, 4, 1, 0, 1, 0),
    (9, 6, 8, 5, 3, 1, 1, 1, 0), (4, 3, 5, 2, 3, 2, 0, 2, 1)]


@pytest.mark.parametrize("C,IH,IW,M,k,s,p,d,op", CONVT)
def test_convT_segment_matches_conv_transpose2d(C, IH, IW, M, k, s, p, d, op):
    g = _gen(C + IH + op)
    x, w = torch.randn(3, C, IH, IW, generator=g), torch.randn(C, M, k, k, generator=g)
    sg = Seg("convT", C, IH, IW, k, s, p, d, op)
    want = F.conv_transpose2d(x.double(), w.double(), stride=s, padding=p, dilation=d, output_padding=op)
    assert tuple(want.shape[2:]) == _plan.seg_out(sg)
    _close(cr.seg_ref(sg, x, w, 1), want)
    _close(cr.seg_ref(sg, x, w.transpose(0, 1).contiguous(), 0), want)


def test_pool_is_avg_pool2d_and_gate_is_a_multiply():
    g = _gen(3)
    x = torch.randn(3, 6, 10, 14, generator=g)
    w = torch.randn(5, 6, 1, 1, generator=g)
    gate = 0.25 + 0.75 * torch.rand(3, 6, generator=g)
    _close(cr.pool2_ref(x), F.avg_pool2d(x.double(), 2, 2))
    pooled = F.avg_pool2d(x.double(), 2, 2)
    _close(cr.seg_ref(Seg("pw", 6, 5, 7, pool=True), x, w, 0), F.conv2d(pooled, w.double()))
    _close(cr.seg_ref(Seg("pw", 6, 5, 7, pool=True, gate=True), x, w, 0, gate),
           F.conv2d(pooled * gate.double()[:, :, None, None], w.double()))
    x1 = torch.randn(3, 6, 5, 7, generator=g)
    _close(cr.seg_ref(Seg("pw", 6, 5, 7, gate=True), x1, w, 0, gate),
           F.conv2d(x1.double() * gate.double()[:, :, None, None], w.double()))
    w3 = torch.randn(5, 6, 3, 3, generator=g)     # the gate multiplies the input, before the taps
    _close(cr.seg_ref(Seg("conv", 6, 5, 7, 3, 1, 1, gate=True), x1, w3, 0, gate),
           F.conv2d(x1.double() * gate.double()[:, :, None, None], w3.double(), padding=1))


@pytest.mark.parametrize("act", [0, 1, 2, 3, 5])
def test_job_is_the_sum_of_its_segments_then_bias_addend_act(act):
    B, M = 3, 7
    segs = [Seg("convT", 5, 3, 5, 4, 2, 1), Seg("convT", 3, 3, 5, 4, 2, 1), Seg("pw", 4, 6, 10, pool=True, gate=True)]
    d = cr.job_inputs(B, M, segs, 6, 10, seed=act, bias=True, addend=True)
    pre, out = cr.conv_job_ref(segs, d["xs"], d["ws"], d["layouts"], d["gates"], d["bias"], d["addend"], act, 0.1)
    want = (F.conv_transpose2d(d["xs"][0].double(), d["ws"][0].double(), stride=2, padding=1)
            + F.conv_transpose2d(d["xs"][1].double(), d["ws"][1].double(), stride=2, padding=1)
            + F.conv2d(F.avg_pool2d(d["xs"][2].double(), 2, 2) * d["gates"][2].double()[:, :, None, None],
                       d["ws"][2].double())
            + d["bias"].double()[None, :, None, None] + d["addend"].double())
    _close(pre, want)
    _close(out, {0: lambda v: v, 1: F.relu, 2: lambda v: F.leaky_relu(v, 0.1), 3: torch.tanh, 5: F.gelu}[act](want))
    assert 0.3 < pre.std() < 3 and all((x != 0).all() for x in d["xs"] + d["ws"])   # O(1), no zeros planted


@pytest.mark.parametrize("C0,C1,M,IH,IW", [(7, 0, 3, 3, 5), (9, 8, 4, 9, 4), (1, 0, 1, 1, 3)])
def test_convt_k4s2_ref_matches_conv_transpose2d(C0, C1, M, IH, IW):
    d = cr.smallm_inputs(2, C0, C1, M, IH, IW, 4, True, seed=C0, bias=True)
    want = F.conv_transpose2d(d["x0"].double(), d["w0"].double(), stride=2, padding=1)
    if C1:
        want = want + F.conv_transpose2d(d["x1"].double(), d["w1"].double(), stride=2, padding=1)
    want = torch.tanh(want + d["bias"].double()[None, :, None, None])
    _close(cr.convt_k4s2_ref(d["x0"], d["w0"], d["x1"], d["w1"], d["bias"], 3), want)


@pytest.mark.parametrize("which", ["none", "seg0", "seg1", "both"])
@pytest.mark.parametrize("noise", [False, True])
def test_conv3x3_ref_matches_conv2d_of_the_transformed_inputs(which, noise):
    B, C0, C1, M, H, W = 2, 5, 4, 3, 7, 12
    d = cr.smallm_inputs(B, C0, C1, M, H, W, 3, False, seed=5, bias=True)
    g = _gen(9)
    tf0 = cr.tf_inputs(B, C0, H, W, 5, noise, g) if which in ("seg0", "both") else None
    tf1 = cr.tf_inputs(B, C1, H, W, 2, noise, g) if which in ("seg1", "both") else None

    def tf(x, t, act):   # transform first; F.conv2d's zero padding then surrounds the transformed tensor
        if t is None:
            return x.double()
        y = act(x.double() * t["scale"].double()[None, :, None, None] + t["shift"].double()[None, :, None, None])
        return y + t["noise_w"].double()[None, :, None, None] * t["noise"].double() if noise else y
    want = (F.conv2d(tf(d["x0"], tf0, F.gelu), d["w0"].double(), padding=1)
            + F.conv2d(tf(d["x1"], tf1, lambda v: F.leaky_relu(v, 0.1)), d["w1"].double(), padding=1)
            + d["bias"].double()[None, :, None, None])
    _close(cr.conv3x3_ref(d["x0"], d["w0"], d["x1"], d["w1"], d["bias"], 3, 0.0, tf0, tf1), torch.tanh(want))


@pytest.mark.parametrize("parts", [(), (1,), (7, 7, 100), (5, 64, 65, 300)])
def test_merge_slab_of_unequal_row_groups_is_mean_and_var(parts):
    x = torch.randn(3, 6, 11, 13, generator=_gen(1)).double() * 3 + 5
    xd = x.transpose(0, 1).reshape(6, -1)
    edges = [0] + list(parts) + [xd.shape[1]]
    rows = []
    for a, b in zip(edges[:-1], edges[1:]):
        seg = xd[:, a:b]
        m = seg.mean(dim=1) if b > a else torch.zeros(6, dtype=torch.float64)
        rows.append(torch.stack((torch.full((6,), float(b - a), dtype=torch.float64), m,
                                 ((seg - m[:, None]) ** 2).sum(dim=1), torch.zeros(6, dtype=torch.float64)), dim=1))
    n, mean, var = cr.merge_slab(torch.stack(rows))
    assert torch.equal(n, torch.full((6,), float(xd.shape[1]), dtype=torch.float64))
    _close(mean, xd.mean(dim=1))
    _close(var, xd.var(dim=1, unbiased=False))


# --------------------------------------------------------------------------- packer references
@pytest.mark.parametrize("n", [1, 7, 8, 257])
def test_split_bf16_ref_is_three_bf16_pieces_that_sum_to_the_input(n):
    x = cr.split_inputs(n, seed=n)
    assert x.shape == (n,) and x.dtype == np.float32
    if n >= 14:
        assert (x == 0).any() and (x < 0).any() and ((x.view(np.uint32) & 0xFFFF) == 0xFFFF).any()
    hi, mid, lo = cr.split_bf16_ref(x)
    assert all(p.dtype == np.uint16 and p.shape == (n,) for p in (hi, mid, lo))
    total = cr.bf16_to_f64(hi) + cr.bf16_to_f64(mid) + cr.bf16_to_f64(lo)
    assert np.array_equal(total, x.astype(np.float64))
    assert np.array_equal(hi, (x.view(np.uint32) >> 16).astype(np.uint16))      # hi is x truncated to bf16
    # each piece takes 8 significand bits: what is left after one / two pieces is below 2^-7 / 2^-15 of |x|
    xd = x.astype(np.float64)
    assert (np.abs(xd - cr.bf16_to_f64(hi)) <= 2.0 ** -7 * np.abs(xd)).all()
    assert (np.abs(xd - cr.bf16_to_f64(hi) - cr.bf16_to_f64(mid)) <= 2.0 ** -15 * np.abs(xd)).all()


def test_pack_ref_of_a_full_tap_conv_is_the_flattened_weight():
    """generic plan of an unpadded Conv2d: every tap of every channel is in bounds, k = (channel, ky, kx),
    so A[:M, :K] is w.reshape(M, C k k); rows M..Mpad and columns K..Kpad are zero"""
    M, C, k = 5, 3, 3
    plan = _plan.plan_job(2, M, [Seg("conv", C, 6, 7, k, 1, 0)])
    w = torch.randn(M, C, k, k, generator=_gen(2))
    A = cr.pack_ref(plan, [w], [0]).reshape(plan.Mpad, plan.phases[0].Kpad)
    assert plan.phases[0].K == C * k * k and plan.phases[0].Kpad == 32 and plan.Mpad == 128
    assert np.array_equal(A[:M, :27], w.reshape(M, 27).numpy())
    assert not A[M:].any() and not A[:, 27:].any()


def test_pack_ref_follows_both_plan_kinds():
    """the patch plan of a 3x3 conv runs 4x4 taps in 4-channel chunks with a zero 4th row / column: the
    same weights at other k, (M, Cpad, 4, 4) with zero padding"""
    M, C = 5, 7
    segs = [Seg("conv", C, 6, 8, 3, 1, 1)]
    pp = _plan.plan_patch_job(2, M, segs, 2)
    assert pp is not None and pp.cc == [4] and pp.cpad == [8]
    w = torch.randn(M, C, 3, 3, generator=_gen(4))
    A = cr.pack_ref(pp, [w], [0]).reshape(pp.Mpad, pp.phases[0]["Kpad"])
    want = np.zeros((M, 8, 4, 4), dtype=np.float32)
    want[:, :C, :3, :3] = w.numpy()
    assert np.array_equal(A[:M], want.reshape(M, 128)) and not A[M:].any()


def test_unpack_a3_inverts_the_documented_fragment_order():
    segs = [Seg("convT", 20, 4, 4, 4, 2, 1), Seg("pw", 8, 8, 8)]
    q = _plan.plan_convq_job(3, 40, segs, 0)
    assert q is not None and q.q
    rng = np.random.default_rng(0)
    planes = [rng.integers(0, 1 << 16, q.a_size).astype(np.uint16) for _ in range(3)]
    A3 = np.zeros(3 * q.a_size, dtype=np.uint16)
    for ph in q.phases:                       # the header's formula, element by element
        Kpad, a_off = ph["Kpad"], ph["a_off"]
        for mtile in range(q.Mpad // 32):
            for kstep in range(Kpad // 16):
                for piece in range(3):
                    for lane in range(64):
                        m, k0 = 32 * mtile + (lane & 31), 16 * kstep + 8 * (lane >> 5)
                        dst = 3 * a_off + ((mtile * (Kpad // 16) + kstep) * 3 + piece) * 512 + lane * 8
                        A3[dst: dst + 8] = planes[piece][a_off + m * Kpad + k0: a_off + m * Kpad + k0 + 8]
    got = cr.unpack_a3(q, A3)
    assert all(np.array_equal(g, p) for g, p in zip(got, planes))
