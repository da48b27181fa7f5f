"""fp64 restatements of the resampling kernels (ffc_act_up2b, ffc_up2b_adjoint, ffc_pool2_act, ffc_relu_sum_pool
and their backwards, include/ffc_amd.h) and of the block formulas of fastfourierconvolution_amd/resnet.py, with the
bounds the GPU tests hold the kernels to.

Bounds, as tests/sn_refs.py takes them: |got - ref| <= TOL * scale elementwise, scale the fp64 sum of the absolute
terms of the element (returned next to every reference).  TOL is fixed by the rule of tests/test_sn_refs_cpu.py --
the smallest power of ten at which the plain fp32 restatement (the same functions at dtype float32) stays under a
quarter of every bound on every input the GPU file uses, while every planted defect exceeds the whole bound
(tests/test_resnet_cpu.py checks both) -- and never by looking at a GPU result.
"""
import numpy as np
import torch
import torch.nn.functional as F

TOL = 1e-6   # test_resnet_cpu.py::test_tol_rule: the fp32 restatement's worst share is below 0.25 here, above at 1e-7

PLANES = ((1, 1), (1, 5), (5, 1), (2, 3), (7, 9), (4, 4), (16, 16))   # the GPU file's planes (h, w)
CPU_PLANES = ((1, 1), (1, 5), (2, 3), (7, 9))                         # checked against F.interpolate / autograd
BCS = ((1, 1), (1, 3), (2, 65))                                        # (B, C): B * C in {1, 3, 130}
ACTS = (0, 1)                                                          # Identity, ReLU
SCALE_FORMS = ("none", "channel", "sample")


def up_matrix(n, dtype=torch.float64, near=0.75, far=0.25, wrap=False, edges=True):
    """U (2n, n): one axis of F.interpolate(scale_factor=2, 'bilinear', align_corners=False):
    Y[2i] = far X[i-1] + near X[i], Y[2i+1] = near X[i] + far X[i+1], indices clamped to [0, n-1].
    Planted defects: near / far swapped by the caller, ``wrap`` (indices modulo n), ``edges=False`` (the clamped
    taps dropped instead of folded onto the edge pixel)"""
    U = torch.zeros(2 * n, n, dtype=dtype)
    for i in range(n):
        for r, j in ((2 * i, i - 1), (2 * i + 1, i + 1)):
            U[r, i] += near
            if 0 <= j < n:
                U[r, j] += far
            elif wrap:
                U[r, j % n] += far
            elif edges:
                U[r, min(max(j, 0), n - 1)] += far
    return U


def act_fn(z, act):
    return torch.relu(z) if act == 1 else z


def affine(x, scale, shift):
    """scale * x + shift with scale / shift None, (C,) or (B, C) -> (z, sum of absolute terms)"""
    if scale is None:
        return x, x.abs()
    s = scale.to(x.dtype).reshape((1, -1, 1, 1) if scale.dim() == 1 else scale.shape + (1, 1))
    t = shift.to(x.dtype).reshape(s.shape)
    return s * x + t, (s * x).abs() + t.abs()


def act_up2b(x, scale=None, shift=None, act=0, dtype=torch.float64, act_after=False, **defect):
    """-> (Y, bound scale): up2(act(scale x + shift)); ``act_after``: the planted defect act(up2(.))"""
    x = x.to(dtype)
    z, mag = affine(x, scale, shift)
    a = z if act_after else act_fn(z, act)
    Uh, Uw = up_matrix(x.shape[2], dtype, **defect), up_matrix(x.shape[3], dtype, **defect)
    y = torch.einsum("ri,bcij,sj->bcrs", Uh, a, Uw)
    if act_after:
        y = act_fn(y, act)
    return y, torch.einsum("ri,bcij,sj->bcrs", Uh.abs(), mag, Uw.abs())


def up2b_adjoint(dy, dtype=torch.float64, **defect):
    """-> (dX, bound scale): the transpose of the plain upsample"""
    dy = dy.to(dtype)
    Uh, Uw = up_matrix(dy.shape[2] // 2, dtype, **defect), up_matrix(dy.shape[3] // 2, dtype, **defect)
    return (torch.einsum("ri,bcrs,sj->bcij", Uh, dy, Uw),
            torch.einsum("ri,bcrs,sj->bcij", Uh.abs(), dy.abs(), Uw.abs()))


def pool2_act(x, act=0, dtype=torch.float64):
    x = x.to(dtype)
    B, C, H, W = x.shape
    v = x.reshape(B, C, H // 2, 2, W // 2, 2)
    return act_fn(0.25 * v.sum((3, 5)), act), 0.25 * v.abs().sum((3, 5))


def pool2_act_bwd(y, dy, act=0, dtype=torch.float64):
    """from the output y: nearest x2 of 0.25 * dy * act'(y)"""
    g = 0.25 * dy.to(dtype) * ((y > 0).to(dtype) if act == 1 else 1.0)
    g = g.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return g, g.abs()


def relu_sum_pool(x, dtype=torch.float64, relu=True):
    """``relu=False``: the planted defect (a plain sum)"""
    x = x.to(dtype)
    return (torch.relu(x) if relu else x).sum((2, 3)), x.abs().sum((2, 3))


def relu_sum_pool_bwd(x, dout, dtype=torch.float64):
    g = (x > 0).to(dtype) * dout.to(dtype)[:, :, None, None]
    return g, g.abs()


def share(got, ref, scale, tol=None):
    """max |got - ref| / (tol * scale); a zero scale admits only an exact result"""
    tol = TOL if tol is None else tol
    err = (got.double() - ref.double()).abs().numpy()
    sc = scale.double().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / (tol * sc))
    return float(np.max(s)) if s.size else 0.0


def inputs(h, w, B, C, seed=0):
    """x, scale / shift in both forms, dy for the (2h, 2w) plane: what the GPU file feeds the kernels"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * h + 13 * w + 7 * B + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()  # noqa: E731
    return dict(x=r(B, C, h, w), scale_c=1.0 + 0.3 * r(C), shift_c=0.5 * r(C), scale_bc=1.0 + 0.3 * r(B, C),
                shift_bc=0.5 * r(B, C), dy=r(B, C, 2 * h, 2 * w), dlow=r(B, C, h, w), dout=r(B, C))


def scale_shift(d, form):
    return {"none": (None, None), "channel": (d["scale_c"], d["shift_c"]), "sample": (d["scale_bc"], d["shift_bc"])}[form]


# ------------------------------------------------------------------ block formulas (fp64)
def conv(x, w, b, pad):
    return F.conv2d(x, w.double(), None if b is None else b.double(), padding=pad)


def pool(x):
    return pool2_act(x)[0]


def dblock(x, P, downsample, shortcut_relu=True, fused=True):
    """DBlock (fgan128_complete.py:208-278) on effective weights P = {c1.weight, c1.bias, ...}: the leading
    nn.ReLU(True) acts on x itself before the shortcut reads it, so out = pool(c2(relu(c1(a)))) + pool(c_sc(a)), a =
    relu(x) (identity shortcut: + a).  ``fused``: pool(c2(.) + c_sc(a)) as resnet.py runs it; ``shortcut_relu=False``:
    the planted defect (the shortcut fed x)"""
    x = x.double()
    a = torch.relu(x)
    s = a if shortcut_relu else x
    h = conv(torch.relu(conv(a, P["c1.weight"], P["c1.bias"], 1)), P["c2.weight"], P["c2.bias"], 1)
    if "c_sc.weight" in P:
        s = conv(s, P["c_sc.weight"], P["c_sc.bias"], 0)
    if not downsample:
        return h + s
    return pool(h + s) if fused else pool(h) + pool(s)


def up(x):
    return act_up2b(x)[0]
