"""float64 references and fixed-seed input builders of the training-path kernels
(csrc/train_kernels.hip), shared by test_gpu_train_kernels.py (kernel against reference on the GPU)
and test_train_refs_cpu.py (reference against an independent statement of the same operation).

Everything here is plain torch on the CPU in float64; inputs are float32 tensors (what the kernels
read), widened exactly.  Nothing in this file imports the package under test."""
import torch
import torch.nn.functional as F

SLOPE = 0.1       # LeakyReLU slope of every case
KINK = 1e-3       # no ReLU / LeakyReLU pre-activation of a built input lies within this of 0
ACTS = (0, 1, 2, 3, 4, 5)   # Identity, ReLU, LeakyReLU, Tanh, Sigmoid, GELU (include/ffc_amd.h)


def act64(z, code, slope=SLOPE):
    return {0: lambda v: v, 1: F.relu, 2: lambda v: F.leaky_relu(v, slope), 3: torch.tanh, 4: torch.sigmoid,
            5: F.gelu}[code](z)


# --------------------------------------------------------------------------- weight gradient
# dW[m][n][kh][kw] = sum_b sum_q U[b,m,q] * V[b,n, qy*s - p + kh*d, qx*s - p + kw*d]
# name: (U shape, V shape, k, s, p, d, reference op, split counts)
WGRAD_CASES = {
    "a": ((2, 24, 8, 8), (2, 16, 8, 8), 3, 1, 1, 1, "conv", (1, 3, 16, 17)),
    "b": ((3, 20, 5, 5), (3, 7, 10, 10), 4, 2, 1, 1, "convT", (1, 2, 5)),
    "c": ((2, 130, 4, 4), (2, 9, 8, 8), 4, 2, 1, 1, "convT", (1, 2, 4)),
    "d": ((1, 5, 6, 6), (1, 3, 6, 6), 3, 1, 2, 2, "conv", (1, 4)),
    "e": ((2, 6, 4, 3), (2, 5, 9, 7), 4, 2, 1, 1, "conv", (1, 3)),
    "f": ((3, 2, 1, 1), (3, 32, 1, 1), 1, 1, 0, 1, "conv", (1,)),
    "f_swapped": ((3, 32, 1, 1), (3, 2, 1, 1), 1, 1, 0, 1, "conv", (1,)),
    "g": ((5, 3, 1, 1), (5, 12, 4, 4), 4, 1, 0, 1, "conv", (1, 5)),
    "h": ((4, 24, 8, 8), (4, 16, 8, 8), 3, 1, 1, 1, "conv", (32, 31)),
}


def wgrad_inputs(name):
    us, vs = WGRAD_CASES[name][:2]
    gen = torch.Generator().manual_seed(1000 + sorted(WGRAD_CASES).index(name))
    return torch.randn(us, generator=gen), torch.randn(vs, generator=gen)


def wgrad_ref_conv(U, V, k, s, p, d):
    """weight gradient of y = conv2d(V, w) under dy = U, by autograd in float64"""
    w = torch.zeros(U.shape[1], V.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(V.double(), w, stride=s, padding=p, dilation=d)
    assert y.shape == U.shape, (y.shape, U.shape)
    y.backward(U.double())
    return w.grad


def wgrad_ref_convT(U, V, k, s, p, d):
    """weight gradient of y = conv_transpose2d(U, w) under dy = V, by autograd in float64"""
    w = torch.zeros(U.shape[1], V.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    op = tuple(V.shape[2 + i] - ((U.shape[2 + i] - 1) * s - 2 * p + d * (k - 1) + 1) for i in range(2))
    y = F.conv_transpose2d(U.double(), w, stride=s, padding=p, dilation=d, output_padding=op)
    assert y.shape == V.shape, (y.shape, V.shape)
    y.backward(V.double())
    return w.grad


def wgrad_ref(name):
    """(U, V, float64 dW) of a case, by the autograd of the op the case is named after"""
    U, V = wgrad_inputs(name)
    _, _, k, s, p, d, kind, _ = WGRAD_CASES[name]
    return U, V, (wgrad_ref_conv if kind == "conv" else wgrad_ref_convT)(U, V, k, s, p, d)


def wgrad_formula(U, V, k, s, p, d):
    """the U/V definition written out with unfold: the columns of V gathered at q*s - p + t*d (zero
    outside V), contracted with U over (b, q)"""
    B, Mu, PH, PW = U.shape
    Nv = V.shape[1]
    cols = F.unfold(V.double(), k, dilation=d, padding=p, stride=s)       # (B, Nv*k*k, L), L >= PH*PW
    oh = (V.shape[2] + 2 * p - d * (k - 1) - 1) // s + 1
    ow = (V.shape[3] + 2 * p - d * (k - 1) - 1) // s + 1
    assert (oh, ow) == (PH, PW)
    return torch.einsum("bmq,bnq->mn", U.double().reshape(B, Mu, PH * PW), cols).reshape(Mu, Nv, k, k)


# --------------------------------------------------------------------------- planar DFTs
DFT_SHAPES = [(5, 4, 4), (3, 6, 10), (2, 1, 2), (3, 5, 7), (70, 4, 4), (1, 64, 48), (1, 48, 64), (3, 8, 8),
              (2, 16, 16), (3, 32, 32), (2, 64, 64), (1, 128, 128)]


def mirror_mask(W):
    """bins of the half spectrum that have a Hermitian mirror: kw != 0 and 2 kw != W"""
    kw = torch.arange(W // 2 + 1)
    return (kw != 0) & (2 * kw != W)


def rfft2_ref(x, scale):
    """(P, H, W) -> (P, 2, H, W/2+1) float64: Re plane then Im plane of rfftn(ortho), mirrored bins x scale"""
    z = torch.fft.rfftn(x.double(), dim=(-2, -1), norm="ortho")
    z = torch.where(mirror_mask(x.shape[-1]), z * scale, z)
    return torch.stack((z.real, z.imag), dim=1)


def irfft2_ref(Z, H, W, scale, addend=None):
    """(P, 2, H, W/2+1) unconstrained Re/Im planes -> (P, H, W) float64: mirrored bins x scale, irfftn(ortho)"""
    z = torch.complex(Z[:, 0].double(), Z[:, 1].double())
    z = torch.where(mirror_mask(W), z * scale, z)
    y = torch.fft.irfftn(z, s=(H, W), dim=(-2, -1), norm="ortho")
    return y if addend is None else y + addend.double()


def dft_inputs(P, H, W):
    gen = torch.Generator().manual_seed(2000 + 131 * H + W)
    x = torch.randn(P, H, W, generator=gen)
    Z = torch.randn(P, 2, H, W // 2 + 1, generator=gen)
    r = torch.randn(P, H, W, generator=gen)
    return x, Z, r


def dot64(a, b):
    return (a.double() * b.double()).sum().item()


def adjoint_gap(lhs_a, lhs_b, rhs_a, rhs_b):
    """|<lhs_a, lhs_b> - <rhs_a, rhs_b>| over ||lhs_a|| ||lhs_b|| + ||rhs_a|| ||rhs_b|| (2-norms): by
    Cauchy-Schwarz an operand off by delta in the 2-norm moves its inner product by at most delta times the
    other operand's norm, so two maps with relative 2-norm error e that are adjoint in exact arithmetic keep
    this ratio below e"""
    den = lhs_a.double().norm() * lhs_b.double().norm() + rhs_a.double().norm() * rhs_b.double().norm()
    return abs(dot64(lhs_a, lhs_b) - dot64(rhs_a, rhs_b)) / max(den.item(), 1e-300)


# --------------------------------------------------------------------------- BatchNorm2d (+ activation)
BN_SHAPES = [(3, 5, 7), (2, 16, 64), (4, 3, 1024), (1, 300, 9), (6, 8, 1)]
BN_EPS = 1e-5


def bn_stats(x, train, rmean, rvar):
    """float64 (mean, biased var) per channel of the float32 x (B, C, HW), or the running ones"""
    if not train:
        return rmean.double(), rvar.double()
    xd = x.double()
    return xd.mean(dim=(0, 2)), xd.var(dim=(0, 2), unbiased=False)


def bn_pre(x, gamma, beta, train, rmean, rvar, eps=BN_EPS):
    """float64 BatchNorm output (the activation's input)"""
    mean, var = bn_stats(x, train, rmean, rvar)
    inv = (var + eps).rsqrt()
    g = gamma.double() if gamma is not None else torch.ones_like(inv)
    return (x.double() - mean[None, :, None]) * (g * inv)[None, :, None] + beta.double()[None, :, None]


def bn_inputs(shape, train, offset=False, with_gamma=True):
    """fixed-seed float32 inputs of one BN backward case: x, dy (B, C, HW), gamma (or None), beta, running
    statistics.  Kink-free: any element whose float64 pre-activation is within KINK of 0 is moved (through
    x) to +-2 KINK on its own side, and the pre-activation is recomputed from the moved float32 x, batch
    statistics included, until none is left; no element is ever left out of a comparison instead"""
    B, C, HW = shape
    gen = torch.Generator().manual_seed(3000 + 7 * B + 11 * C + HW + (1 if train else 0) + (2 if offset else 0))
    x = torch.randn(B, C, HW, generator=gen)
    if offset:
        x = x + 20.0
    dy = torch.randn(B, C, HW, generator=gen)
    gamma = (1.0 + 0.5 * torch.rand(C, generator=gen)) * (1 - 2 * (torch.arange(C) % 2)) if with_gamma else None
    beta = 0.3 * torch.randn(C, generator=gen)
    rmean = (20.0 if offset else 0.0) + 0.2 * torch.randn(C, generator=gen)
    rvar = 0.5 + torch.rand(C, generator=gen)
    for _ in range(100):
        z = bn_pre(x, gamma, beta, train, rmean, rvar)
        bad = z.abs() < KINK
        if not bad.any():
            break
        _, var = bn_stats(x, train, rmean, rvar)
        slope = ((gamma.double() if gamma is not None else 1.0) * (var + BN_EPS).rsqrt())[None, :, None].expand_as(z)
        target = torch.where(z >= 0, 2 * KINK, -2 * KINK)
        x = torch.where(bad, x.double() + (target - z) / slope, x.double()).float()
    else:
        raise AssertionError("kink-free builder did not converge")
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar)


def bn_ref(inp, act, train, eps=BN_EPS):
    """float64 autograd of act(F.batch_norm(x)) -> dx, dgamma (without gamma: that of gamma = 1), dbeta"""
    B, C, HW = inp["x"].shape
    x = inp["x"].double().reshape(B, C, HW, 1).requires_grad_(True)
    gamma = (inp["gamma"].double() if inp["gamma"] is not None else torch.ones(C, dtype=torch.float64))
    gamma = gamma.requires_grad_(True)
    beta = inp["beta"].double().requires_grad_(True)
    y = act64(F.batch_norm(x, inp["rmean"].double().clone(), inp["rvar"].double().clone(), gamma, beta, train, 0.1,
                           eps), act)
    y.backward(inp["dy"].double().reshape(B, C, HW, 1))
    return x.grad.reshape(B, C, HW), gamma.grad, beta.grad


def bn_ref_eval_dx(inp, act, eps=BN_EPS):
    """the eval-mode closed form dx = gamma * inv * g, g = dy * act'(pre)"""
    pre = bn_pre(inp["x"], inp["gamma"], inp["beta"], False, inp["rmean"], inp["rvar"], eps).requires_grad_(True)
    act64(pre, act).backward(inp["dy"].double())
    inv = (inp["rvar"].double() + eps).rsqrt()
    g = inp["gamma"].double() if inp["gamma"] is not None else torch.ones_like(inv)
    return (g * inv)[None, :, None] * pre.grad


def bn_forward_consts(inp, train, eps=BN_EPS):
    """what the forward hands the backward: float32 scale / shift (y = act(x * scale + shift)) and the
    float64 batch moments [C][3] = {n, sum x, sum x^2} (None in eval)"""
    x = inp["x"]
    B, C, HW = x.shape
    mean, var = bn_stats(x, train, inp["rmean"], inp["rvar"])
    inv = (var + eps).rsqrt()
    g = inp["gamma"].double() if inp["gamma"] is not None else torch.ones_like(inv)
    scale = (g * inv).float()
    shift = (inp["beta"].double() - mean * g * inv).float()
    moments = None
    if train:
        xd = x.double()
        moments = torch.stack((torch.full((C,), float(B * HW), dtype=torch.float64), xd.sum(dim=(0, 2)),
                               (xd * xd).sum(dim=(0, 2))), dim=1).contiguous()
    return scale, shift, moments


# --------------------------------------------------------------------------- SELayer
SE_CASES = [(2, 16, 8, 8, 1), (3, 5, 3, 3, 2), (1, 300, 2, 2, 4), (2, 64, 4, 4, 32), (2, 8, 4, 4, 0), (2, 16, 5, 4, 1)]


def se_hidden_pre(x, w1):
    return x.double().mean(dim=(2, 3)) @ w1.double().t()     # (B, hidden)


def se_inputs(case):
    """x, dy (B, C, H, W), w1 (hidden, C), w2 (C, hidden); w1 is moved, by the rule of bn_inputs, until no
    hidden pre-activation w1 . mean(x) lies within KINK of 0"""
    B, C, H, W, hid = case
    gen = torch.Generator().manual_seed(4000 + 13 * C + 5 * H * W + hid)
    x = torch.randn(B, C, H, W, generator=gen) + 0.5
    dy = torch.randn(B, C, H, W, generator=gen)
    w1 = torch.randn(hid, C, generator=gen) / C ** 0.5
    w2 = torch.randn(C, hid, generator=gen) / max(1, hid) ** 0.5
    m = x.double().mean(dim=(2, 3))                           # (B, C)
    for _ in range(100):
        pre = se_hidden_pre(x, w1)
        bad = pre.abs() < KINK
        if not bad.any():
            break
        b, j = [int(v) for v in bad.nonzero()[0]]
        target = 2 * KINK if pre[b, j] >= 0 else -2 * KINK
        row = w1[j].double() + (target - pre[b, j]) / (m[b] @ m[b]) * m[b]
        w1 = w1.clone()
        w1[j] = row.float()
    else:
        raise AssertionError("SE builder did not converge")
    return x, dy, w1, w2


def se_ref(x, dy, w1, w2):
    """float64 autograd of x * sigmoid(W2 . relu(W1 . mean(x))) -> y, dx, dw1, dw2"""
    xd = x.double().requires_grad_(True)
    a = w1.double().requires_grad_(True)
    b = w2.double().requires_grad_(True)
    gate = torch.sigmoid(F.linear(F.relu(F.linear(xd.mean(dim=(2, 3)), a)), b))
    y = xd * gate[:, :, None, None]
    y.backward(dy.double())
    return y.detach(), xd.grad, a.grad, b.grad


# --------------------------------------------------------------------------- small ops
def act_bwd_inputs(n, act):
    """pre-activation (kink-free for ReLU / LeakyReLU), dy, and t = what the kernel is given: the float32
    activation output, or the input for GELU"""
    gen = torch.Generator().manual_seed(5000 + act + n % 977)
    pre = torch.randn(n, generator=gen)
    pre = torch.where(pre.abs() < KINK, torch.where(pre >= 0, 2 * KINK, -2 * KINK), pre.double()).float()
    dy = torch.randn(n, generator=gen)
    t = pre if act == 5 else act64(pre.double(), act).float()
    return pre, dy, t


def act_bwd_ref(pre, dy, act):
    z = pre.double().requires_grad_(True)
    act64(z, act).backward(dy.double())
    return z.grad


def pool2_ref(x, scale):
    return F.avg_pool2d(x.double(), 2) * 4 * scale


def up2_ref(x, scale):
    return F.interpolate(x.double(), scale_factor=2, mode="nearest") * scale


def full_smallm_ref(x0, w0, x1, w1, bias, act):
    out = x0.double() @ w0.double().t()
    if x1 is not None:
        out = out + x1.double() @ w1.double().t()
    if bias is not None:
        out = out + bias.double()
    return act64(out, act)
