"""float64 references, fixed-seed inputs and the case table of the small-M ConvTranspose2d(k3, s1, p1) head
kernels (csrc/convt3_smallm.hip: ffc_convt3x3_smallm and ffc_convt3x3_smallm_dgrad), shared by
test_baseline_cpu.py (references against float64 autograd, fp32 headroom) and test_gpu_convt3_kernels.py
(kernels against the references through the C ABI).

The references are written out tap by tap from the definition
    out[b, m, oy, ox] = act(bias[m] + sum_{c, ky, kx} x[b, c, oy + 1 - ky, ox + 1 - kx] w[c, m, ky, kx])
    dx[b, c, iy, ix]  =           sum_{m, ky, kx} dpre[b, m, iy - 1 + ky, ix - 1 + kx] w[c, m, ky, kx]
and do not call conv_transpose2d; test_baseline_cpu.py pins them against it.

Bound (the project's kernel bound): |got - ref| <= 1e-5 (|ref| + rms(ref)) per element.
"""
import numpy as np
import torch
import torch.nn.functional as F

TANH, IDENT = 3, 0
TILE_W, TILE_H = 32, 16     # CT3_TW, CT3_TH of csrc/convt3_smallm.hip

# name: (B, C, M, H, W, bias, act, seed) -> the branch it is there for
CASES = {
    "c1_m1_1x1": (1, 1, 1, 1, 1, True, TANH, 11),         # one pixel: every tap but the centre out of bounds
    "c3_m3_3x5_b3": (3, 3, 3, 3, 5, False, IDENT, 12),    # odd width (scalar path), fewer channels than waves
    "c64_m3_8x8": (1, 64, 3, 8, 8, True, TANH, 13),       # the generators' head at mg = 1 (float4 path)
    "c64_m4_24x24_b3": (3, 64, 4, 24, 24, True, IDENT, 14),   # mg = 3 plane: two row tiles, the second partial
    "cap_m3_33x7": (1, 256, 3, 33, 7, True, TANH, 15),    # the channel cap, odd width, three row tiles
    "c3_m1_5x72_b3": (3, 3, 1, 5, 72, False, TANH, 16),   # wider than one LDS tile: three column tiles, float4
    "c64_m4_20x37": (1, 64, 4, 20, 37, True, TANH, 17),   # 2 x 2 tiles, both edges partial, scalar path
    "c1_m4_8x8_b3": (3, 1, 4, 8, 8, False, IDENT, 18),    # one channel: three waves idle
    "cap_m4_24x24": (1, 256, 4, 24, 24, False, TANH, 19),  # the cap at M = 4 (the largest register footprint)
}


def inputs(name):
    """-> x (B, C, H, W), w (C, M, 3, 3), bias (M) or None, dpre (B, M, H, W): float32 CPU tensors"""
    B, C, M, H, W, has_bias, _, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, M, 3, 3, generator=g) * (9 * C) ** -0.5
    bias = 0.1 * torch.randn(M, generator=g) if has_bias else None
    dpre = torch.randn(B, M, H, W, generator=g)
    return x, w, bias, dpre


def act64(v, act):
    return torch.tanh(v) if act == TANH else v


def head_ref(x, w, bias, act):
    """float64 forward, tap by tap"""
    x, w = x.double(), w.double()
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(B, w.shape[1], H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("bchw,cm->bmhw", xp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W], w[:, :, ky, kx])
    if bias is not None:
        out += bias.double().view(1, -1, 1, 1)
    return act64(out, act)


def dgrad_ref(dpre, w):
    """float64 data gradient, tap by tap"""
    dpre, w = dpre.double(), w.double()
    B, M, H, W = dpre.shape
    gp = F.pad(dpre, (1, 1, 1, 1))
    dx = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dx += torch.einsum("bmhw,cm->bchw", gp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return dx


def bound(ref):
    """per-element bound 1e-5 (|ref| + rms(ref))"""
    ref = ref.double()
    return 1e-5 * (ref.abs() + float(ref.pow(2).mean().sqrt()))


def worst(got, ref):
    """largest |got - ref| as a share of the per-element bound (<= 1 passes)"""
    return float(((got.double() - ref.double()).abs() / bound(ref)).max())


def normal_state(mod, seed):
    """weights for a model built here: N(0, 1 / fan_in) convs and Linear, BN weight about 1, gamma 0.7"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            if not v.is_floating_point():
                continue
            if k.endswith("gamma"):
                v.fill_(0.7)
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif v.dim() > 1:
                v.copy_(torch.randn(v.shape, generator=g) / max(1, v[0].numel()) ** 0.5)
            else:
                v.copy_((1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=g))
    return mod


def as_numpy(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())
