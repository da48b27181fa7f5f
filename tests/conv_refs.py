"""float64 references and fixed-seed input builders of the forward convolution kernels
(csrc/conv_kernels.hip, convp_kernels.hip, pw_gemm.hip, convt_smallm.hip and the weight packers),
shared by test_gpu_conv_kernels.py (kernel against reference on the GPU) and test_conv_refs_cpu.py
(reference against torch.nn.functional in float64).

Written from the contracts in include/ffc_amd.h ("local branch") and the segment description of
_plan.Seg (kind, k, s, p, d, op, pool, gate).  Everything here is plain torch / numpy on the CPU in
float64: a convolution is a sum over taps of a channel contraction of a strided slice, never a call of
torch's own convolutions.  Inputs are float32 tensors (what the kernels read), widened exactly.
Nothing in this file imports the package under test; segments and plans arrive as objects."""
import os
import re

import numpy as np
import torch

from spectral_refs import channel_stats, merge_slab  # noqa: F401  (the {n, mean, M2} row merge, shared)

SLOPE = 0.1


def _act_codes():
    """FFC_ACT_* of include/ffc_amd.h, read from the header the kernels are compiled against"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ffc_amd.h")
    with open(path) as f:
        codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FFC_ACT_(\w+)\s+(\d+)", f.read())}
    assert set(codes) == {"IDENTITY", "RELU", "LEAKY_RELU", "TANH", "SIGMOID", "GELU"}, codes
    return codes


ACT = _act_codes()


def act64(z, code, slope=SLOPE):
    """the epilogue activations of ffc::apply_act (GELU is the exact erf form)"""
    if code == ACT["IDENTITY"]:
        return z
    if code == ACT["RELU"]:
        return z.clamp_min(0)
    if code == ACT["LEAKY_RELU"]:
        return torch.where(z > 0, z, z * slope)
    if code == ACT["TANH"]:
        return torch.tanh(z)
    if code == ACT["SIGMOID"]:
        return 1 / (1 + torch.exp(-z))
    if code == ACT["GELU"]:
        return 0.5 * z * (1 + torch.erf(z * 0.5 ** 0.5))
    raise ValueError(f"unknown activation code {code}")


# --------------------------------------------------------------------------- convolutions, tap by tap
def _weight_mc(w, layout):
    """(M, C, kh, kw) float64 view of a weight: layout 0 = Conv2d (O, I, kh, kw), 1 = ConvTranspose2d
    (I, O, kh, kw) (ffc_conv_pack's w_layout)"""
    w = w.double()
    return w if layout == 0 else w.transpose(0, 1)


def conv2d_ref(x, wmc, s, p, d):
    """out[b, m, oy, ox] = sum x[b, c, oy s - p + ky d, ox s - p + kx d] w[m, c, ky, kx], zeros outside"""
    B, C, IH, IW = x.shape
    M, _, kh, kw = wmc.shape
    OH = (IH + 2 * p - d * (kh - 1) - 1) // s + 1
    OW = (IW + 2 * p - d * (kw - 1) - 1) // s + 1
    xp = torch.zeros(B, C, IH + 2 * p, IW + 2 * p, dtype=torch.float64)
    xp[:, :, p:p + IH, p:p + IW] = x
    out = torch.zeros(B, M, OH, OW, dtype=torch.float64)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, :, ky * d: ky * d + (OH - 1) * s + 1: s, kx * d: kx * d + (OW - 1) * s + 1: s]
            out += torch.einsum("mc,bchw->bmhw", wmc[:, :, ky, kx], win)
    return out


def convT2d_ref(x, wmc, s, p, d, op):
    """out[b, m, iy s - p + ky d, ix s - p + kx d] += x[b, c, iy, ix] w[m, c, ky, kx]; output size
    (I - 1) s - 2 p + d (k - 1) + op + 1"""
    B, C, IH, IW = x.shape
    M, _, kh, kw = wmc.shape
    FH = (IH - 1) * s + d * (kh - 1) + 1 + op
    FW = (IW - 1) * s + d * (kw - 1) + 1 + op
    full = torch.zeros(B, M, FH, FW, dtype=torch.float64)
    for ky in range(kh):
        for kx in range(kw):
            full[:, :, ky * d: ky * d + (IH - 1) * s + 1: s, kx * d: kx * d + (IW - 1) * s + 1: s] += \
                torch.einsum("mc,bchw->bmhw", wmc[:, :, ky, kx], x)
    return full[:, :, p:FH - p, p:FW - p].contiguous()


def pool2_ref(x):
    """2x2 average of the double-resolution input (the pooled load of a pool=True segment)"""
    B, C, H2, W2 = x.shape
    return x.double().reshape(B, C, H2 // 2, 2, W2 // 2, 2).sum(dim=(3, 5)) * 0.25


def seg_ref(sg, x, w, layout, gate=None):
    """one segment of a job: pool, gate, then the taps of its kind"""
    x = pool2_ref(x) if sg.pool else x.double()
    assert tuple(x.shape[1:]) == (sg.C, sg.IH, sg.IW), (x.shape, sg)
    if gate is not None:
        x = x * gate.double().reshape(x.shape[0], sg.C, 1, 1)
    wmc = _weight_mc(w, layout)
    if sg.kind == "conv":
        return conv2d_ref(x, wmc, sg.s, sg.p, sg.d)
    if sg.kind == "convT":
        return convT2d_ref(x, wmc, sg.s, sg.p, sg.d, sg.op)
    assert sg.kind == "pw" and wmc.shape[2:] == (1, 1)
    return torch.einsum("mc,bchw->bmhw", wmc[:, :, 0, 0], x)


def conv_job_ref(segs, xs, ws, layouts, gates=None, bias=None, addend=None, act=0, act_param=SLOPE):
    """(pre, out): the sum over segments, + bias[m] + addend, and its activation"""
    gates = gates or [None] * len(segs)
    pre = sum(seg_ref(sg, x, w, lay, g) for sg, x, w, lay, g in zip(segs, xs, ws, layouts, gates))
    if bias is not None:
        pre = pre + bias.double()[None, :, None, None]
    if addend is not None:
        pre = pre + addend.double()
    return pre, act64(pre, act, act_param)


def convt_k4s2_ref(x0, w0, x1=None, w1=None, bias=None, act=0, act_param=SLOPE):
    """ffc_convt_k4s2_smallm: act(conv_t(x0; w0) [+ conv_t(x1; w1)] + bias), ConvTranspose2d k4 s2 p1,
    weights (C, M, 4, 4)"""
    pre = convT2d_ref(x0.double(), _weight_mc(w0, 1), 2, 1, 1, 0)
    if x1 is not None:
        pre = pre + convT2d_ref(x1.double(), _weight_mc(w1, 1), 2, 1, 1, 0)
    if bias is not None:
        pre = pre + bias.double()[None, :, None, None]
    return act64(pre, act, act_param)


def in_tf_ref(x, tf):
    """ffc_in_tf: act(x * scale[c] + shift[c]) + noise_w[c] * noise[b, 0, y, x] (tf None: x as stored);
    tf = dict(scale, shift, act, act_param, noise_w, noise), noise (B, 1, H, W) or None"""
    x = x.double()
    if tf is None:
        return x
    y = act64(x * tf["scale"].double()[None, :, None, None] + tf["shift"].double()[None, :, None, None],
              tf["act"], tf.get("act_param", SLOPE))
    if tf.get("noise") is not None:
        y = y + tf["noise_w"].double()[None, :, None, None] * tf["noise"].double()
    return y


def conv3x3_ref(x0, w0, x1=None, w1=None, bias=None, act=0, act_param=SLOPE, tf0=None, tf1=None):
    """ffc_conv3x3_smallm(_tf): each segment through its input transform (the zero padding belongs to
    the transformed tensor), Conv2d k3 s1 p1 with weights (M, C, 3, 3), + bias, activation"""
    pre = conv2d_ref(in_tf_ref(x0, tf0), w0.double(), 1, 1, 1)
    if x1 is not None:
        pre = pre + conv2d_ref(in_tf_ref(x1, tf1), w1.double(), 1, 1, 1)
    if bias is not None:
        pre = pre + bias.double()[None, :, None, None]
    return act64(pre, act, act_param)


# --------------------------------------------------------------------------- packers
def split_bf16_ref(x):
    """fp32 array -> three uint16 planes (hi, mid, lo) by truncation, ffc_split_bf16 / split3: hi = the
    top 16 bits of x, mid = the top 16 bits of x - hi, lo = the top 16 bits of x - hi - mid.  Every
    subtraction is exact in fp32 (24 significand bits = 8 + 8 + 8), so the last truncation drops nothing
    for normal numbers: hi + mid + lo == x."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    planes = []
    for _ in range(3):
        top = a.view(np.uint32) & np.uint32(0xFFFF0000)
        planes.append((top >> np.uint32(16)).astype(np.uint16))
        a = a - top.view(np.float32)
    return planes


def bf16_to_f64(p):
    """uint16 bf16 bit patterns -> float64 values"""
    return (np.asarray(p).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def phase_table(plan, pi):
    """(kt_off, K, Kpad, a_off) of phase pi for both plan kinds (JobPlan / PatchPlan)"""
    ph = plan.phases[pi]
    if isinstance(ph, dict):
        return ph["kt_off"], ph["K"], ph["Kpad"], ph["a_off"]
    return plan.kt_off[pi], ph.K, ph.Kpad, plan.a_off[pi]


def pack_ref(plan, ws, layouts):
    """the packed weight buffer of ffc_conv_pack as a flat float32 array of plan.a_size elements:
    A[phase][Mpad][Kpad], element (m, k) the weight the phase's k-table entry k names ((segment,
    channel, ky, kx); segment 15 = padding), zero for m >= M and k >= K"""
    A = np.zeros(plan.a_size, dtype=np.float32)
    wmc = [np.asarray(_weight_mc(w, lay).float()) for w, lay in zip(ws, layouts)]
    for pi in range(len(plan.phases)):
        kt_off, K, Kpad, a_off = phase_table(plan, pi)
        a = np.zeros((plan.Mpad, Kpad), dtype=np.float32)
        for k, (sx, _, _, kk) in enumerate(plan.ktab[kt_off: kt_off + K]):
            if (sx & 15) == 15:
                continue
            a[:plan.M, k] = wmc[sx & 15][:, sx >> 4, kk & 0xFFFF, kk >> 16]
        A[a_off: a_off + a.size] = a.reshape(-1)
    return A


def unpack_a3(plan, A3):
    """ffc_convq_pack_a3's fragment order inverted (include/ffc_amd.h): element
    3 a_off + ((mtile Kpad/16 + kstep) 3 + piece) 512 + lane 8 + j is piece `piece` of
    A[32 mtile + (lane & 31)][16 kstep + 8 (lane >> 5) + j] -> three uint16 arrays laid out like A"""
    A3 = np.asarray(A3).view(np.uint16)
    out = [np.zeros(plan.a_size, dtype=np.uint16) for _ in range(3)]
    for pi in range(len(plan.phases)):
        _, _, Kpad, a_off = phase_table(plan, pi)
        mt, ks = plan.Mpad // 32, Kpad // 16
        fr = A3[3 * a_off: 3 * a_off + mt * ks * 1536].reshape(mt, ks, 3, 2, 32, 8)   # mtile, kstep, piece, half, row, j
        for piece in range(3):
            a = fr[:, :, piece].transpose(0, 3, 1, 2, 4).reshape(plan.Mpad, Kpad)     # (mtile, row), (kstep, half, j)
            out[piece][a_off: a_off + a.size] = a.reshape(-1)
    return out


# --------------------------------------------------------------------------- input builders
def randn(shape, gen):
    return torch.randn(shape, generator=gen)


def _taps(sg):
    """taps of a segment that meet one output pixel (its fan-in per channel)"""
    return max(1, sg.k * sg.k // (sg.s * sg.s)) if sg.kind == "convT" else sg.k * sg.k


def job_inputs(B, M, segs, OH, OW, seed=0, bias=False, addend=False):
    """O(1) normal inputs, weights scaled by 1 / sqrt(fan-in of the whole job) so that the output is O(1),
    gates in [0.25, 1] for gated segments, optional bias / addend.  No zeros are planted.
    -> dict(xs, ws, layouts, gates, bias, addend); weights in the layout of their nn module (convT:
    (C, M, k, k), layout 1; conv / pw: (M, C, k, k), layout 0)"""
    gen = torch.Generator().manual_seed(seed)
    fan = sum(sg.C * _taps(sg) for sg in segs)
    xs, ws, layouts, gates = [], [], [], []
    for sg in segs:
        r = 2 if sg.pool else 1
        xs.append(randn((B, sg.C, sg.IH * r, sg.IW * r), gen))
        shape = (sg.C, M, sg.k, sg.k) if sg.kind == "convT" else (M, sg.C, sg.k, sg.k)
        ws.append(randn(shape, gen) / fan ** 0.5)
        layouts.append(1 if sg.kind == "convT" else 0)
        gates.append(0.25 + 0.75 * torch.rand((B, sg.C), generator=gen) if sg.gate else None)
    return dict(xs=xs, ws=ws, layouts=layouts, gates=gates,
                bias=randn((M,), gen) if bias else None,
                addend=randn((B, M, OH, OW), gen) if addend else None)


def smallm_inputs(B, C0, C1, M, H, W, k, transposed, seed=0, bias=False):
    """inputs of the small-M entry points: x0 (B, C0, H, W) [, x1 (B, C1, H, W)], weights (C, M, k, k) when
    transposed else (M, C, k, k), scaled by 1 / sqrt(fan-in)"""
    gen = torch.Generator().manual_seed(seed)
    taps = k * k // 4 if transposed else k * k
    fan = (C0 + C1) * taps
    xs = [randn((B, C, H, W), gen) for C in (C0, C1) if C]
    ws = [randn((C, M, k, k) if transposed else (M, C, k, k), gen) / fan ** 0.5 for C in (C0, C1) if C]
    return dict(x0=xs[0], w0=ws[0], x1=xs[1] if C1 else None, w1=ws[1] if C1 else None,
                bias=randn((M,), gen) if bias else None)


def tf_inputs(B, C, H, W, act, noise, gen):
    """an ffc_in_tf: scale near 1, small shift, optional NoiseInjection weight and (B, 1, H, W) noise"""
    return dict(scale=1 + 0.2 * randn((C,), gen), shift=0.1 * randn((C,), gen), act=act, act_param=SLOPE,
                noise_w=randn((C,), gen) if noise else None, noise=randn((B, 1, H, W), gen) if noise else None)


def split_inputs(n, seed=0):
    """the first n of: values whose low mantissa bits are all set (either sign), zeros, powers of two,
    negatives, then normal draws"""
    ones = np.array([0x3F80FFFF, 0xBFFFFFFF, 0x40FFFFFF, 0x3F7FFFFF, 0xC2000001, 0x3F8000FF, 0x3F80FF01],
                    dtype=np.uint32).view(np.float32)
    special = np.array([0.0, -0.0, 1.0, -2.0, 2.0 ** -20, 2.0 ** 20, -(2.0 ** -7)], dtype=np.float32)
    draws = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    return np.concatenate([ones, special, draws])[:n].copy()
