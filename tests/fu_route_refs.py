"""float64 restatement, with state, of what one row of tests/fu_route_cases.py computes: the outputs of
three calls and the BatchNorm buffers they leave behind, in the reference project's order of operations
(layers/ffc/fourier_unity.py:32-56, layers/ffc/spectral_transform.py:77-110), shared by
test_fu_route_refs_cpu.py (the restatement against the oracle, the bound rule, planted defects) and
test_gpu_fu_route_values.py (the package against the restatement, row by row).

Plain torch on the CPU; nothing here imports the package under test.  The BatchNorms are torch.nn.BatchNorm2d
modules, so the running statistics, momentum=None (the cumulative average) and num_batches_tracked are
torch's own; the FFTs are torch.fft.rfftn / irfftn (norm="ortho"), the rest F.conv2d, F.interpolate(nearest)
and F.avg_pool2d.  The quadrant stack of the local Fourier unit is lfu_refs.lfu_split / lfu_tile.

    'fu' rows, FourierUnitSN._run(t, up=up):     s = t nearest-upsampled by up
                                                 out = irfftn(relu(bn(mix(rfftn(s)))))
    'st' rows, SpectralTransform.spectral(x):    s = relu(bn1(conv1(se(upsample or pool(x)))))
                                                 out = s + fu(s) [+ tile(lfu(quadrants of s)) with run_lfu]

The package runs SE, conv1 and bn1 in front of the x2 upsample (they commute with it) and corrects bn1's
unbiased variance by count_mult = 4; the restatement upsamples first, so that equivalence is part of what a
comparison checks.  fp16 rows are restated with exact products: the rounding of the operands is what their
wider bound covers.

Geometry as in test_gpu_fu_route.build (SpectralTransform(16, 2C, ...), square planes), with one addition:
every 'st' module is built with enable_lfu=True, so that lfu.bn exists in the rows that do not run it and
"left alone" can be asserted; run_lfu is the row's.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import lfu_refs
from fu_route_cases import ROWS

CALLS = 3
# the bounds the GPU rows are held to (test_gpu_fu_route_values.py); the float32 CPU restatement has to stay
# within ROOM of each (test_fu_route_refs_cpu.py), the rule of optim_refs / convlayer_refs
OUT_TOL = {"fp32": 1e-5, "fp16": 2e-3}     # normwise; fp16: the one-unit gate of test_gpu_sn_fp16.py
BUF_RTOL, BUF_ATOL = 1e-5, 1e-6            # the project's criterion for slab statistics
F16_BUF_TOL = 2e-3                         # the unit's BN of an fp16 train row: rtol, and atol as a share of max|ref|
ROOM = 0.25
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")

# one seed per row (state and input); a row that broke the bound rule would get another one here
SEEDS = {r.id: 1000 + 7 * i for i, r in enumerate(ROWS)}

DEFECTS = ("bn1_count", "fu_bn_twice", "skip:bn1", "skip:fu.bn", "skip:lfu.bn", "momentum_01", "eval_batch_stats",
           "no_residual", "lfu_order", "lfu_bn_bump")


def _bn(bn, x, name, defect):
    """bn(x), or what a planted defect makes of it"""
    if defect == "eval_batch_stats" and not bn.training:
        return F.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)
    if defect == "skip:" + name and bn.training:      # normalised as it should be, the buffers never touched
        return F.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)
    if defect == "fu_bn_twice" and name == "fu.bn":
        bn(x)
    return bn(x)


class FuRef(nn.Module):
    """FourierUnitSN (fourier_unity.py:17-56, y=None): same submodule names and state_dict keys"""

    def __init__(self, C):
        super().__init__()
        self.conv_layer = nn.Conv2d(2 * C, 2 * C, 1, bias=False)
        self.bn = nn.BatchNorm2d(2 * C)

    def forward(self, s, name="fu.bn", defect=None):
        B, C, H, W = s.shape
        X = torch.fft.rfftn(s, dim=(-2, -1), norm="ortho")
        Z = torch.stack((X.real, X.imag), dim=2).reshape(B, 2 * C, H, W // 2 + 1)   # channel 2c = Re, 2c + 1 = Im
        Y = F.relu(_bn(self.bn, F.conv2d(Z, self.conv_layer.weight), name, defect))
        Y = Y.reshape(B, C, 2, H, W // 2 + 1)
        return torch.fft.irfftn(torch.complex(Y[:, :, 0], Y[:, :, 1]), s=(H, W), dim=(-2, -1), norm="ortho")


class SERef(nn.Module):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction, bias=False), nn.ReLU(),
                                nn.Linear(channel // reduction, channel, bias=False), nn.Sigmoid())

    def forward(self, x):
        return x * self.fc(x.mean(dim=(2, 3)))[:, :, None, None]


class StRef(nn.Module):
    """SpectralTransform up to conv2 (spectral_transform.py:36-108), the local Fourier unit as the comment at
    :94-105 states it; submodules registered in the package's order, so the state_dict keys line up"""

    def __init__(self, cin, C, stride, upsample):
        super().__init__()
        self.stride, self.upsample = stride, upsample
        self.conv1 = nn.Conv2d(cin, C, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(C)
        self.fu = FuRef(C)
        self.lfu = FuRef(C)
        self.conv2 = nn.Conv2d(C, 2 * C, 1, bias=False)
        self.se_block = SERef(cin)
        self.run_lfu = False

    def resample(self, x):
        if self.stride == 2 and self.upsample:
            return F.interpolate(x, scale_factor=2, mode="nearest")
        return F.avg_pool2d(x, 2, 2) if self.stride == 2 else x

    def from_t(self, t, defect=None):
        """from conv1's output on: s = relu(bn1(t)), then the Fourier units and the residual"""
        s = F.relu(_bn(self.bn1, t, "bn1", defect))
        v = self.fu(s, "fu.bn", defect)
        if defect != "no_residual":
            v = s + v
        if self.run_lfu:
            xs = lfu_refs.lfu_split(s)
            if defect == "lfu_order":      # the halves along W stacked first, then those along H
                H, W = s.shape[-2:]
                xs = torch.cat(torch.split(s[:, :s.shape[1] // 4], W // 2, dim=-1), dim=1)
                xs = torch.cat(torch.split(xs, H // 2, dim=-2), dim=1).contiguous()
            v = v + lfu_refs.lfu_tile(self.lfu(xs, "lfu.bn", defect))
        elif defect == "lfu_bn_bump" and self.training:
            self.lfu.bn.num_batches_tracked += 1
        return v

    def forward(self, x, defect=None):
        if defect == "bn1_count" and self.stride == 2 and self.upsample:
            # SE, conv1 and bn1 at the input resolution and no count correction: the same output, and an
            # unbiased variance over a quarter of the samples
            t = self.conv1(self.se_block(x))
            s = self.resample(F.relu(_bn(self.bn1, t, "bn1", defect)))
            return s + self.fu(s, "fu.bn", defect)
        return self.from_t(self.conv1(self.se_block(self.resample(x))), defect)


def build(row):
    """the restatement's module of a row, float64, untrained state"""
    if row.kind == "fu":
        return FuRef(row.C).double()
    stride = 2 if (row.pool or row.up == 2) else 1
    return StRef(16, row.C, stride, row.up == 2).double()


def input_shape(row):
    if row.kind == "fu":
        return (row.B, row.C, row.H // row.up, row.H // row.up)
    h = row.H * 2 if row.pool else row.H // row.up
    return (row.B, 16, h, h)


def from_row(row, seed=None):
    """-> (state, x): a float32 state_dict of CPU tensors under the package module's keys (BN affine away from
    1 / 0, randomised running statistics, num_batches_tracked 0: lfu_refs.random_state) and the float32 input"""
    seed = SEEDS[row.id] if seed is None else seed
    state = lfu_refs.random_state(build(row), seed, running=True)
    x = torch.randn(input_shape(row), generator=torch.Generator().manual_seed(seed + 500))
    return state, x


def bn_names(row):
    return ("bn",) if row.kind == "fu" else ("bn1", "fu.bn", "lfu.bn")


def buffers_of(state, row):
    return {f"{bn}.{k}": state[f"{bn}.{k}"].clone() for bn in bn_names(row) for k in BN_BUFFERS}


def run(row, state, x, calls=CALLS, dtype=torch.float64, defect=None):
    """-> (outs, buffers): the output of every call and the buffers of every BN after the last, the module in the
    row's mode throughout.  dtype=torch.float32: the same graph in float32 (the bound rule); defect: one of
    DEFECTS planted in it"""
    assert defect is None or defect in DEFECTS, defect
    mod = build(row)
    mod.load_state_dict(state)
    mod = mod.to(dtype).train(row.train)
    x = x.to(dtype)
    if row.kind == "st":
        mod.run_lfu = row.lfu
        mod.bn1.momentum = None if (row.momentum_none and defect != "momentum_01") else 0.1
    outs = []
    with torch.no_grad():
        for _ in range(calls):
            if row.kind == "fu":
                s = F.interpolate(x, scale_factor=row.up, mode="nearest") if row.up > 1 else x
                outs.append(mod(s, "fu.bn", defect))
            else:
                outs.append(mod(x, defect))
    return outs, buffers_of(mod.state_dict(), row)


def run_from_t(C, state, t, calls=CALLS, dtype=torch.float64):
    """FourierUnitSN._run(t, in_relu=True, residual=True, in_fold=<bn1 over t's own statistics>): relu(bn1(t))
    through the unit plus the residual; `state` of an 'st' row with C channels (bn1.* and fu.* are used)"""
    mod = StRef(16, C, 1, False).double()
    mod.load_state_dict(state)
    mod = mod.to(dtype).train()
    with torch.no_grad():
        outs = [mod.from_t(t.to(dtype)) for _ in range(calls)]
    sd = mod.state_dict()
    return outs, {f"{bn}.{k}": sd[f"{bn}.{k}"].clone() for bn in ("bn1", "fu.bn") for k in BN_BUFFERS}


# --------------------------------------------------------------------------- bounds and shares
def is_unit_bn(row, key):
    return key.startswith("bn." if row.kind == "fu" else "fu.bn.")


def buffer_tol(row, key, ref):
    """(rtol, atol) of one running_mean / running_var"""
    if row.mix == "fp16" and row.train and is_unit_bn(row, key):
        return F16_BUF_TOL, F16_BUF_TOL * ref.abs().max().item()
    return BUF_RTOL, BUF_ATOL


def normwise(a, ref):
    den = ref.abs().max().item()
    return (a.double() - ref.double()).abs().max().item() / (den if den > 0 else 1.0)


def shares(row, got, ref):
    """error over bound of every tensor: {'out<i>': normwise / OUT_TOL, '<bn>.running_*': max |d| / (atol +
    rtol |ref|), '<bn>.num_batches_tracked': 0 or inf}; got, ref: (outs, buffers) as run() returns them"""
    out = {}
    for i, (a, r) in enumerate(zip(got[0], ref[0])):
        out[f"out{i}"] = float("inf") if torch.isnan(a).any() else normwise(a, r) / OUT_TOL[row.mix]
    for key, r in ref[1].items():
        a = got[1][key]
        if key.endswith("num_batches_tracked"):
            out[key] = 0.0 if int(a) == int(r) else float("inf")
            continue
        rtol, atol = buffer_tol(row, key, r)
        out[key] = ((a.double() - r.double()).abs() / (atol + rtol * r.double().abs())).max().item()
    return out
