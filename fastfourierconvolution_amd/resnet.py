"""The ResNet SNGAN family of fgan128_complete.py:75-438 on the HIP ops: GBlock, DBlock, DBlockOptimized,
SNGANGenerator128 and SNGANDiscriminator128 -- the 128x128 baseline the FFC FGenerator / Discriminator of the
same script are compared against.  Constructor signatures, attributes, initialisation and state_dict keys are
the reference's: every conv of both models sits under hook-style torch.nn.utils.spectral_norm whatever the
``spectral_norm`` argument says (weight_orig / weight_u / weight_v), as the reference builds them.

What runs (no torch compute):

  GBlock   b1 + ReLU + bilinear x2   ffc::bn_act_up2b: one pass, the activated low-resolution tensor is never
                                     written (conditional: ffc::cbn_act, then ffc::up2_bilinear)
           c1                        one ffc::conv_layer job
           b2 + ReLU                 ffc::bn_act / ffc::cbn_act
           c2 + shortcut             ONE two-segment job: c2 (3x3) on h plus c_sc (1x1, a 'pw' segment) on the
                                     upsampled x (ffc::up2_bilinear in its plain form); both biases ride in the job
  DBlock   out = pool(c2(relu(c1(a))) + c_sc(a)), a = relu(x): the reference's leading nn.ReLU(True) acts on x
           itself before the shortcut reads it, so the shortcut sees relu(x).  Pooling is linear, so the block is
           c1 (ReLU in the epilogue), one two-segment job c2 + c_sc at the input resolution, and ONE pooling launch
           (ffc::pool2_act, which applies the next block's ReLU inside a model).  The identity shortcut (block6)
           is the job's addend.  The caller's tensor is not written: a comes from ffc::act, or from the previous
           block's pool2_act.
  DBlockOptimized   c1 (ReLU), then c2 + c_sc(x) as one job (c_sc(pool(x)) = pool(c_sc(x))) and one pooling launch
  critic tail       torch.sum(relu(h), (2, 3)) on ffc::relu_sum_pool, l7 on the 1x1 GEMM job

A down-sampling block on an odd plane raises NotImplementedError (the reference floors); CPU and non-fp32
tensors are refused as everywhere in the package (there is no CPU fallback).
"""
import math

import torch
import torch.nn as nn

from . import _autograd as ag
from . import _plan
from . import _runtime as rt
from .ffc import ConditionalBatchNorm2d
from .models import FFCModel

RELU = (1, 0.0)
IDENT = (0, 0.0)
TANH = (3, 0.0)


def _conv3(mod, x):
    B, C, H, W = x.shape
    if C != mod.in_channels:
        raise RuntimeError(f"expected input with {mod.in_channels} channels, got {C}")
    return _plan.Seg("conv", C, H, W, 3, 1, 1)


def _pw(mod, x):
    B, C, H, W = x.shape
    if C != mod.in_channels:
        raise RuntimeError(f"expected input with {mod.in_channels} channels, got {C}")
    return _plan.Seg("pw", C, H, W)


def _conv(mod, x, act=IDENT):
    """one Conv2d(k3, s1, p1) with its bias and ``act`` in the epilogue"""
    (y,) = ag.conv_layer(x.shape[0], [(mod.out_channels,) + tuple(act)], [(0, 0, _conv3(mod, x), mod)], [x])
    return y


def _conv_plus(c2, h, c_sc, s, addend=None):
    """c2(h) + c_sc(s) [+ addend] as one job: the 3x3 segment and the block's 1x1 shortcut as a 'pw' segment at the
    same resolution (their biases are summed when the job's weights are packed), or the identity shortcut as
    the job's addend"""
    edges, inputs, adds = [(0, 0, _conv3(c2, h), c2)], [h], None
    if c_sc is not None:
        edges.append((0, 1, _pw(c_sc, s), c_sc))
        inputs.append(s)
    elif addend is not None:
        inputs.append(addend)
        adds = [(0, 1)]
    (y,) = ag.conv_layer(h.shape[0], [(c2.out_channels,) + IDENT], edges, inputs, adds)
    return y


def _sn_convs(block):
    return [m for m in (block.c1, block.c2, getattr(block, "c_sc", None)) if m is not None]


class GBlock(nn.Module):
    """fgan128_complete.py:75-205: the generator's residual block, b1 -> ReLU -> [bilinear x2] -> c1 -> b2 -> ReLU
    -> c2, plus the shortcut [bilinear x2 ->] c_sc (``learnable_sc``: in != out or upsample), else x.
    ``num_classes`` > 0: b1 / b2 are ConditionalBatchNorm2d and the call is ``forward(x, y)``."""

    def __init__(self, in_channels, out_channels, hidden_channels=None, upsample=False, num_classes=0,
                 spectral_norm=False):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.hidden_channels = hidden_channels if hidden_channels is not None else out_channels
        self.learnable_sc = in_channels != out_channels or upsample
        self.upsample = upsample
        self.num_classes = num_classes
        self.spectral_norm = spectral_norm
        sn_fn = torch.nn.utils.spectral_norm
        self.c1 = sn_fn(nn.Conv2d(self.in_channels, self.hidden_channels, 3, 1, padding=1))
        self.c2 = sn_fn(nn.Conv2d(self.hidden_channels, self.out_channels, 3, 1, padding=1))
        if self.num_classes == 0:
            self.b1 = nn.BatchNorm2d(self.in_channels)
            self.b2 = nn.BatchNorm2d(self.hidden_channels)
        else:
            self.b1 = ConditionalBatchNorm2d(self.in_channels, self.num_classes)
            self.b2 = ConditionalBatchNorm2d(self.hidden_channels, self.num_classes)
        self.activation = nn.ReLU(True)
        nn.init.xavier_uniform_(self.c1.weight.data, math.sqrt(2.0))
        nn.init.xavier_uniform_(self.c2.weight.data, math.sqrt(2.0))
        if self.learnable_sc:
            self.c_sc = sn_fn(nn.Conv2d(in_channels, out_channels, 1, 1, padding=0))
            nn.init.xavier_uniform_(self.c_sc.weight.data, 1.0)

    def forward(self, x, y=None):
        x = rt.require(x, "x")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"GBlock: x must be (B, {self.in_channels}, H, W), got {tuple(x.shape)}")
        cond = isinstance(self.b1, ConditionalBatchNorm2d)
        if cond != (y is not None):
            raise TypeError("GBlock: labels go with num_classes > 0 (forward(x, y)) and only with it")
        with rt.sn_batch(_sn_convs(self)):
            if cond:
                h = ag.cbn_act(self.b1, x, y, RELU)
                if self.upsample:
                    h = torch.ops.ffc.up2_bilinear(h, None, None, 0, 0.0)
            elif self.upsample:
                h = ag.bn_act_up2b(self.b1, x, RELU)
            else:
                h = ag.bn_act(self.b1, x, RELU)
            h = _conv(self.c1, h)
            h = ag.cbn_act(self.b2, h, y, RELU) if cond else ag.bn_act(self.b2, h, RELU)
            if not self.learnable_sc:
                return _conv_plus(self.c2, h, None, None, addend=x)
            s = torch.ops.ffc.up2_bilinear(x, None, None, 0, 0.0) if self.upsample else x
            return _conv_plus(self.c2, h, self.c_sc, s)


class DBlock(nn.Module):
    """fgan128_complete.py:208-278: the critic's residual block.  With a = relu(x) (see the module docstring):
    out = [pool](c2(relu(c1(a))) + c_sc(a)), or + a itself without ``learnable_sc``."""

    def __init__(self, in_channels, out_channels, hidden_channels=None, downsample=False, spectral_norm=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.hidden_channels = hidden_channels if hidden_channels is not None else in_channels
        self.downsample = downsample
        self.learnable_sc = (in_channels != out_channels) or downsample
        self.spectral_norm = spectral_norm
        sn_fn = torch.nn.utils.spectral_norm
        self.c1 = sn_fn(nn.Conv2d(self.in_channels, self.hidden_channels, 3, 1, 1))
        self.c2 = sn_fn(nn.Conv2d(self.hidden_channels, self.out_channels, 3, 1, 1))
        self.activation = nn.ReLU(True)
        nn.init.xavier_uniform_(self.c1.weight.data, math.sqrt(2.0))
        nn.init.xavier_uniform_(self.c2.weight.data, math.sqrt(2.0))
        if self.learnable_sc:
            self.c_sc = sn_fn(nn.Conv2d(in_channels, out_channels, 1, 1, 0))
            nn.init.xavier_uniform_(self.c_sc.weight.data, 1.0)

    def run(self, a, act_out=IDENT):
        """the block on a = relu(x) -> act_out(block output): act_out = ReLU hands the next DBlock its ``a``"""
        if a.dim() != 4 or a.shape[1] != self.in_channels:
            raise RuntimeError(f"DBlock: x must be (B, {self.in_channels}, H, W), got {tuple(a.shape)}")
        if self.downsample and (a.shape[2] % 2 or a.shape[3] % 2):
            raise NotImplementedError(f"DBlock: AvgPool2d(2) of an odd {a.shape[2]}x{a.shape[3]} plane (the "
                                      "reference floors)")
        h = _conv(self.c1, a, RELU)
        if self.learnable_sc:
            h = _conv_plus(self.c2, h, self.c_sc, a)
        else:
            h = _conv_plus(self.c2, h, None, None, addend=a)
        if self.downsample:
            return torch.ops.ffc.pool2_act(h, int(act_out[0]), float(act_out[1]))
        return h if act_out[0] == 0 else torch.ops.ffc.act(h, int(act_out[0]), float(act_out[1]))

    def forward(self, x):
        x = rt.require(x, "x")
        if x.dim() != 4:
            raise RuntimeError(f"DBlock: x must be (B, {self.in_channels}, H, W), got {tuple(x.shape)}")
        with rt.sn_batch(_sn_convs(self)):
            return self.run(torch.ops.ffc.act(x, 1, 0.0))


class DBlockOptimized(nn.Module):
    """fgan128_complete.py:281-332: the critic's first block, pool(c2(relu(c1(x)))) + c_sc(pool(x)) -- no leading
    ReLU.  c_sc(pool(x)) = pool(c_sc(x)): one two-segment job at the input resolution and one pooling launch."""

    def __init__(self, in_channels, out_channels, spectral_norm=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.spectral_norm = spectral_norm
        sn_fn = torch.nn.utils.spectral_norm
        self.c1 = sn_fn(nn.Conv2d(self.in_channels, self.out_channels, 3, 1, 1))
        self.c2 = sn_fn(nn.Conv2d(self.out_channels, self.out_channels, 3, 1, 1))
        self.c_sc = sn_fn(nn.Conv2d(self.in_channels, self.out_channels, 1, 1, 0))
        self.activation = nn.ReLU(True)
        nn.init.xavier_uniform_(self.c1.weight.data, math.sqrt(2.0))
        nn.init.xavier_uniform_(self.c2.weight.data, math.sqrt(2.0))
        nn.init.xavier_uniform_(self.c_sc.weight.data, 1.0)

    def run(self, x, act_out=IDENT):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"DBlockOptimized: x must be (B, {self.in_channels}, H, W), got {tuple(x.shape)}")
        if x.shape[2] % 2 or x.shape[3] % 2:
            raise NotImplementedError(f"DBlockOptimized: AvgPool2d(2) of an odd {x.shape[2]}x{x.shape[3]} plane (the "
                                      "reference floors)")
        h = _conv(self.c1, x, RELU)
        h = _conv_plus(self.c2, h, self.c_sc, x)
        return torch.ops.ffc.pool2_act(h, int(act_out[0]), float(act_out[1]))

    def forward(self, x):
        x = rt.require(x, "x")
        with rt.sn_batch(_sn_convs(self)):
            return self.run(x)


class SNGANGenerator128(FFCModel):
    """fgan128_complete.py:335-387: l1 = Linear(nz, bottom_width^2 * ngf) -> (ngf, bw, bw) -> five up-sampling
    GBlocks (ngf -> ngf -> ngf/2 -> ngf/4 -> ngf/8 -> ngf/16, planes x32) -> b7 + ReLU -> c7 = Conv2d(ngf/16, 3, 3,
    1, 1) + tanh: a (B, 3, 32 bw, 32 bw) float image in train and eval mode alike (the reference has no uint8
    branch here).  c7 carries no spectral norm; every GBlock conv does."""

    def __init__(self, nz=128, ngf=1024, bottom_width=4, **kwargs):
        super().__init__()
        self.nz = nz
        self.ngf = ngf
        self.bottom_width = bottom_width
        self.l1 = nn.Linear(self.nz, (self.bottom_width ** 2) * self.ngf)
        self.block2 = GBlock(self.ngf, self.ngf, upsample=True)
        self.block3 = GBlock(self.ngf, self.ngf >> 1, upsample=True)
        self.block4 = GBlock(self.ngf >> 1, self.ngf >> 2, upsample=True)
        self.block5 = GBlock(self.ngf >> 2, self.ngf >> 3, upsample=True)
        self.block6 = GBlock(self.ngf >> 3, self.ngf >> 4, upsample=True)
        self.b7 = nn.BatchNorm2d(self.ngf >> 4)
        self.c7 = nn.Conv2d(self.ngf >> 4, 3, 3, 1, padding=1)
        self.activation = nn.ReLU(True)
        nn.init.xavier_uniform_(self.l1.weight.data, 1.0)
        nn.init.xavier_uniform_(self.c7.weight.data, 1.0)

    def _blocks(self):
        return (self.block2, self.block3, self.block4, self.block5, self.block6)

    def forward(self, x):
        x = rt.require(x, "z")
        if x.dim() != 2 or x.shape[1] != self.nz:
            raise RuntimeError(f"SNGANGenerator128: z must be (B, {self.nz}), got {tuple(x.shape)}")
        if ag.wants_grad(self.l1, x):
            h = ag.linear(self.l1, x)
        else:
            h = torch.ops.ffc.linear(x, self.l1.weight, self.l1.bias)
        h = h.view(x.shape[0], -1, self.bottom_width, self.bottom_width)
        with rt.sn_batch([m for b in self._blocks() for m in _sn_convs(b)]):   # set_sn_hip: all 15 convs, one table
            for block in self._blocks():
                h = block(h)
            h = ag.bn_act(self.b7, h, RELU)
            return _conv(self.c7, h, TANH)


class SNGANDiscriminator128(FFCModel):
    """fgan128_complete.py:390-438: DBlockOptimized(3, ndf/16), four down-sampling DBlocks up to ndf, DBlock(ndf,
    ndf) without down-sampling, ReLU, global sum pooling, l7 = Linear(ndf, 1) under spectral norm: logits (B, 1).
    Any (B, 3, H, W) whose planes stay even through the five poolings."""

    def __init__(self, ndf=1024, **kwargs):
        super().__init__()
        self.ndf = ndf
        sn_fn = torch.nn.utils.spectral_norm
        self.block1 = DBlockOptimized(3, self.ndf >> 4)
        self.block2 = DBlock(self.ndf >> 4, self.ndf >> 3, downsample=True)
        self.block3 = DBlock(self.ndf >> 3, self.ndf >> 2, downsample=True)
        self.block4 = DBlock(self.ndf >> 2, self.ndf >> 1, downsample=True)
        self.block5 = DBlock(self.ndf >> 1, self.ndf, downsample=True)
        self.block6 = DBlock(self.ndf, self.ndf, downsample=False)
        self.l7 = sn_fn(nn.Linear(self.ndf, 1))
        self.activation = nn.ReLU(True)
        nn.init.xavier_uniform_(self.l7.weight.data, 1.0)

    def _blocks(self):
        return (self.block1, self.block2, self.block3, self.block4, self.block5, self.block6)

    def forward(self, x):
        x = rt.require(x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"SNGANDiscriminator128: x must be (B, 3, H, W), got {tuple(x.shape)}")
        with rt.sn_batch([m for b in self._blocks() for m in _sn_convs(b)] + [self.l7]):
            a = x
            for block in self._blocks()[:-1]:   # every block hands the next one relu(its output)
                a = block.run(a, RELU)
            h = self.block6.run(a)
            return ag.linear(self.l7, torch.ops.ffc.relu_sum_pool(h))   # :432-436
