"""The custom-op boundary: every launch of the FFC hot path is reached through a ``torch.ops.ffc.*``
op registered with ``torch.library.custom_op``, over the C ABI of libffc_amd.so
(include/ffc_amd.h).  Each op has a fake (meta) implementation, so FakeTensor tracing,
``torch.export`` and ``torch.library.opcheck`` see the path; the training ops carry their backward
through ``register_autograd`` (the backward is another ffc op).

Training ops (autograd): one per op the reference's forward is made of (see _autograd.py)
  ffc::conv_layer      local convs / ConvT + ST conv2 summed per output branch, 1x1 convs, Linear
                       (ffc.py:89-97, ffc_transpose.py:96-106, spectral_transform.py:89,108,
                       fourier_unity.py:45)                        backward: ffc::conv_layer_backward
  ffc::bn_act          BatchNorm2d + activation (ffc_bn_act.py:73-81, spectral_transform.py:89,
                       fourier_unity.py:46-49)                      backward: ffc::bn_act_backward
  ffc::se_scale        SELayer (spectral_transform.py:12-28)        backward: ffc::se_scale_backward
  ffc::pool2, ffc::up2 AvgPool2d(2) / Upsample(x2) (:44-47)         backward: each other
  ffc::rfft2           rfftn(ortho) + Re/Im interleave (fourier_unity.py:38-42)   backward: ffc::irfft2
  ffc::irfft2          de-interleave + irfftn(s=(H, W), ortho) (:51-56) [+ x]     backward: ffc::rfft2
  ffc::noise_inject    NoiseInjection (layers/noise_injection.py:25-32)  backward: ffc::noise_wgrad
  ffc::lfu_split       quadrant stack of the local Fourier unit (spectral_transform.py:96-101, a comment
                       there; run with set_lfu)                     backward: ffc::lfu_split_backward
  ffc::lfu_tile_add    v + its output repeated 2 x 2 (:104-108)     backward: ffc::lfu_tile_backward
  ffc::up2_bilinear, ffc::bn_act_up2b   bilinear x2 upsample [of BatchNorm2d + activation] (GBlock,
                       fgan128_complete.py:148-165)                 backward: ffc::up2_bilinear_adjoint [+ bn_act_backward]
  ffc::pool2_act, ffc::act, ffc::relu_sum_pool   DBlock's pooling + ReLU and the critic's global sum pooling
                       (fgan128_complete.py:249-278, :432-435)      backward: ffc::*_backward

Inference ops (the fused kernels; used under torch.no_grad() / when nothing needs a gradient):
  ffc::ffc_bn_act      one FFC_BN_ACT / FFC / FFCTranspose layer (ffc_bn_act.py:70-83, ffc.py:84-99,
                       ffc_transpose.py:91-110): its local GEMM launch(es), SpectralTransform,
                       BN + activation (+ fgan128's NoiseInjection, + a deferred input transform)
  ffc::spectral_transform   SpectralTransform.forward (spectral_transform.py:77-110)
  ffc::fourier_unit    FourierUnitSN.forward (fourier_unity.py:32-56)
  ffc::linear          nn.Linear (fgan128_complete.py:453-455)
  ffc::quantize_u8     the fgan128 eval-mode uint8 image (fgan128_complete.py:516-521)

A layer op is a function of its arguments: the layer's structure travels as a JSON ``spec``
(constructor arguments and every submodule's mode / BN settings / activation), its parameters and
buffers as tensor lists.  The op runs the spec's *template* -- the same module class built once on
the meta device -- with the argument tensors bound in place of its parameters, so the fused
executor of ffc.py / spectral_transform.py / fourier_unity.py (plan caches, packed weights keyed by
rt.weight_key) serves every module of that structure.
"""
from __future__ import annotations

import contextlib
import functools
import io
import json
import threading
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _autograd as ag
from . import _metrics as mt
from . import _plan
from . import _runtime as rt

# =========================================================================== training ops
# ---------------------------------------------------------------- ffc::conv_layer


@torch.library.custom_op("ffc::conv_layer", mutates_args=())
def conv_layer(xs: List[Tensor], ws: List[Tensor], bs: List[Tensor], spec: str) -> List[Tensor]:
    return ag.conv_layer_impl(xs, ws, bs, spec)


@conv_layer.register_fake
def _(xs, ws, bs, spec):
    outs_s, edges = ag.parse_conv_spec(spec)
    outs, pres = [], []
    for j, (M, act, _) in enumerate(outs_s):
        e = next(e for e in edges if e[0] == j)
        y = xs[e[1]].new_empty(ag.conv_layer_out_shape(e, xs[e[1]], M))
        outs.append(y)
        if act == 5:
            pres.append(xs[e[1]].new_empty(y.shape))
    return outs + pres


@torch.library.custom_op("ffc::conv_layer_backward", mutates_args=())
def conv_layer_backward(xs: List[Tensor], ws: List[Tensor], ts: List[Tensor], gouts: List[Optional[Tensor]],
                        needs: List[bool], spec: str) -> List[Tensor]:
    return ag.conv_layer_backward_impl(xs, ws, ts, gouts, needs, spec)


@conv_layer_backward.register_fake
def _(xs, ws, ts, gouts, needs, spec):
    _, edges = ag.parse_conv_spec(spec)
    nb = sum(1 for e in edges if e[9] >= 0)
    srcs = list(xs) + list(ws)
    res = [t.new_empty(t.shape) if needs[k] else t.new_empty(0) for k, t in enumerate(srcs)]
    bias_ch = {}
    for e in edges:
        if e[9] >= 0:
            bias_ch[e[9]] = ws[edges.index(e)].shape[1 if e[2] == "convT" else 0]
    res += [xs[0].new_empty(bias_ch[b]) if needs[len(srcs) + b] else xs[0].new_empty(0) for b in range(nb)]
    return res


def _conv_layer_setup(ctx, inputs, output):
    xs, ws, bs, spec = inputs
    outs_s, _ = ag.parse_conv_spec(spec)
    no = len(outs_s)
    pres = iter(output[no:])
    ts = [next(pres) if act == 5 else output[j] for j, (_, act, _) in enumerate(outs_s)]
    ctx.spec, ctx.n = spec, (len(xs), len(ws), len(bs))
    ctx.needs = [bool(t.requires_grad) for t in list(xs) + list(ws) + list(bs)]
    ctx.save_for_backward(*xs, *ws, *ts)


def _conv_layer_bwd(ctx, grads):
    n_in, ne, nb = ctx.n
    saved = ctx.saved_tensors
    xs, ws, ts = list(saved[:n_in]), list(saved[n_in:n_in + ne]), list(saved[n_in + ne:])
    gouts = list(grads[:len(ts)])
    res = torch.ops.ffc.conv_layer_backward(xs, ws, ts, gouts, ctx.needs, ctx.spec)
    g = [r if need else None for r, need in zip(res, ctx.needs)]
    return g[:n_in], g[n_in:n_in + ne], g[n_in + ne:], None


conv_layer.register_autograd(_conv_layer_bwd, setup_context=_conv_layer_setup)

# ---------------------------------------------------------------- ffc::bn_act


@torch.library.custom_op("ffc::bn_act", mutates_args=())
def bn_act(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], running_mean: Optional[Tensor],
           running_var: Optional[Tensor], use_batch: bool, eps: float, act: int, act_param: float) -> List[Tensor]:
    """functional (the running statistics are updated by ffc::bn_update_running)"""
    return ag.bn_act_impl(x, weight, bias, running_mean, running_var, use_batch, eps, act, act_param)


def _bn_act_fake(up):
    """the fake of ffc::bn_act and, with ``up``, of ffc::bn_act_up2b (y at twice the height and width)"""
    def fake(x, weight, bias, running_mean, running_var, use_batch, eps, act, act_param):
        C = x.shape[1]
        y = x.new_empty((x.shape[0], C, 2 * x.shape[2], 2 * x.shape[3])) if up else torch.empty_like(x)
        stats = x.new_empty((C, 3), dtype=torch.float64) if use_batch else x.new_empty((2, C))
        return [y, x.new_empty(C), x.new_empty(C), stats]
    return fake


bn_act.register_fake(_bn_act_fake(False))


@torch.library.custom_op("ffc::bn_update_running",
                         mutates_args=("running_mean", "running_var", "num_batches_tracked"))
def bn_update_running(running_mean: Tensor, running_var: Tensor, num_batches_tracked: Optional[Tensor],
                      stats: Tensor, momentum: float, count_mult: float) -> None:
    """nn.BatchNorm2d's running-statistics update from the batch moments ffc::bn_act returned
    (momentum < 0: None, the cumulative average over num_batches_tracked)"""
    ag.bn_update_running_impl(running_mean, running_var, num_batches_tracked, stats, momentum, count_mult)


@bn_update_running.register_fake
def _(running_mean, running_var, num_batches_tracked, stats, momentum, count_mult):
    return None


@torch.library.custom_op("ffc::bn_act_backward", mutates_args=())
def bn_act_backward(x: Tensor, dy: Tensor, scale: Tensor, shift: Tensor, stats: Tensor, weight: Optional[Tensor],
                    use_batch: bool, sync: bool, eps: float, act: int, act_param: float, need_dx: bool,
                    has_weight: bool, has_bias: bool) -> List[Tensor]:
    return ag.bn_act_backward_impl(x, dy, scale, shift, stats, weight, use_batch, sync, eps, act, act_param,
                                   need_dx, has_weight, has_bias)


@bn_act_backward.register_fake
def _(x, dy, scale, shift, stats, weight, use_batch, sync, eps, act, act_param, need_dx, has_weight, has_bias):
    C = x.shape[1]
    return [torch.empty_like(x) if need_dx else x.new_empty(0), x.new_empty(C) if has_weight else x.new_empty(0),
            x.new_empty(C) if has_bias else x.new_empty(0)]


def _bn_act_setup(ctx, inputs, output):
    x, weight, bias, rm, rv, use_batch, eps, act, act_param = inputs
    _, scale, shift, stats = output
    ctx.mark_non_differentiable(scale, shift, stats)
    ctx.use_batch = use_batch
    ctx.sync = ctx.use_batch and rt._sync_group() is not None
    ctx.cfg = (float(eps), int(act), float(act_param))
    ctx.has = (weight is not None, bias is not None)
    ctx.need_dx = bool(x.requires_grad)
    ctx.save_for_backward(x, scale, shift, stats, weight)


def _bn_act_bwd(ctx, grads):
    x, scale, shift, stats, weight = ctx.saved_tensors
    dy = grads[0]
    if dy is None:
        return (None,) * 9
    eps, act, act_param = ctx.cfg
    dx, dw, db = torch.ops.ffc.bn_act_backward(x, dy, scale, shift, stats, weight, ctx.use_batch, ctx.sync, eps, act,
                                               act_param, ctx.need_dx, ctx.has[0], ctx.has[1])
    return (dx if ctx.need_dx else None, dw if ctx.has[0] else None, db if ctx.has[1] else None) + (None,) * 6


bn_act.register_autograd(_bn_act_bwd, setup_context=_bn_act_setup)

# ---------------------------------------------------------------- ffc::se_scale


@torch.library.custom_op("ffc::se_scale", mutates_args=())
def se_scale(x: Tensor, w1: Tensor, w2: Tensor) -> Tensor:
    return ag.se_scale_impl(x, w1, w2)


@se_scale.register_fake
def _(x, w1, w2):
    return torch.empty_like(x)


@torch.library.custom_op("ffc::se_scale_backward", mutates_args=())
def se_scale_backward(x: Tensor, dy: Tensor, w1: Tensor, w2: Tensor) -> List[Tensor]:
    return ag.se_scale_backward_impl(x, dy, w1, w2)


@se_scale_backward.register_fake
def _(x, dy, w1, w2):
    return [torch.empty_like(x), torch.empty_like(w1), torch.empty_like(w2)]


def _se_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _se_bwd(ctx, dy):
    x, w1, w2 = ctx.saved_tensors
    return tuple(torch.ops.ffc.se_scale_backward(x, dy, w1, w2))


se_scale.register_autograd(_se_bwd, setup_context=_se_setup)

# ---------------------------------------------------------------- ffc::pool2 / ffc::up2 (adjoints of each other)


@torch.library.custom_op("ffc::pool2", mutates_args=())
def pool2(x: Tensor, scale: float) -> Tensor:
    return ag.pool2_impl(x, scale)


@pool2.register_fake
def _(x, scale):
    return x.new_empty((x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2))


@torch.library.custom_op("ffc::up2", mutates_args=())
def up2(x: Tensor, scale: float) -> Tensor:
    return ag.up2_impl(x, scale)


@up2.register_fake
def _(x, scale):
    return x.new_empty((x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3]))


def _scale_setup(ctx, inputs, output):
    ctx.scale = inputs[1]


pool2.register_autograd(lambda ctx, dy: (torch.ops.ffc.up2(dy, ctx.scale), None), setup_context=_scale_setup)
up2.register_autograd(lambda ctx, dy: (torch.ops.ffc.pool2(dy, ctx.scale), None), setup_context=_scale_setup)

# ---------------------------------------------------------------- ffc::up2_bilinear (+ adjoint), ffc::bn_act_up2b
# F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) of GBlock (fgan128_complete.py:148-156)


@torch.library.custom_op("ffc::up2_bilinear", mutates_args=())
def up2_bilinear(x: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], act: int, act_param: float) -> Tensor:
    """up2(act(scale * x + shift)); scale / shift (C,), (B, C) or None.  Differentiable in its plain form (no
    affine, Identity); the BatchNorm form with a backward is ffc::bn_act_up2b"""
    return ag.up2_bilinear_impl(x, scale, shift, act, act_param)


@up2_bilinear.register_fake
def _(x, scale, shift, act, act_param):
    return x.new_empty((x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3]))


@torch.library.custom_op("ffc::up2_bilinear_adjoint", mutates_args=())
def up2_bilinear_adjoint(dy: Tensor) -> Tensor:
    return ag.up2_bilinear_adjoint_impl(dy)


@up2_bilinear_adjoint.register_fake
def _(dy):
    return dy.new_empty((dy.shape[0], dy.shape[1], dy.shape[2] // 2, dy.shape[3] // 2))


def _up2b_setup(ctx, inputs, output):
    _, scale, _, act, _ = inputs
    ctx.plain = scale is None and act == 0


def _up2b_bwd(ctx, dy):
    if not ctx.plain:
        raise NotImplementedError("ffc::up2_bilinear has a backward in its plain form only (ffc::bn_act_up2b "
                                  "differentiates the BatchNorm + activation form)")
    return torch.ops.ffc.up2_bilinear_adjoint(dy), None, None, None, None


up2_bilinear.register_autograd(_up2b_bwd, setup_context=_up2b_setup)
up2_bilinear_adjoint.register_autograd(lambda ctx, g: torch.ops.ffc.up2_bilinear(g, None, None, 0, 0.0),
                                       setup_context=lambda ctx, inputs, output: None)


@torch.library.custom_op("ffc::bn_act_up2b", mutates_args=())
def bn_act_up2b(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], running_mean: Optional[Tensor],
                running_var: Optional[Tensor], use_batch: bool, eps: float, act: int, act_param: float) -> List[Tensor]:
    """ffc::bn_act with the bilinear x2 upsample applied to its output: [y (B, C, 2h, 2w), scale, shift, stats]"""
    return ag.bn_act_impl(x, weight, bias, running_mean, running_var, use_batch, eps, act, act_param, up=True)


bn_act_up2b.register_fake(_bn_act_fake(True))


def _bn_act_up2b_bwd(ctx, grads):
    """the adjoint upsample brings dy to the low resolution, where it is ffc::bn_act's backward (x, scale and shift
    are what that needs)"""
    if grads[0] is None:
        return (None,) * 9
    return _bn_act_bwd(ctx, [torch.ops.ffc.up2_bilinear_adjoint(grads[0])])


bn_act_up2b.register_autograd(_bn_act_up2b_bwd, setup_context=_bn_act_setup)

# ---------------------------------------------------------------- ffc::pool2_act, ffc::relu_sum_pool (DBlock, critic)


@torch.library.custom_op("ffc::pool2_act", mutates_args=())
def pool2_act(x: Tensor, act: int, act_param: float) -> Tensor:
    """act(AvgPool2d(2)(x)) (act: Identity, ReLU, LeakyReLU, Tanh, Sigmoid)"""
    return ag.pool2_act_impl(x, act, act_param)


@pool2_act.register_fake
def _(x, act, act_param):
    return x.new_empty((x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2))


@torch.library.custom_op("ffc::pool2_act_backward", mutates_args=())
def pool2_act_backward(y: Tensor, dy: Tensor, act: int, act_param: float) -> Tensor:
    return ag.pool2_act_backward_impl(y, dy, act, act_param)


@pool2_act_backward.register_fake
def _(y, dy, act, act_param):
    return y.new_empty((y.shape[0], y.shape[1], 2 * y.shape[2], 2 * y.shape[3]))


def _pool2_act_setup(ctx, inputs, output):
    ctx.cfg = (int(inputs[1]), float(inputs[2]))
    ctx.save_for_backward(output)


def _pool2_act_bwd(ctx, dy):
    (y,) = ctx.saved_tensors
    return torch.ops.ffc.pool2_act_backward(y, dy, *ctx.cfg), None, None


pool2_act.register_autograd(_pool2_act_bwd, setup_context=_pool2_act_setup)


@torch.library.custom_op("ffc::act", mutates_args=())
def act(x: Tensor, act: int, act_param: float) -> Tensor:
    """act(x) out of place (ReLU, LeakyReLU, Tanh, Sigmoid); backward: ffc_act_bwd through the output"""
    return ag.act_impl(x, act, act_param)


@act.register_fake
def _(x, act, act_param):
    return torch.empty_like(x)


@torch.library.custom_op("ffc::act_backward", mutates_args=())
def act_backward(y: Tensor, dy: Tensor, act: int, act_param: float) -> Tensor:
    return ag.act_backward(y.contiguous(), dy, act, act_param)


@act_backward.register_fake
def _(y, dy, act, act_param):
    return torch.empty_like(y)


def _act_setup(ctx, inputs, output):
    ctx.cfg = (int(inputs[1]), float(inputs[2]))
    ctx.save_for_backward(output)


def _act_bwd(ctx, dy):
    (y,) = ctx.saved_tensors
    return torch.ops.ffc.act_backward(y, dy, *ctx.cfg), None, None


act.register_autograd(_act_bwd, setup_context=_act_setup)


@torch.library.custom_op("ffc::relu_sum_pool", mutates_args=())
def relu_sum_pool(x: Tensor) -> Tensor:
    """torch.sum(relu(x), (2, 3)) -> (B, C)"""
    return ag.relu_sum_pool_impl(x)


@relu_sum_pool.register_fake
def _(x):
    return x.new_empty((x.shape[0], x.shape[1]))


@torch.library.custom_op("ffc::relu_sum_pool_backward", mutates_args=())
def relu_sum_pool_backward(x: Tensor, dout: Tensor) -> Tensor:
    return ag.relu_sum_pool_backward_impl(x, dout)


@relu_sum_pool_backward.register_fake
def _(x, dout):
    return torch.empty_like(x)


def _rsp_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _rsp_bwd(ctx, dout):
    (x,) = ctx.saved_tensors
    return torch.ops.ffc.relu_sum_pool_backward(x, dout)


relu_sum_pool.register_autograd(_rsp_bwd, setup_context=_rsp_setup)

# ---------------------------------------------------------------- ffc::rfft2 / ffc::irfft2


@torch.library.custom_op("ffc::rfft2", mutates_args=())
def rfft2(x: Tensor, mirror_scale: float) -> Tensor:
    return ag.rfft2_impl(x, mirror_scale)


@rfft2.register_fake
def _(x, mirror_scale):
    return x.new_empty((x.shape[0], 2 * x.shape[1], x.shape[2], x.shape[3] // 2 + 1))


@torch.library.custom_op("ffc::irfft2", mutates_args=())
def irfft2(Z: Tensor, H: int, W: int, mirror_scale: float, r: Optional[Tensor]) -> Tensor:
    return ag.irfft2_impl(Z, H, W, mirror_scale, r)


@irfft2.register_fake
def _(Z, H, W, mirror_scale, r):
    return Z.new_empty((Z.shape[0], Z.shape[1] // 2, H, W))


def _rfft2_setup(ctx, inputs, output):
    x, ms = inputs
    ctx.hw, ctx.ms = (x.shape[2], x.shape[3]), ms


def _rfft2_bwd(ctx, dZ):
    if ctx.ms != 1.0:
        raise NotImplementedError("ffc::rfft2 backward: mirror_scale 1 only")
    # d/dx of rfftn(ortho): irfftn(ortho) with the mirrored bins halved
    return torch.ops.ffc.irfft2(dZ, ctx.hw[0], ctx.hw[1], 0.5, None), None


def _irfft2_setup(ctx, inputs, output):
    ctx.ms, ctx.has_r = inputs[3], inputs[4] is not None


def _irfft2_bwd(ctx, dy):
    if ctx.ms != 1.0:
        raise NotImplementedError("ffc::irfft2 backward: mirror_scale 1 only")
    # d/dZ of irfftn(ortho): rfftn(ortho) with the mirrored bins doubled
    return torch.ops.ffc.rfft2(dy, 2.0), None, None, None, (dy if ctx.has_r else None)


rfft2.register_autograd(_rfft2_bwd, setup_context=_rfft2_setup)
irfft2.register_autograd(_irfft2_bwd, setup_context=_irfft2_setup)

# ---------------------------------------------------------------- ffc::lfu_split / ffc::lfu_tile_add
# the data movement of SpectralTransform's local Fourier unit (csrc/lfu_kernels.hip)


@torch.library.custom_op("ffc::lfu_split", mutates_args=())
def lfu_split(s: Tensor) -> Tensor:
    """(B, c, H, W) -> the quadrants of the first c/4 channels stacked on the channel axis (B, c, H/2, W/2)"""
    return ag.lfu_split_impl(s)


@lfu_split.register_fake
def _(s):
    return s.new_empty((s.shape[0], s.shape[1], s.shape[2] // 2, s.shape[3] // 2))


@torch.library.custom_op("ffc::lfu_split_backward", mutates_args=())
def lfu_split_backward(dxs: Tensor) -> Tensor:
    return ag.lfu_split_backward_impl(dxs)


@lfu_split_backward.register_fake
def _(dxs):
    return dxs.new_empty((dxs.shape[0], dxs.shape[1], 2 * dxs.shape[2], 2 * dxs.shape[3]))


@torch.library.custom_op("ffc::lfu_tile_add", mutates_args=())
def lfu_tile_add(v: Tensor, ys: Tensor) -> Tensor:
    """v (B, c, H, W) + ys (B, c, H/2, W/2) repeated 2 x 2 over the plane"""
    return ag.lfu_tile_add_impl(v, ys)


@lfu_tile_add.register_fake
def _(v, ys):
    return torch.empty_like(v)


@torch.library.custom_op("ffc::lfu_tile_backward", mutates_args=())
def lfu_tile_backward(dv: Tensor) -> Tensor:
    return ag.lfu_tile_backward_impl(dv)


@lfu_tile_backward.register_fake
def _(dv):
    return dv.new_empty((dv.shape[0], dv.shape[1], dv.shape[2] // 2, dv.shape[3] // 2))


# split <-> split_backward are each other's adjoints (a permutation and its zero-filled inverse);
# tile_add passes the gradient through to v and sums its four quadrants for ys
lfu_split.register_autograd(lambda ctx, dxs: torch.ops.ffc.lfu_split_backward(dxs))
lfu_split_backward.register_autograd(lambda ctx, ds: torch.ops.ffc.lfu_split(ds))
lfu_tile_add.register_autograd(lambda ctx, dv: (dv, torch.ops.ffc.lfu_tile_backward(dv)))

# ---------------------------------------------------------------- ffc::noise_inject


@torch.library.custom_op("ffc::noise_inject", mutates_args=())
def noise_inject(x: Tensor, weight: Tensor, noise: Tensor) -> Tensor:
    return ag.noise_inject_impl(x, weight, noise)


@noise_inject.register_fake
def _(x, weight, noise):
    return torch.empty_like(x)


@torch.library.custom_op("ffc::noise_wgrad", mutates_args=())
def noise_wgrad(g: Tensor, noise: Tensor) -> Tensor:
    return ag.noise_wgrad_impl(g, noise)


@noise_wgrad.register_fake
def _(g, noise):
    return g.new_empty((1, g.shape[1], 1, 1))


def _noise_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[2])
    ctx.need_w = bool(inputs[1].requires_grad)


def _noise_bwd(ctx, g):
    (noise,) = ctx.saved_tensors
    dw = torch.ops.ffc.noise_wgrad(g, noise).view(ctx.wshape) if ctx.need_w else None
    return g, dw, None


def _noise_setup_shape(ctx, inputs, output):
    _noise_setup(ctx, inputs, output)
    ctx.wshape = tuple(inputs[1].shape)


noise_inject.register_autograd(_noise_bwd, setup_context=_noise_setup_shape)

# ---------------------------------------------------------------- ffc::cond_stem / ffc::embed_rows
# class-conditional fgan128 (fgan128_cond_complete.py:33-180); labels: an int64 device tensor the
# kernels read (no host read: a captured step replays with new labels in the same buffer)


@torch.library.custom_op("ffc::cond_stem", mutates_args=())
def cond_stem(z: Tensor, labels: Tensor, label_embed: Tensor, w_in: Tensor, b_in: Tensor, w_label: Tensor,
              b_label: Tensor, gamma_in: Tensor, beta_in: Tensor, gamma_label: Tensor, beta_label: Tensor,
              rmean_in: Tensor, rvar_in: Tensor, rmean_label: Tensor, rvar_label: Tensor, use_batch: bool,
              eps: float) -> List[Tensor]:
    """FCondGenerator's stem (:91-101) -> [y (B, 512, 4, 4), pre, scale, shift, stats]; functional (the
    running statistics are updated by ffc::bn_update_running from stats)"""
    return ag.cond_stem_impl(z, labels, label_embed, w_in, b_in, w_label, b_label, gamma_in, beta_in, gamma_label,
                             beta_label, rmean_in, rvar_in, rmean_label, rvar_label, use_batch, eps)


@cond_stem.register_fake
def _(z, labels, label_embed, w_in, b_in, w_label, b_label, gamma_in, beta_in, gamma_label, beta_label, rmean_in,
      rvar_in, rmean_label, rvar_label, use_batch, eps):
    C = 2 * ag.STEM_CH
    y = z.new_empty((z.shape[0], C, 4, 4))
    stats = z.new_empty((C, 3), dtype=torch.float64) if use_batch else z.new_empty((2, C))
    return [y, torch.empty_like(y), z.new_empty(C), z.new_empty(C), stats]


@torch.library.custom_op("ffc::cond_stem_backward", mutates_args=())
def cond_stem_backward(dpre: Tensor, z: Tensor, labels: Tensor, label_embed: Tensor, w_in: Tensor, w_label: Tensor,
                       needs: List[bool]) -> List[Tensor]:
    """-> [dz, d label_embed, dw_in, db_in, dw_label, db_label] (empty tensors where not needed)"""
    return ag.cond_stem_backward_impl(dpre, z, labels, label_embed, w_in, w_label, needs)


@cond_stem_backward.register_fake
def _(dpre, z, labels, label_embed, w_in, w_label, needs):
    shapes = [z.shape, label_embed.shape, w_in.shape, (ag.STEM_CH,), w_label.shape, (ag.STEM_CH,)]
    return [z.new_empty(s if n else (0,)) for s, n in zip(shapes, needs)]


def _cond_stem_setup(ctx, inputs, output):
    z, labels, embed, w_in, b_in, w_label, b_label, gamma_in, beta_in, gamma_label, beta_label = inputs[:11]
    _, pre, scale, shift, stats = output
    ctx.mark_non_differentiable(pre, scale, shift, stats)
    ctx.use_batch, ctx.eps = inputs[15], float(inputs[16])
    ctx.needs = [bool(t.requires_grad) for t in (z, embed, w_in, b_in, w_label, b_label)]
    ctx.needs_bn = [bool(t.requires_grad) for t in (gamma_in, beta_in, gamma_label, beta_label)]
    ctx.save_for_backward(z, labels, embed, w_in, w_label, pre, scale, shift, stats,
                          torch.cat((gamma_in.detach(), gamma_label.detach())))


def _cond_stem_bwd(ctx, grads):
    dy = grads[0]
    if dy is None:
        return (None,) * 17
    z, labels, embed, w_in, w_label, pre, scale, shift, stats, gamma = ctx.saved_tensors
    dpre, dgamma, dbeta = torch.ops.ffc.bn_act_backward(pre, dy, scale, shift, stats, gamma, ctx.use_batch, False,
                                                        ctx.eps, 5, 0.0, True, True, True)
    dz, dembed, dw_in, db_in, dw_label, db_label = torch.ops.ffc.cond_stem_backward(dpre, z, labels, embed, w_in,
                                                                                    w_label, ctx.needs)
    C = ag.STEM_CH
    bn = (dgamma[:C], dbeta[:C], dgamma[C:], dbeta[C:])
    n = ctx.needs
    return (dz if n[0] else None, None, dembed if n[1] else None, dw_in if n[2] else None, db_in if n[3] else None,
            dw_label if n[4] else None, db_label if n[5] else None) + \
        tuple(g if need else None for g, need in zip(bn, ctx.needs_bn)) + (None,) * 6


cond_stem.register_autograd(_cond_stem_bwd, setup_context=_cond_stem_setup)


@torch.library.custom_op("ffc::embed_rows", mutates_args=())
def embed_rows(weight: Tensor, labels: Tensor) -> Tensor:
    """nn.Embedding lookup weight[labels] -> (B, D) (the critic's label plane, :159-163)"""
    return ag.embed_rows_impl(weight, labels)


@embed_rows.register_fake
def _(weight, labels):
    return weight.new_empty((labels.shape[0], weight.shape[1]))


@torch.library.custom_op("ffc::embed_rows_backward", mutates_args=())
def embed_rows_backward(grad: Tensor, labels: Tensor, num_classes: int) -> Tensor:
    return ag.embed_rows_backward_impl(grad, labels, num_classes)


@embed_rows_backward.register_fake
def _(grad, labels, num_classes):
    return grad.new_empty((num_classes, grad.shape[1]))


def _embed_rows_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])
    ctx.num_classes = inputs[0].shape[0]


def _embed_rows_bwd(ctx, g):
    (labels,) = ctx.saved_tensors
    return torch.ops.ffc.embed_rows_backward(g, labels, ctx.num_classes), None


embed_rows.register_autograd(_embed_rows_bwd, setup_context=_embed_rows_setup)

# ---------------------------------------------------------------- ffc::cbn_act
# ConditionalBatchNorm2d + activation (+ NoiseInjection) (layers/cond/cond_bn.py:16-24 inside
# ffc_bn_act.py:70-83); labels as above: an int64 device tensor the kernels read


@torch.library.custom_op("ffc::cbn_act", mutates_args=())
def cbn_act(x: Tensor, labels: Tensor, embed: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
            use_batch: bool, eps: float, act: int, act_param: float, noise_w: Optional[Tensor],
            noise: Optional[Tensor]) -> List[Tensor]:
    """-> [y, scale0, shift0, stats]; functional (the running statistics are updated by
    ffc::bn_update_running from stats).  noise_w / noise: the NoiseInjection that follows, or None (no
    defaults in the schema: the dispatcher drops arguments equal to their default, and the backward
    returns one gradient per argument)"""
    return ag.cbn_act_impl(x, labels, embed, running_mean, running_var, use_batch, eps, act, act_param, noise_w,
                           noise)


@cbn_act.register_fake
def _(x, labels, embed, running_mean, running_var, use_batch, eps, act, act_param, noise_w, noise):
    C = x.shape[1]
    stats = x.new_empty((C, 3), dtype=torch.float64) if use_batch else x.new_empty((2, C))
    return [x.new_empty(x.shape), x.new_empty(C), x.new_empty(C), stats]


@torch.library.custom_op("ffc::cbn_act_backward", mutates_args=())
def cbn_act_backward(x: Tensor, dy: Tensor, labels: Tensor, embed: Tensor, scale: Tensor, shift: Tensor,
                     use_batch: bool, act: int, act_param: float, need_dx: bool, need_embed: bool) -> List[Tensor]:
    """-> [dx, d embed] (empty tensors where not needed)"""
    return ag.cbn_act_backward_impl(x, dy, labels, embed, scale, shift, use_batch, act, act_param, need_dx,
                                    need_embed)


@cbn_act_backward.register_fake
def _(x, dy, labels, embed, scale, shift, use_batch, act, act_param, need_dx, need_embed):
    return [x.new_empty(x.shape) if need_dx else x.new_empty(0),
            embed.new_empty(embed.shape) if need_embed else x.new_empty(0)]


def _cbn_act_setup(ctx, inputs, output):
    x, labels, embed, _, _, use_batch, _, act, act_param, noise_w, noise = inputs
    _, scale, shift, stats = output
    ctx.mark_non_differentiable(scale, shift, stats)
    ctx.cfg = (bool(use_batch), int(act), float(act_param))
    ctx.needs = (bool(x.requires_grad), bool(embed.requires_grad),
                 noise_w is not None and bool(noise_w.requires_grad))
    ctx.wshape = tuple(noise_w.shape) if noise_w is not None else None
    ctx.has_noise = noise is not None
    ctx.save_for_backward(x, labels, embed, scale, shift, *((noise,) if noise is not None else ()))


def _cbn_act_bwd(ctx, grads):
    dy = grads[0]
    if dy is None:
        return (None,) * 11
    x, labels, embed, scale, shift = ctx.saved_tensors[:5]
    use_batch, act, act_param = ctx.cfg
    need_dx, need_embed, need_nw = ctx.needs
    dx = dembed = dnw = None
    if need_dx or need_embed:
        dx, dembed = torch.ops.ffc.cbn_act_backward(x, dy, labels, embed, scale, shift, use_batch, act, act_param,
                                                    need_dx, need_embed)
    if need_nw:
        dnw = torch.ops.ffc.noise_wgrad(dy, ctx.saved_tensors[5]).view(ctx.wshape)
    return (dx if need_dx else None, None, dembed if need_embed else None) + (None,) * 6 + (dnw, None)


cbn_act.register_autograd(_cbn_act_bwd, setup_context=_cbn_act_setup)

# ---------------------------------------------------------------- ffc::sn_weight
# torch.nn.utils.spectral_norm's pre-hook (one power iteration, sigma, W = W_orig / sigma) for a list
# of layers on csrc/sn_kernels.hip; the autograd wrapper is _autograd.SpectralNormWeight


@torch.library.custom_op("ffc::sn_weight", mutates_args=("u", "v", "w", "sigma", "saved"))
def sn_weight(w_orig: List[Tensor], u: List[Tensor], v: List[Tensor], w: List[Tensor], sigma: Tensor, saved: Tensor,
              dims: List[int], training: bool, flags: Optional[List[int]] = None) -> None:
    """w[i] <- w_orig[i] / sigma[i]; training: u[i], v[i] advanced in place by one power iteration;
    saved: a flat copy of this call's (u, v) per layer, or an empty tensor; flags: ffc_sn_job.flags per
    layer (None: 0, the hook's normalize)"""
    ag.sn_weight_impl(w_orig, u, v, w, sigma, saved, dims, training, flags)


@sn_weight.register_fake
def _(w_orig, u, v, w, sigma, saved, dims, training, flags=None):
    return None


@torch.library.custom_op("ffc::sn_weight_bwd", mutates_args=())
def sn_weight_bwd(dw: List[Tensor], w_orig: List[Tensor], saved: Tensor, sigma: Tensor,
                  dims: List[int]) -> List[Tensor]:
    """-> [dw_orig]: dw / sigma - (<dw, w_orig> / sigma^2) u v^T per layer"""
    return ag.sn_weight_bwd_impl(dw, w_orig, saved, sigma, dims)


@sn_weight_bwd.register_fake
def _(dw, w_orig, saved, sigma, dims):
    return [t.new_empty(t.shape) for t in w_orig]


# ---------------------------------------------------------------- ffc::aw_weights / ffc::aw_combine
# aw_method.aw_loss (layers/aw_loss.py:13-107) after its two gradient passes, on csrc/aw_kernels.hip; the
# module is aw_loss.aw_method


@torch.library.custom_op("ffc::aw_weights", mutates_args=())
def aw_weights(g_real: List[Tensor], g_fake: List[Tensor], real_validity: Tensor, fake_validity: Tensor,
               alpha1: float, alpha2: float, delta: float, epsilon: float, normalized: bool) -> Tensor:
    """-> stats (8,) fp64 on the device: [rr, ff, rf, rs, fs, w_r, w_f, case]"""
    return ag.aw_weights_impl(g_real, g_fake, real_validity, fake_validity, alpha1, alpha2, delta, epsilon,
                              normalized)


@aw_weights.register_fake
def _(g_real, g_fake, real_validity, fake_validity, alpha1, alpha2, delta, epsilon, normalized):
    return real_validity.new_empty((ag.AW_STATS,), dtype=torch.float64)


@torch.library.custom_op("ffc::aw_combine", mutates_args=("out",))
def aw_combine(g_real: List[Tensor], g_fake: List[Tensor], stats: Tensor, out: List[Tensor]) -> None:
    """out[i] <- w_r * g_real[i] + w_f * g_fake[i], the weights read from ``stats`` on the device"""
    ag.aw_combine_impl(g_real, g_fake, stats, out)


@aw_combine.register_fake
def _(g_real, g_fake, stats, out):
    return None


# ---------------------------------------------------------------- ffc::feat_moments_update / kid_sums / isc_sums
# torch_fidelity's FID / KID / Inception-score arithmetic from feature batches on csrc/metric_kernels.hip; the
# callers are fidelity.FeatureStats, kid_features_to_metric and isc_features_to_metric.  Metrics carry no gradient.


@torch.library.custom_op("ffc::feat_moments_update", mutates_args=("state",))
def feat_moments_update(state: Tensor, features: Tensor) -> None:
    """state [n, pivot[D], s1[D], S2[D][D]] (fp64) <- state + the batch ``features`` (B, D)"""
    mt.feat_moments_update_impl(state, features)


@feat_moments_update.register_fake
def _(state, features):
    return None


@torch.library.custom_op("ffc::kid_sums", mutates_args=())
def kid_sums(features_1: Tensor, features_2: Tensor, idx1: Tensor, idx2: Tensor, degree: int, gamma: float,
             coef0: float) -> Tensor:
    """-> (subsets, 6) fp64: [sum K_XX, sum diag K_XX, sum K_YY, sum diag K_YY, sum K_XY, trace K_XY]"""
    return mt.kid_sums_impl(features_1, features_2, idx1, idx2, degree, gamma, coef0)


@kid_sums.register_fake
def _(features_1, features_2, idx1, idx2, degree, gamma, coef0):
    return features_1.new_empty((idx1.shape[0], mt.KID_SUMS), dtype=torch.float64)


@torch.library.custom_op("ffc::isc_sums", mutates_args=())
def isc_sums(logits: Tensor, perm: Tensor, splits: int) -> Tensor:
    """-> (splits, 4 + C) fp64 per chunk: [n_i, sum p log p, exponent, score, column sums of p]"""
    return mt.isc_sums_impl(logits, perm, splits)


@isc_sums.register_fake
def _(logits, perm, splits):
    return logits.new_empty((splits, mt.ISC_HEAD + logits.shape[1]), dtype=torch.float64)


# ---------------------------------------------------------------- ffc::prc
# torch_fidelity's improved precision and recall (metric_prc.py) from two feature matrices on csrc/prc_kernels.hip;
# the caller is fidelity.prc_features_to_metric.  No gradient.


@torch.library.custom_op("ffc::prc", mutates_args=())
def prc(features_1: Tensor, features_2: Tensor, neighborhood: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (radii2_1 (N1,) fp64, radii2_2 (N2,) fp64, hit_2 (N2,) int32, hit_1 (N1,) int32, counts (2,) fp64 =
    [sum hit_2, sum hit_1]); features_1 is the real set"""
    return mt.prc_impl(features_1, features_2, neighborhood)


@prc.register_fake
def _(features_1, features_2, neighborhood):
    n1, n2 = features_1.shape[0], features_2.shape[0]
    return (features_1.new_empty((n1,), dtype=torch.float64), features_1.new_empty((n2,), dtype=torch.float64),
            features_1.new_empty((n2,), dtype=torch.int32), features_1.new_empty((n1,), dtype=torch.int32),
            features_1.new_empty((2,), dtype=torch.float64))


# ---------------------------------------------------------------- ffc::optim_step / ffc::optim_tick
# torch.optim's single-tensor Adam / AdamW and LambdaLR(lambda s: 1 - s / T).step() on csrc/optim_kernels.hip, the
# step and schedule counts in ``state`` on the device; the optimizers are optim.FusedAdamW / FusedAdam


@torch.library.custom_op("ffc::optim_step", mutates_args=("params", "exp_avgs", "exp_avg_sqs", "state"))
def optim_step(params: List[Tensor], grads: List[Tensor], exp_avgs: List[Tensor], exp_avg_sqs: List[Tensor],
               state: Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
               decay_steps: int, adam_mode: int) -> None:
    """state[0] (t) += 1, then the Adam (adam_mode 1) / AdamW (0) update of every entry in place.  (An argument
    called ``mode`` would collide with a keyword of torch's functionalization of mutating ops.)"""
    ag.optim_step_impl(params, grads, exp_avgs, exp_avg_sqs, state, lr, beta1, beta2, eps, weight_decay, decay_steps,
                       adam_mode)


@optim_step.register_fake
def _(params, grads, exp_avgs, exp_avg_sqs, state, lr, beta1, beta2, eps, weight_decay, decay_steps, adam_mode):
    return None


@torch.library.custom_op("ffc::optim_tick", mutates_args=("state",))
def optim_tick(state: Tensor) -> None:
    """s += 1 in every 4-word block of ``state``"""
    ag.optim_tick_impl(state)


@optim_tick.register_fake
def _(state):
    return None


# ---------------------------------------------------------------- ffc::self_attn
# Self_Attn (layers/attention_layer.py:30-39) after its stacked q / k / v projection, on csrc/attn_kernels.hip


@torch.library.custom_op("ffc::self_attn", mutates_args=())
def self_attn(x: Tensor, qkv: Tensor, gamma: Tensor, save: bool) -> List[Tensor]:
    """-> [y = gamma * attention(qkv) + x, L (B, N), o (B, C, N) for the backward when ``save`` else empty]"""
    return ag.self_attn_impl(x, qkv, gamma, save)


@self_attn.register_fake
def _(x, qkv, gamma, save):
    B, C, H, W = x.shape
    return [torch.empty_like(x), x.new_empty((B, H * W)), x.new_empty((B, C, H * W) if save else (0,))]


@torch.library.custom_op("ffc::self_attn_matrix", mutates_args=())
def self_attn_matrix(qkv: Tensor, L: Tensor, C: int) -> Tensor:
    """the attention matrix (B, N, N), written only when asked for; carries no gradient"""
    return ag.self_attn_matrix_impl(qkv, L, C)


@self_attn_matrix.register_fake
def _(qkv, L, C):
    return qkv.new_empty((L.shape[0], L.shape[1], L.shape[1]))


@torch.library.custom_op("ffc::self_attn_bwd", mutates_args=())
def self_attn_bwd(dy: Tensor, qkv: Tensor, o: Tensor, L: Tensor, gamma: Tensor) -> List[Tensor]:
    """-> [dqkv, dgamma]; deterministic (no atomics)"""
    return ag.self_attn_bwd_impl(dy, qkv, o, L, gamma)


@self_attn_bwd.register_fake
def _(dy, qkv, o, L, gamma):
    return [torch.empty_like(qkv), gamma.new_empty((1,))]


def _self_attn_setup(ctx, inputs, output):
    x, qkv, gamma, save = inputs
    ctx.saved = bool(save)
    ctx.gshape = tuple(gamma.shape)
    if save:
        ctx.save_for_backward(qkv, output[2], output[1], gamma)


def _self_attn_bwd(ctx, grads):
    dy = grads[0]
    if dy is None:
        return None, None, None, None
    if not ctx.saved:
        raise RuntimeError("ffc::self_attn ran with save=False; it has no backward")
    qkv, o, L, gamma = ctx.saved_tensors
    dqkv, dgamma = torch.ops.ffc.self_attn_bwd(dy, qkv, o, L, gamma)
    return dy, dqkv, dgamma.view(ctx.gshape), None


self_attn.register_autograd(_self_attn_bwd, setup_context=_self_attn_setup)

# =========================================================================== inference ops


@torch.library.custom_op("ffc::linear", mutates_args=())
def linear(z: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """nn.Linear on the dense HIP GEMM: z (B, K) . weight^T (K, N) + bias"""
    z = rt.require(z, "z")
    N, K = weight.shape
    if z.dim() != 2 or z.shape[1] != K:
        raise RuntimeError(f"linear: z must be (B, {K}), got {tuple(z.shape)}")
    rt.note_tensors([weight, bias])
    w = rt.require(weight.detach(), "weight")
    b = rt.require(bias.detach(), "bias") if bias is not None else None
    with _PACKS.hold() as packs:
        Wt = packs.get("linearT", [w], lambda: w.t().contiguous())
        B = z.shape[0]
        out = torch.empty((B, N), device=z.device, dtype=torch.float32)
        with rt.observe("dense", flops=2.0 * B * K * N):
            rt.check(rt.lib().ffc_dense_forward(rt.ptr(z), rt.ptr(Wt), rt.ptr(b), B, K, N, N, rt.ptr(out), None, 0,
                                                0.0, rt.stream_of(z)), "ffc_dense_forward")
    return out


@linear.register_fake
def _(z, weight, bias):
    return z.new_empty((z.shape[0], weight.shape[0]))


_PACKS = rt.StreamPool(lambda: rt.PackCache(64))   # transposed Linear weights


@torch.library.custom_op("ffc::quantize_u8", mutates_args=())
def quantize_u8(x: Tensor) -> Tensor:
    """fgan128_complete.py:516-521: the float image -> uint8 over its own global min / max"""
    x = rt.require(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    rt.check(rt.lib().ffc_quantize_u8(rt.ptr(x), rt.ptr(out), x.numel(), rt.stream_of(x)), "ffc_quantize_u8")
    return out


@quantize_u8.register_fake
def _(x):
    return torch.empty_like(x, dtype=torch.uint8)


# ---------------------------------------------------------------- layer templates
_ACTS = {"Identity": nn.Identity, "ReLU": nn.ReLU, "LeakyReLU": nn.LeakyReLU, "Tanh": nn.Tanh,
         "Sigmoid": nn.Sigmoid, "GELU": nn.GELU, "BatchNorm2d": nn.BatchNorm2d}
_ACT_MODS = (nn.Identity, nn.ReLU, nn.LeakyReLU, nn.Tanh, nn.Sigmoid, nn.GELU)


def _module_state(m: nn.Module):
    """the per-submodule settings a layer op depends on besides its tensors"""
    out = []
    for name, sub in m.named_modules():
        e = [name, bool(sub.training)]
        if isinstance(sub, nn.BatchNorm2d):
            e += [sub.momentum, float(sub.eps), bool(sub.affine), bool(sub.track_running_stats), sub.num_features]
        elif isinstance(sub, nn.LeakyReLU):
            e += [float(sub.negative_slope)]
        elif isinstance(sub, nn.GELU):
            e += [sub.approximate]
        elif hasattr(sub, "mix_precision"):
            e += [sub.mix_precision]
        elif getattr(sub, "run_lfu", False):   # a SpectralTransform running its local Fourier unit: another
            e += ["run_lfu"]                   # spec, so another template and plan (off: the spec is unchanged)
        out.append(e)
    return out


def layer_spec(m: nn.Module) -> str:
    """JSON spec of a FFC_BN_ACT / FFC / FFCTranspose / SpectralTransform / FourierUnitSN module"""
    ctor = getattr(m, "_ffc_ctor", None)
    if ctor is None:
        raise NotImplementedError(f"{type(m).__name__} has no layer op")
    return json.dumps({"ctor": ctor, "state": _module_state(m)}, separators=(",", ":"))


class _Template:
    """a layer module of the spec's structure on the meta device, plus its tensor slots"""

    def __init__(self, spec: str):
        from .ffc import FFC, FFC_BN_ACT, FFCTranspose, FourierUnitSN, SpectralTransform
        d = json.loads(spec)
        kind, args = d["ctor"][0], dict(d["ctor"][1])
        cls = {"FFC_BN_ACT": FFC_BN_ACT, "FFC": FFC, "FFCTranspose": FFCTranspose,
               "SpectralTransform": SpectralTransform, "FourierUnitSN": FourierUnitSN}[kind]
        for k in ("norm_layer", "activation_layer"):
            if k in args:
                if args[k] not in _ACTS:
                    raise NotImplementedError(f"{k} {args[k]} has no HIP path")
                args[k] = _ACTS[args[k]]
        # built outside any active tracing / fake mode (a template is a cached object, not graph content)
        from torch.utils._python_dispatch import _disable_current_modes
        with _disable_current_modes(), torch.device("meta"), contextlib.redirect_stdout(io.StringIO()):
            mod = cls(**args)
        subs = dict(mod.named_modules())
        for e in d["state"]:
            name, training = e[0], e[1]
            sub = subs.get(name)
            if sub is None:
                raise NotImplementedError(f"layer op: submodule {name!r} is not part of {kind}'s structure")
            sub.training = training
            if isinstance(sub, nn.BatchNorm2d):
                sub.momentum, sub.eps = e[2], e[3]
                if not e[4]:
                    sub.weight = sub.bias = None
                if not e[5]:
                    sub.track_running_stats = False
                    sub.register_buffer("running_mean", None)
                    sub.register_buffer("running_var", None)
                    sub.register_buffer("num_batches_tracked", None)
            elif isinstance(sub, nn.LeakyReLU):
                sub.negative_slope = e[2]
            elif isinstance(sub, nn.GELU):
                sub.approximate = e[2]
            elif len(e) > 2 and hasattr(sub, "mix_precision"):
                sub.mix_precision = e[2]
            elif len(e) > 2 and e[2] == "run_lfu" and hasattr(sub, "run_lfu"):
                sub.run_lfu = True
        self.kind, self.module = kind, mod
        self.param_names = [n for n, _ in mod.named_parameters()]
        self.buffer_names = [n for n, _ in mod.named_buffers()]
        self._slots = [self._slot(mod, n, "_parameters") for n in self.param_names] + \
                      [self._slot(mod, n, "_buffers") for n in self.buffer_names]
        self._meta = [getattr(sub, kind)[leaf] for sub, kind, leaf in self._slots]

    @staticmethod
    def _slot(mod, name, kind):
        path, _, leaf = name.rpartition(".")
        return (mod.get_submodule(path) if path else mod), kind, leaf

    @contextlib.contextmanager
    def bound(self, params, buffers):
        """this instance with the op's tensors in place of its parameters and buffers (the caller
        holds the instance exclusively: _TemplatePool.bound)"""
        ts = list(params) + list(buffers)
        if len(ts) != len(self._slots):
            raise RuntimeError(f"layer op: {len(ts)} tensors for {len(self._slots)} slots")
        for (sub, kind, leaf), t in zip(self._slots, ts):
            getattr(sub, kind)[leaf] = t
        try:
            yield self.module
        finally:
            for (sub, kind, leaf), t in zip(self._slots, self._meta):
                getattr(sub, kind)[leaf] = t


class _TemplatePool:
    """the template instances of one spec (an rt.StreamPool).  A layer op checks an instance out for
    the whole forward -- binding, launches, unbinding -- and returns it afterwards; the pool's lock
    covers only the check-out and the return.  Concurrent callers (nn.DataParallel-style threads,
    each on its own stream: SURVEY.md §8b "Threading", /root/reference/train_cond.py:66-68) therefore
    run on different instances, and an instance's plan caches, packed weights and split-K partial
    buffers (all kept on its modules) are used by one thread at a time, in stream order."""

    def __init__(self, spec: str):
        self.spec = spec
        self.pool = rt.StreamPool(lambda: _Template(spec))
        first = self.pool.first()
        # structure shared by every instance (fake impls, layer_tensors)
        self.kind, self.module = first.kind, first.module
        self.param_names, self.buffer_names = first.param_names, first.buffer_names

    @property
    def instances(self) -> int:
        return self.pool.instances

    @contextlib.contextmanager
    def bound(self, params, buffers):
        """a template instance of this spec held exclusively, with the op's tensors bound in"""
        rt.note_tensors(params)
        with self.pool.hold() as inst, inst.bound(params, buffers) as m:
            yield m


def template(spec: str) -> _TemplatePool:
    """the spec's template pool under the current plan switches (rt.plan_knobs: the templates' plan
    caches are made under them)"""
    return _template(spec, rt.plan_knobs())


@functools.lru_cache(maxsize=512)
def _template(spec: str, knobs) -> _TemplatePool:
    return _TemplatePool(spec)


def layer_tensors(m: nn.Module, spec: str):
    """(params, buffers) of module m in its template's slot order.  Parameters are read as attributes,
    so a spectral-norm wrapped conv contributes its normalised weight (refreshed by the caller)."""
    tpl = template(spec)

    def get(name):
        path, _, leaf = name.rpartition(".")
        return getattr(m.get_submodule(path) if path else m, leaf)
    return [get(n) for n in tpl.param_names], [get(n) for n in tpl.buffer_names]


# ---------------------------------------------------------------- output shapes of a layer (fake impls)
def _conv_out_hw(conv, H, W):
    if isinstance(conv, nn.ConvTranspose2d):
        k, s, p, d, op = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0], conv.output_padding[0]
        return _plan.convT_out(H, k, s, p, d, op), _plan.convT_out(W, k, s, p, d, op)
    k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
    return _plan.conv_out(H, k, s, p, d), _plan.conv_out(W, k, s, p, d)


def _st_out_shape(st, x):
    B, _, H, W = x.shape
    if st.stride == 2 and st.upsample:
        H, W = 2 * H, 2 * W
    elif st.stride == 2:
        H, W = H // 2, W // 2
    return (B, st.conv2.out_channels, H, W)


def ffc_out_shapes(ffc, x_l, x_g):
    """(shape of out_l or None, shape of out_g or None) of FFC / FFCTranspose ``ffc`` (ffc.py:84-99):
    a branch is None when it is the int 0 of the tuple protocol"""
    from .ffc.spectral_transform import SpectralTransform

    def branch(parts):
        for mod, t in parts:
            if t is None:
                continue
            if isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
                h, w = _conv_out_hw(mod, t.shape[2], t.shape[3])
                return (t.shape[0], mod.out_channels, h, w)
            if isinstance(mod, SpectralTransform):
                return _st_out_shape(mod, t)
            if isinstance(mod, nn.Identity):
                return tuple(t.shape)
        return None
    sl = branch([(ffc.convl2l, x_l), (ffc.convg2l, x_g)]) if ffc.ratio_gout != 1 else None
    sg = branch([(ffc.convl2g, x_l), (ffc.convg2g, x_g)]) if ffc.ratio_gout != 0 else None
    return sl, sg


# ---------------------------------------------------------------- ffc::ffc_bn_act
@torch.library.custom_op("ffc::ffc_bn_act", mutates_args=("buffers",))
def ffc_bn_act(x_l: Optional[Tensor], x_g: Optional[Tensor], params: List[Tensor], buffers: List[Tensor],
               noise: List[Tensor], pending: List[Tensor], pending_act: List[float], defer: bool,
               spec: str) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """one layer's forward.  noise: [] or NoiseInjection (weight_l, noise_l, weight_g, noise_g) applied
    after the BN + activation (fgan128_complete.py:496-515); pending: [] or the deferred BN + activation
    (+ noise) of the inputs, (scale_l, shift_l, weight_l, noise_l, scale_g, ...) with pending_act =
    (act_l, param_l, act_g, param_g) (zero-size tensors for absent parts); defer: return (raw, scale,
    shift) per output branch instead of applying BN + activation (+ noise).
    -> (out_l, out_g, scale_l, shift_l, scale_g, shift_g): zero-size tensors for the int-0 branches of
    the tuple protocol and, unless defer, for the scales / shifts (a fixed-arity tuple: the op
    mutates its buffers, and functionalization takes no list outputs beside mutated arguments)"""
    tpl = template(spec)
    with tpl.bound(params, buffers) as m:
        x_in = _pending_inputs(x_l, x_g, pending, pending_act)
        nz = None
        if noise:
            from .layers_misc import NoiseInjection
            nz = {}
            for k, (w, n) in (("l", noise[0:2]), ("g", noise[2:4])):
                if w.numel():
                    mod = NoiseInjection.__new__(NoiseInjection)
                    nn.Module.__init__(mod)
                    mod._parameters["weight"] = w
                    nz[k] = (mod, n)
        if tpl.kind == "FFC_BN_ACT":
            bn_l, bn_g = m._norm(m.bn_l), m._norm(m.bn_g)
            out = m.ffc._run(x_in, None, rt.act_code(m.act_l), rt.act_code(m.act_g), bn_l, bn_g, noise=nz,
                             defer=defer)
        else:
            out = m._run(x_in, None, noise=nz, defer=defer)
    ref = x_l if x_l is not None else x_g
    res = [ref.new_empty(0) for _ in range(6)]
    for k, o in enumerate(out):
        if isinstance(o, rt.PendingAct):
            res[k], res[2 + 2 * k], res[3 + 2 * k] = o.raw, o.scale, o.shift
        elif isinstance(o, torch.Tensor):
            res[k] = o
    return tuple(res)


def _pending_inputs(x_l, x_g, pending, pending_act):
    if not pending:
        return (x_l if x_l is not None else 0, x_g if x_g is not None else 0)
    xs = []
    for k, x in enumerate((x_l, x_g)):
        sc, sh, w, n = pending[4 * k: 4 * k + 4]
        if x is None:
            xs.append(0)
        elif sc.numel():
            xs.append(rt.PendingAct.from_tensors(x, sc, sh, int(pending_act[2 * k]), pending_act[2 * k + 1],
                                                 w if w.numel() else None, n if n.numel() else None))
        else:
            xs.append(x)
    return tuple(xs)


@ffc_bn_act.register_fake
def _(x_l, x_g, params, buffers, noise, pending, pending_act, defer, spec):
    tpl = template(spec)
    ffc = tpl.module.ffc if tpl.kind == "FFC_BN_ACT" else tpl.module
    ref = x_l if x_l is not None else x_g
    res = [ref.new_empty(0) for _ in range(6)]
    for k, shp in enumerate(ffc_out_shapes(ffc, x_l, x_g)):
        if shp is None:
            continue
        res[k] = ref.new_empty(shp)
        if defer:
            res[2 + 2 * k], res[3 + 2 * k] = ref.new_empty(shp[1]), ref.new_empty(shp[1])
    return tuple(res)


# ---------------------------------------------------------------- ffc::spectral_transform / ffc::fourier_unit
@torch.library.custom_op("ffc::spectral_transform", mutates_args=("buffers",))
def spectral_transform(x: Tensor, params: List[Tensor], buffers: List[Tensor], spec: str) -> Tensor:
    tpl = template(spec)
    with tpl.bound(params, buffers) as m:
        return m._forward_fused(x)


@spectral_transform.register_fake
def _(x, params, buffers, spec):
    return x.new_empty(_st_out_shape(template(spec).module, x))


@torch.library.custom_op("ffc::fourier_unit", mutates_args=("buffers",))
def fourier_unit(x: Tensor, params: List[Tensor], buffers: List[Tensor], spec: str) -> Tensor:
    tpl = template(spec)
    with tpl.bound(params, buffers) as m:
        return m._run(rt.require(x, "x"))


@fourier_unit.register_fake
def _(x, params, buffers, spec):
    return torch.empty_like(x)


# =========================================================================== module-facing helpers
def _refresh_sn(m: nn.Module):
    """spectral-norm pre-hooks of every conv in m, where the reference's module calls would run them"""
    for sub in m.modules():
        if isinstance(sub, (nn.Conv2d, nn.ConvTranspose2d)):
            rt.sn_refresh(sub)


def layer_forward(m: nn.Module, x, noise=None, defer=False):
    """FFC_BN_ACT / FFC / FFCTranspose inference forward through ffc::ffc_bn_act.
    noise: {"l"|"g": (NoiseInjection, noise or None)}; defer: rt.PendingAct outputs.
    -> (out_l, out_g) with the int 0 for absent branches"""
    x_l, x_g = x if type(x) is tuple else (x, 0)
    pend = []
    pact = []
    ins = []
    for v in (x_l, x_g):
        if isinstance(v, rt.PendingAct):
            ins.append(v.raw)
        elif isinstance(v, torch.Tensor):
            ins.append(rt.require(v, "x"))
        else:
            ins.append(None)
    ref = next((t for t in ins if t is not None), None)
    if ref is None:
        raise TypeError("FFC input has no tensor branch")
    e = ref.new_empty(0) if noise or any(isinstance(v, rt.PendingAct) for v in (x_l, x_g)) else None   # placeholder
    if any(isinstance(v, rt.PendingAct) for v in (x_l, x_g)):
        for v in (x_l, x_g):
            if isinstance(v, rt.PendingAct):
                pend += [v.scale, v.shift, v.noise_w if v.noise_w is not None else e,
                         v.noise if v.noise is not None else e]
                pact += [float(v.act), float(v.param)]
            else:
                pend += [e, e, e, e]
                pact += [0.0, 0.0]
    _refresh_sn(m)
    spec = layer_spec(m)
    tpl = template(spec)
    ffc = tpl.module.ffc if tpl.kind == "FFC_BN_ACT" else tpl.module
    shapes = ffc_out_shapes(ffc, ins[0], ins[1])
    nz = []
    if noise:
        for k, shp in zip(("l", "g"), shapes):
            mod, n = noise.get(k, (None, None))
            if mod is None or shp is None:
                nz += [e, e]
                continue
            if n is None:   # drawn here, in branch order, as NoiseInjection draws it (noise_injection.py:26-28)
                n = ref.new_empty((shp[0], 1, shp[2], shp[3])).normal_()
            nz += [mod.weight.detach(), rt.require(n, "noise")]
    params, buffers = layer_tensors(m, spec)
    res = torch.ops.ffc.ffc_bn_act(ins[0], ins[1], params, buffers, nz, pend, pact, bool(defer), spec)
    out = []
    for k, (name, shp) in enumerate(zip(("l", "g"), shapes)):
        if shp is None:
            out.append(0)
        elif defer:
            raw, sc, sh = res[k], res[2 + 2 * k], res[3 + 2 * k]
            act = rt.act_code(m.act_l if name == "l" else m.act_g) if hasattr(m, "act_l") else (0, 0.0)
            w, n = (nz[0:2] if name == "l" else nz[2:4]) if nz else (None, None)
            out.append(rt.PendingAct.from_tensors(raw, sc, sh, act[0], act[1], w if w is not None and w.numel() else None,
                                                  n if n is not None and n.numel() else None))
        else:
            out.append(res[k])
    return tuple(out)


def st_forward(st: nn.Module, x):
    _refresh_sn(st)
    spec = layer_spec(st)
    params, buffers = layer_tensors(st, spec)
    return torch.ops.ffc.spectral_transform(rt.require(x, "x"), params, buffers, spec)


def fu_forward(fu: nn.Module, x):
    spec = layer_spec(fu)
    params, buffers = layer_tensors(fu, spec)
    return torch.ops.ffc.fourier_unit(rt.require(x, "x"), params, buffers, spec)
