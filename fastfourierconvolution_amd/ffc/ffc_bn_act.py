"""Drop-in ``FFC_BN_ACT`` (reference: layers/ffc/ffc_bn_act.py:11-83): the model-facing block.

forward runs the ``ffc::ffc_bn_act`` custom op (ops.py; the training ops under autograd).  The
activation is fused into the local-branch GEMM epilogue; with norm_layer=BatchNorm2d the GEMM
epilogue collects BN partials and one BN+activation pass follows.

With norm_layer=ConditionalBatchNorm2d (cond_bn.py) the FFC part runs as its own layer op and each
branch's conditional norm + activation (+ NoiseInjection) is one ``ffc::cbn_act`` pass.  By default
the labels also go into the FFC part, as in the reference, which raises TypeError where they reach a
SpectralTransform (fourier_unity.py:46-47); ``set_cond_bn`` makes them condition bn_l / bn_g only --
what the reference's constructors build (spectral_transform.py:54-57, fourier_unity.py:25-28).
"""
import torch
import torch.nn as nn

from .. import _autograd as ag
from .. import _runtime as rt
from .cond_bn import ConditionalBatchNorm2d
from .ffc import FFC, layer_call
from .ffc_transpose import FFCTranspose
from .spectral_transform import SpectralTransform


def set_cond_bn(model: nn.Module, on: bool = True) -> nn.Module:
    """labels condition only bn_l / bn_g of every FFC_BN_ACT of ``model`` (``cond_bn_only``): the FFC part,
    spectral branch included, runs without them.  Off (the default): the reference's forward, which
    raises TypeError when a label reaches a SpectralTransform.  State dicts are the same either way."""
    for m in model.modules():
        if isinstance(m, FFC_BN_ACT):
            m.cond_bn_only = bool(on)
    return model


class FFC_BN_ACT(nn.Module):
    def __init__(self, in_channels, out_channels,
                 kernel_size, ratio_gin, ratio_gout,
                 stride=1, padding=0, dilation=1, groups=1, bias=False,
                 norm_layer: nn.Module = nn.Identity, activation_layer: nn.Module = nn.Identity,
                 enable_lfu=True, upsampling=False, out_padding=0,
                 uses_noise: bool = False, uses_sn: bool = False, num_classes: int = 1):
        super().__init__()
        self.cond_bn_only = False   # set_cond_bn
        self._ffc_ctor = ["FFC_BN_ACT", dict(in_channels=in_channels, out_channels=out_channels,
                                             kernel_size=kernel_size, ratio_gin=ratio_gin, ratio_gout=ratio_gout,
                                             stride=stride, padding=padding, dilation=dilation, groups=groups,
                                             bias=bias, norm_layer=norm_layer.__name__,
                                             activation_layer=activation_layer.__name__, enable_lfu=enable_lfu,
                                             upsampling=upsampling, out_padding=out_padding,
                                             num_classes=num_classes)]
        self.uses_sn = uses_sn
        if upsampling:
            self.ffc = FFCTranspose(in_channels, out_channels, kernel_size, ratio_gin, ratio_gout, stride, padding,
                                    dilation, groups, bias, enable_lfu, out_padding=out_padding,
                                    num_classes=num_classes)
        else:
            self.ffc = FFC(in_channels, out_channels, kernel_size, ratio_gin, ratio_gout, stride, padding,
                           dilation, groups, bias, enable_lfu, num_classes=num_classes)
        out_ch_l = int(out_channels * (1 - ratio_gout))
        out_ch_g = int(out_channels * ratio_gout)
        lnorm = nn.Identity if ratio_gout == 1 else norm_layer
        gnorm = nn.Identity if ratio_gout == 0 else norm_layer
        if num_classes > 1:
            self.bn_l = lnorm(out_ch_l, num_classes)
            self.bn_g = gnorm(out_ch_g, num_classes)
        else:
            self.bn_l = lnorm(out_ch_l)
            self.bn_g = gnorm(out_ch_g)
        lact = nn.Identity if ratio_gout == 1 else activation_layer
        gact = nn.Identity if ratio_gout == 0 else activation_layer
        self.act_l = lact(0.1, inplace=True) if isinstance(lact(), nn.LeakyReLU) else lact()
        self.act_g = gact(0.1, inplace=True) if isinstance(gact(), nn.LeakyReLU) else gact()

    @staticmethod
    def _norm(m):
        if isinstance(m, nn.Identity):
            return None
        if isinstance(m, (nn.BatchNorm2d, ConditionalBatchNorm2d)):
            return m
        raise NotImplementedError(f"norm layer {type(m).__name__} has no HIP path")

    def _call(self, x, y=None, noise=None, defer=False):
        bn_l, bn_g = self._norm(self.bn_l), self._norm(self.bn_g)
        if isinstance(bn_l, ConditionalBatchNorm2d) or isinstance(bn_g, ConditionalBatchNorm2d):
            return self._call_cond(x, y, bn_l, bn_g, noise)
        if y is not None and (bn_l is not None or bn_g is not None):
            raise TypeError("FFC_BN_ACT: BatchNorm2d.forward() takes no label input (reference ffc_bn_act.py:73-81)")
        return layer_call(self, self.ffc, x, y, rt.act_code(self.act_l), rt.act_code(self.act_g), bn_l, bn_g,
                          noise=noise, defer=defer)

    def _call_cond(self, x, y, bn_l, bn_g, noise):
        """conditional norms (ffc_bn_act.py:70-83 with y): the FFC part, then one conditional
        norm + activation (+ noise) pass per branch; outputs are materialised (never deferred)"""
        if y is None:
            raise TypeError("ConditionalBatchNorm2d.forward() missing 1 required positional argument: 'y'")
        if not all(bn is None or isinstance(bn, ConditionalBatchNorm2d) for bn in (bn_l, bn_g)):
            raise NotImplementedError("FFC_BN_ACT: conditional and plain norms in one layer")
        ffc = self.ffc
        if not self.cond_bn_only and ffc.ratio_gout != 0 and isinstance(ffc.convg2g, SpectralTransform):
            # the reference hands y to SpectralTransform -> FourierUnitSN.bn(ffted, y)
            raise TypeError("FFC_BN_ACT: the label reaches a SpectralTransform, whose BatchNorm2d.forward() takes "
                            "no label (reference fourier_unity.py:46-47); set_cond_bn(model) conditions bn_l / "
                            "bn_g only")
        if rt._sync_group() is not None:
            raise NotImplementedError("ConditionalBatchNorm2d has no SyncBN path (sharded conditional training "
                                      "is not supported)")
        labels = ag.cbn_labels(y)
        outs = layer_call(ffc, ffc, rt.materialize(x), None)
        noise = noise or {}
        res = []
        for name, out, bn, act in (("l", outs[0], bn_l, self.act_l), ("g", outs[1], bn_g, self.act_g)):
            nz = noise.get(name)
            if not isinstance(out, torch.Tensor):
                res.append(out)
            elif bn is not None:
                res.append(ag.cbn_act(bn, out, labels, rt.act_code(act), nz))
            else:
                raise NotImplementedError("FFC_BN_ACT: a tensor branch without its conditional norm")
        return tuple(res)

    def forward(self, x, y=None):
        return self._call(x, y)

    def forward_noise(self, x, noise_l, noise_g, y=None):
        """forward followed by NoiseInjection on both outputs (fgan128_complete.py:496-515), the noise add
        fused into the BN + activation pass.  noise_*: (NoiseInjection module, noise tensor or None)."""
        return self._call(x, y, noise={"l": noise_l, "g": noise_g})

    def forward_deferred(self, x, noise_l=None, noise_g=None, y=None):
        """forward (plus NoiseInjection when noise_* are given, as forward_noise) whose outputs are
        rt.PendingAct: BN + activation + noise are left to the consuming layer, which applies them
        while it stages its operands (or materializes them).  Not for autograd."""
        noise = {k: v for k, v in (("l", noise_l), ("g", noise_g)) if v is not None}
        return self._call(x, y, noise=noise or None, defer=True)
