"""Drop-in ``ConditionalBatchNorm2d`` (reference: layers/cond/cond_bn.py:6-24): an affine-less
BatchNorm2d whose scale and shift are, per sample, the two halves of the row of an
``nn.Embedding(num_classes, 2 * num_features)`` that the sample's class label selects.

forward runs the ``ffc::cbn_act`` custom op (ops.py): the batch moments, then one fused pass that
normalises, looks the label's row up on the device and applies it (csrc/cbn_kernels.hip).  The labels
stay on the GPU and are read by the kernels only, so a captured forward replays with new labels
written into the same tensor.  Submodule names, initialisation and state_dict keys are the reference's.
"""
import torch.nn as nn

from .. import _autograd as ag
from .. import _runtime as rt


class ConditionalBatchNorm2d(nn.Module):
    def __init__(self, num_features, num_classes):
        super().__init__()
        self.num_classes = num_classes
        self.num_features = num_features
        self.bn = nn.BatchNorm2d(num_features, affine=False)
        self.embed = nn.Embedding(num_classes, num_features * 2)
        if not self.embed.weight.is_meta:
            self.embed.weight.data[:, :num_features].normal_(1, 0.02)   # scale ~ N(1, 0.02)
            self.embed.weight.data[:, num_features:].zero_()            # shift 0

    def forward(self, x, y):
        """x (B, C, H, W) fp32 and y int64 labels of shape (B,), (B, 1) or (B, 1, 1), both on the GPU"""
        return ag.cbn_act(self, rt.require(x, "x"), y)
