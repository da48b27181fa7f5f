"""Self_Attn (layers/attention_layer.py:8-40) on the fused HIP attention of csrc/attn_kernels.hip."""
import torch
import torch.nn as nn


class Self_Attn(nn.Module):
    """Self attention layer with the reference's constructor, attributes and state_dict keys.

    forward(x) -> (out, attention): out = gamma * (value . softmax(query^T key)^T) + x, computed by one
    stacked 1x1 projection on the pointwise GEMM and one flash-style kernel that never writes an N x N
    matrix (N = H * W).  ``attention`` (B, N, N) is written by a second kernel, only because the
    reference returns it: it carries NO gradient (no caller in the reference differentiates through it;
    gradients flow through ``out`` alone).  Set ``need_attention = False`` to skip it: forward then
    returns (out, None) and nothing of size N x N is allocated.

    x: (B, C, H, W) fp32 on the GPU with C % 8 == 0 and 8 <= C <= 256 (NotImplementedError otherwise);
    C <= 64 runs the ffc_attn_* entry points, 72 <= C <= 256 the wide ffc_attnw_* ones.
    There is no CPU fallback."""

    need_attention = True

    def __init__(self, in_dim, activation):
        super().__init__()
        self.chanel_in = in_dim
        self.activation = activation
        self.query_conv = nn.Conv2d(in_channels=in_dim, out_channels=in_dim // 8, kernel_size=1)
        self.key_conv = nn.Conv2d(in_channels=in_dim, out_channels=in_dim // 8, kernel_size=1)
        self.value_conv = nn.Conv2d(in_channels=in_dim, out_channels=in_dim, kernel_size=1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x):
        from . import _autograd as ag
        return ag.self_attn(self, x)
