"""fp64 expectation of SpectralTransform with its local Fourier unit (LFU) running.

The reference keeps the LFU call in a comment (layers/ffc/spectral_transform.py:94-108) and never
executes it, so there is no reference golden for this branch: the expectation is this restatement of
the semantics, built on oracle.ffc_oracle.fourier_unit for both Fourier units and plain torch ops
(in the dtype of the inputs: float64 for parity) for SE / conv1 / bn1 / conv2.

    s   = relu(bn1(conv1(se(downsample(x)))))                       (B, c, H, W)
    xs  = quadrants of s[:, :c/4] stacked on channels               (B, c, H/2, W/2)
          (top-left, bottom-left, top-right, bottom-right)
    ys  = lfu(xs)                                                   a FourierUnitSN, its own BN
    out = conv2(s + fu(s) + ys.repeat(1, 1, 2, 2))
"""
import torch
import torch.nn.functional as F

from oracle import ffc_oracle as O


def lfu_split(s):
    """steps 1-4: first c/4 channels, halves along H stacked on channels, then halves along W"""
    B, c, H, W = s.shape
    xs = s[:, :c // 4]
    xs = torch.cat(torch.split(xs, H // 2, dim=-2), dim=1)
    return torch.cat(torch.split(xs, W // 2, dim=-1), dim=1).contiguous()


def lfu_tile(ys):
    return ys.repeat(1, 1, 2, 2)


def spectral_transform_lfu(x, sd, prefix, stride, upsample, training, fft="numpy", run_lfu=True):
    """SpectralTransform.forward with the LFU (run_lfu=False: the oracle's spectral_transform, op for
    op).  fft="torch" keeps the FFTs differentiable (fp64 autograd of the restatement)."""
    if stride == 2 and upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    elif stride == 2:
        x = F.avg_pool2d(x, 2, 2)
    x = O.se_layer(x, sd, prefix + "se_block.")
    x = F.conv2d(x, sd[prefix + "conv1.weight"].to(x.dtype))
    s = F.relu(O.batch_norm(x, sd, prefix + "bn1.", training))
    v = s + O.fourier_unit(s, sd, prefix + "fu.", training, fft)
    if run_lfu:
        v = v + lfu_tile(O.fourier_unit(lfu_split(s), sd, prefix + "lfu.", training, fft))
    return F.conv2d(v, sd[prefix + "conv2.weight"].to(x.dtype))


def random_state(mod, seed, running=False):
    """seeded fp32 state for a drop-in module (fan-in scaled weights, BN affine near 1 / 0; running:
    randomised running statistics for eval-mode cases) -> state_dict of CPU tensors"""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in mod.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=gen) if running else torch.ones_like(v)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(v.shape, generator=gen) if running else torch.zeros_like(v)
        elif v.dim() == 1:
            sd[k] = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=gen)
        else:
            fan = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=gen) / max(1.0, fan) ** 0.5
    return sd


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
