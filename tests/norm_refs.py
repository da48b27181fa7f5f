"""References and fixed-seed input builders of the batch-norm forward kernels (csrc/bn_se_kernels.hip:
reduce, finalize, apply, plane sums, the SE gate from sums) and of the two caller streams
(csrc/caller_kernels.hip: NoiseInjection, the uint8 quantizer), shared by test_gpu_norm_kernels.py
(kernel against reference on the GPU) and test_norm_refs_cpu.py (reference against torch.nn and the
oracle).

Plain torch on the CPU in float64; inputs are float32 tensors (what the kernels read), widened exactly.
quantize_u8 is the exception: the operation is defined in fp32, so it is stated in fp32, twice.  Nothing
in this file imports the package under test."""
import numpy as np
import torch

from spectral_refs import KINK, SLOPE, act64, make_slab, merge_slab, se_gate  # noqa: F401  (shared, not copied)

BN_EPS = float(np.float32(1e-5))      # the eps the kernels are handed: the float32 nearest 1e-5
SLOPE32 = float(np.float32(SLOPE))    # likewise the LeakyReLU slope
PLANE_CHUNK = 4096                    # PLANE_CHUNK4 * 4 of csrc/bn_se_kernels.hip


def _per_channel(v):
    return v.double()[None, :, None]


# --------------------------------------------------------------------------- statistics
def slab_moments(slab):
    """partial rows [rows][C] {n, mean, M2, -} -> float64 raw moments (n, sum, sumsq), each [C]: what
    ffc_bn_reduce writes (the merge of tests/test_gpu_bn_reduce.py)"""
    s = slab.double()
    return s[..., 0].sum(0), (s[..., 0] * s[..., 1]).sum(0), (s[..., 2] + s[..., 0] * s[..., 1] ** 2).sum(0)


def finalize(n, sum, sumsq, gamma=None, beta=None, eps=BN_EPS, momentum=0.1, count_mult=1.0, running_mean=None,
             running_var=None, num_batches_tracked=0, use_batch_stats=True, update_running=True):
    """nn.BatchNorm2d's rule as finalize_channel (csrc/bn_se_kernels.hip) documents it, from the raw
    moments {n, sum, sumsq} per channel.  Train (use_batch_stats): mean = sum / n, the biased variance
    sumsq / n - mean^2 clamped at 0 normalises; with update_running the running statistics move by
    `momentum` (momentum < 0 or None: the cumulative average 1 / (num_batches_tracked + 1)) towards the mean
    and the unbiased variance over n * count_mult samples -- left biased when n * count_mult <= 1 -- and
    num_batches_tracked grows by one.  Eval: the running statistics normalise, nothing is updated.
    gamma / beta None: 1 / 0.  Returns scale, shift, running_mean, running_var, num_batches_tracked (the
    running values as given, widened, where nothing updates them; None where none were given)."""
    rm = None if running_mean is None else running_mean.double()
    rv = None if running_var is None else running_var.double()
    nbt = int(num_batches_tracked)
    if use_batch_stats:
        n = torch.as_tensor(n, dtype=torch.float64)
        mean = sum.double() / n
        var = (sumsq.double() / n - mean * mean).clamp_min(0.0)
        if update_running:
            fm = 1.0 / (nbt + 1) if momentum is None or momentum < 0 else float(momentum)
            nfull = n * count_mult
            unb = torch.where(nfull > 1.0, var * nfull / (nfull - 1.0).clamp_min(1e-300), var)
            rm = (1.0 - fm) * rm + fm * mean
            rv = (1.0 - fm) * rv + fm * unb
            nbt += 1
    else:
        mean, var = rm, rv
    g = torch.ones_like(mean) if gamma is None else gamma.double()
    b = torch.zeros_like(mean) if beta is None else beta.double()
    scale = g / torch.sqrt(var + eps)
    return scale, b - mean * scale, rm, rv, nbt


# --------------------------------------------------------------------------- apply
def bn_act_apply(x, scale, shift, act, p, noise_w=None, noise=None):
    """act(x * scale[c] + shift[c]) + noise_w[c] * noise[b]; x (B, C, HW), noise (B, 1, HW) or None"""
    y = act64(x.double() * _per_channel(scale) + _per_channel(shift), act, p)
    if noise is not None:
        y = y + _per_channel(noise_w) * noise.double().reshape(x.shape[0], 1, -1)
    return y


def plane_chunk_sums(y, chunk=PLANE_CHUNK):
    """[B][C][chunks] float64 sums of y (B, C, ...) over consecutive runs of `chunk` elements of each plane"""
    yd = y.double().reshape(y.shape[0], y.shape[1], -1)
    return torch.stack([part.sum(dim=2) for part in yd.split(chunk, dim=2)], dim=2)


def noise_inject(x, w, noise):
    """NoiseInjection.forward: x + w[c] * noise[b]; x (B, C, HW), w (C), noise (B, 1, HW)"""
    return x.double() + _per_channel(w) * noise.double().reshape(x.shape[0], 1, -1)


# --------------------------------------------------------------------------- quantizer (fp32)
def quantize_u8(x):
    """uint8(255 * (x * 0.5 + 0.5)), every step in float32, the conversion truncating: torch float32"""
    assert x.dtype == torch.float32
    return (255 * (x * 0.5 + 0.5)).to(torch.uint8)


def quantize_u8_np(x):
    """the same in numpy float32 arithmetic, with the truncation spelled out"""
    a = x.numpy()
    assert a.dtype == np.float32
    v = np.float32(255.0) * (a * np.float32(0.5) + np.float32(0.5))
    assert v.dtype == np.float32
    return torch.from_numpy(np.trunc(v).astype(np.int32).astype(np.uint8))


def quantize_u8_fp64(x):
    """what an fp64 evaluation of the formula would give (not the operation: test_norm_refs_cpu.py counts
    where it differs)"""
    return torch.floor(255 * (x.double() * 0.5 + 0.5)).to(torch.uint8)


QUANT_EDGES = 3 + 3 * 256 - 2


def quantize_inputs(n=1024, seed=0):
    """n float32 values in [-1, 1]: -1, 0, 1; for every k in 0..255 the fp32 neighbours (nextafter down, the
    value, nextafter up) of 2k/255 - 1, the point where 255 * (x/2 + 1/2) crosses k and truncation decides
    the byte (the two neighbours that leave [-1, 1] are dropped); then uniform random values.  Nothing lies
    outside [-1, 1]: the cast of an out-of-range float is undefined in torch."""
    assert n >= QUANT_EDGES
    k = np.arange(256, dtype=np.float64)
    edge = (2.0 * k / 255.0 - 1.0).astype(np.float32)
    vals = np.concatenate((np.array([-1.0, 0.0, 1.0], dtype=np.float32), np.nextafter(edge, np.float32(-2.0)), edge,
                           np.nextafter(edge, np.float32(2.0))))
    vals = vals[(vals >= -1.0) & (vals <= 1.0)]
    assert vals.dtype == np.float32 and vals.size == QUANT_EDGES
    gen = torch.Generator().manual_seed(4000 + seed)
    rnd = (torch.rand(n - vals.size, generator=gen) * 2.0 - 1.0).clamp(-1.0, 1.0)
    return torch.cat((torch.from_numpy(vals), rnd))


# --------------------------------------------------------------------------- input builders
def slab_inputs(nrows, C, seed=0, zero_rows=()):
    """a float32 slab [nrows][C] {n, mean, M2, 0} as _slab of tests/test_gpu_bn_reduce.py builds it (n <= 63
    per row and |mean| of order 1, so the float64 merge alone stays within that file's bound); the rows in
    zero_rows are {0, 0, 0, 0}"""
    gen = torch.Generator().manual_seed(1000 + 7 * nrows + C + 100003 * seed)
    n = torch.randint(1, 64, (nrows, C), generator=gen).double()
    mean = torch.randn((nrows, C), generator=gen, dtype=torch.float64)
    m2 = torch.rand((nrows, C), generator=gen, dtype=torch.float64) * n
    slab = torch.stack([n, mean, m2, torch.zeros_like(n)], dim=-1).float()
    for r in zero_rows:
        slab[r] = 0.0
    return slab


def bn_params(C, seed=0):
    """gamma (both signs), beta, running_mean, running_var"""
    gen = torch.Generator().manual_seed(2000 + C + 1009 * seed)
    gamma = (0.5 + torch.rand(C, generator=gen)) * (1 - 2 * (torch.arange(C) % 2)).float()
    return gamma, 0.2 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen), \
        0.5 + torch.rand(C, generator=gen)


def apply_inputs(B, C, HW, seed=0, with_noise=False):
    """x (B, C, HW), scale (both signs), shift [, noise_w, noise (B, 1, HW): its own draw per sample]"""
    gen = torch.Generator().manual_seed(3000 + 131 * B + 17 * C + HW + 100003 * seed)
    x = torch.randn(B, C, HW, generator=gen) + 0.25
    scale = (0.5 + torch.rand(C, generator=gen)) * (1 - 2 * (torch.arange(C) % 2)).float()
    shift = 0.3 * torch.randn(C, generator=gen)
    if not with_noise:
        return x, scale, shift
    return x, scale, shift, torch.randn(C, generator=gen), torch.randn(B, 1, HW, generator=gen)
