"""The references of tests/norm_refs.py against independent statements of the same operations
(torch.nn.BatchNorm2d in float64, the module oracle), to 1e-12: what test_gpu_norm_kernels.py compares
the kernels with is itself checked here, without a GPU."""
import pytest
import torch
import torch.nn as nn

import norm_refs as nr
from oracle import ffc_oracle as O

TOL = 1e-12
ACT_MODULES = {0: nn.Identity(), 1: nn.ReLU(), 2: nn.LeakyReLU(nr.SLOPE32), 3: nn.Tanh(), 4: nn.Sigmoid(), 5: nn.GELU()}


def _close(a, b, tol=TOL):
    e = O.normwise_err(a, b)
    assert e <= tol, e


def _moments(x):
    xd = x.double().transpose(0, 1).reshape(x.shape[1], -1)
    return float(xd.shape[1]), xd.sum(dim=1), (xd * xd).sum(dim=1)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("training", [True, False])
def test_finalize_matches_batchnorm2d(training, momentum, affine):
    """scale / shift (through the module's output), running statistics and num_batches_tracked over two
    consecutive steps"""
    B, C, H, W = 3, 5, 4, 6
    gen = torch.Generator().manual_seed(21)
    bn = nn.BatchNorm2d(C, eps=nr.BN_EPS, momentum=momentum, affine=affine).double()
    gamma, beta, rm0, rv0 = nr.bn_params(C)
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
        if affine:
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    bn.train(training)
    rm, rv, nbt = rm0.double(), rv0.double(), 0
    for step in range(2):
        x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * (1.0 + step) + 0.4
        with torch.no_grad():
            y = bn(x)
        scale, shift, rm, rv, nbt = nr.finalize(*_moments(x), gamma if affine else None, beta if affine else None,
                                                nr.BN_EPS, momentum, 1.0, rm, rv, nbt, use_batch_stats=training,
                                                update_running=training)
        _close(x * scale[None, :, None, None] + shift[None, :, None, None], y)
        _close(rm, bn.running_mean)
        _close(rv, bn.running_var)
        assert nbt == int(bn.num_batches_tracked) == (step + 1 if training else 0)
    if not training:
        assert torch.equal(rm, rm0.double()) and torch.equal(rv, rv0.double())


def test_finalize_forms_outside_batchnorm2d():
    """what nn.BatchNorm2d has no switch for: update_running off leaves the running values alone; count_mult
    scales the sample count of the unbiased variance only; n * count_mult <= 1 keeps the biased variance (where
    sr.bn_finalize divides by zero); a negative momentum is momentum=None; the variance is clamped at 0"""
    C = 4
    gamma, beta, rm0, rv0 = nr.bn_params(C)
    x = torch.randn(2, C, 3, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    n, s, q = _moments(x)
    mean, var = s / n, q / n - (s / n) ** 2
    sc, sh, rm, rv, nbt = nr.finalize(n, s, q, gamma, beta, running_mean=rm0, running_var=rv0, num_batches_tracked=5,
                                      update_running=False)
    assert torch.equal(rm, rm0.double()) and torch.equal(rv, rv0.double()) and nbt == 5
    _close(sc, gamma.double() / torch.sqrt(var + nr.BN_EPS))
    _close(sh, beta.double() - mean * sc)
    sc4, sh4, rm4, rv4, _ = nr.finalize(n, s, q, gamma, beta, count_mult=4.0, running_mean=rm0, running_var=rv0)
    assert torch.equal(sc4, sc) and torch.equal(sh4, sh)
    _close(rm4, 0.9 * rm0.double() + 0.1 * mean)
    _close(rv4, 0.9 * rv0.double() + 0.1 * var * (4 * n) / (4 * n - 1))
    a = nr.finalize(n, s, q, None, None, momentum=-1.0, running_mean=rm0, running_var=rv0, num_batches_tracked=3)
    b = nr.finalize(n, s, q, None, None, momentum=None, running_mean=rm0, running_var=rv0, num_batches_tracked=3)
    assert all(torch.equal(u, v) for u, v in zip(a[:4], b[:4])) and a[4] == b[4] == 4
    _close(a[2], 0.75 * rm0.double() + 0.25 * mean)
    # one sample: variance 0, biased and unbiased alike, everything finite
    one = torch.tensor([1.5, -2.0, 0.0, 100.0], dtype=torch.float64)
    sc1, sh1, rm1, rv1, _ = nr.finalize(1.0, one, one * one, gamma, beta, running_mean=rm0, running_var=rv0)
    _close(rv1, 0.9 * rv0.double())
    _close(rm1, 0.9 * rm0.double() + 0.1 * one)
    assert all(torch.isfinite(t).all() for t in (sc1, sh1, rm1, rv1))
    # sumsq / n < mean^2 by rounding: the clamp makes the variance 0, not negative
    scn, _, _, _, _ = nr.finalize(3.0, torch.tensor([300.0]), torch.tensor([30000.0 - 1e-9]), None, None,
                                  update_running=False)
    _close(scn, torch.tensor([1.0 / nr.BN_EPS ** 0.5], dtype=torch.float64))


def test_slab_moments_are_the_slab_merge():
    """slab_moments against make_slab / merge_slab of spectral_refs.py: the raw moments of x itself"""
    x = torch.randn(3, 4, 5, 7, generator=torch.Generator().manual_seed(8)) + 0.3
    slab = nr.make_slab(x, (9, 9, 40, 77))          # an empty part among them
    n, s, q = nr.slab_moments(slab)
    n0, s0, q0 = _moments(x)
    assert torch.equal(n, torch.full_like(n, n0))
    assert O.normwise_err(s, s0) <= 1e-6 and O.normwise_err(q, q0) <= 1e-6    # float32 rows
    nm, mean, var = nr.merge_slab(slab)
    _close(mean, s / n)
    assert O.normwise_err(var, q / n - (s / n) ** 2) <= 1e-10


@pytest.mark.parametrize("act", range(6))
@pytest.mark.parametrize("with_noise", [False, True])
def test_bn_act_apply_matches_modules(act, with_noise):
    """nn.BatchNorm2d (train) + activation + the oracle's noise_injection, with finalize's scale / shift"""
    B, C, H, W = 3, 4, 3, 4
    x, _, _, nw, noise = nr.apply_inputs(B, C, H * W, with_noise=True)
    gamma, beta, _, _ = nr.bn_params(C)
    bn = nn.BatchNorm2d(C, eps=nr.BN_EPS).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        ref = ACT_MODULES[act].double()(bn(x.double().reshape(B, C, H, W)))
    if with_noise:
        ref = O.noise_injection(ref, {"n.weight": nw.reshape(1, C, 1, 1)}, "n.", noise.double().reshape(B, 1, H, W))
    scale, shift, _, _, _ = nr.finalize(*_moments(x), gamma, beta, update_running=False)
    got = nr.bn_act_apply(x, scale, shift, act, nr.SLOPE32, nw if with_noise else None, noise if with_noise else None)
    _close(got.reshape(B, C, H, W), ref)


def test_noise_inject_matches_oracle():
    x, _, _, w, noise = nr.apply_inputs(3, 5, 12, with_noise=True)
    ref = O.noise_injection(x.double().reshape(3, 5, 3, 4), {"n.weight": w.reshape(1, 5, 1, 1)}, "n.",
                            noise.double().reshape(3, 1, 3, 4))
    _close(nr.noise_inject(x, w, noise).reshape(3, 5, 3, 4), ref)
    # a different draw per sample: indexing the noise by plane instead of by sample is another tensor
    assert not torch.equal(noise[0], noise[1])


@pytest.mark.parametrize("B,C,HW", [(2, 3, 256), (2, 2, 4100), (1, 3, 16384), (2, 2, 36)])
def test_plane_chunk_sums_add_up_to_the_plane(B, C, HW):
    y = torch.randn(B, C, HW, generator=torch.Generator().manual_seed(HW))
    sums = nr.plane_chunk_sums(y)
    assert sums.shape == (B, C, (HW + 4095) // 4096) and sums.dtype == torch.float64
    _close(sums.sum(dim=2), y.double().sum(dim=2))
    _close(sums[:, :, 0], y.double()[:, :, :4096].sum(dim=2))
    if HW == 4100:
        _close(sums[:, :, 1], y.double()[:, :, 4096:].sum(dim=2))      # the four elements of the second chunk
    _close(nr.plane_chunk_sums(y.reshape(B, C, -1, 4)), sums)           # (B, C, H, W) alike


def test_quantize_u8_statements_agree():
    """the torch-fp32 and numpy-fp32 statements and oracle.ffc_oracle.quantize_u8, byte for byte, on the
    boundary set; printed, not asserted: how many of these inputs an fp64 evaluation would quantize
    differently (the builder sits on the truncation boundaries)"""
    x = nr.quantize_inputs(4096)
    assert x.dtype == torch.float32 and x.min() == -1.0 and x.max() == 1.0 and (x == 0).any()
    a, b, c = nr.quantize_u8(x), nr.quantize_u8_np(x), O.quantize_u8(x)
    assert a.dtype == b.dtype == c.dtype == torch.uint8
    assert torch.equal(a, b) and torch.equal(a, c)
    assert a[x == -1.0].eq(0).all() and a[x == 1.0].eq(255).all() and a[x == 0.0].eq(127).all()
    assert set(a[:nr.QUANT_EDGES].tolist()) == set(range(256))           # every byte value is an outcome
    edges = x[:nr.QUANT_EDGES]
    d64 = nr.quantize_u8_fp64(edges) != a[:nr.QUANT_EDGES]
    print(f"OBS quantize fp64 evaluation differs on {int(d64.sum())} of {nr.QUANT_EDGES} boundary inputs, "
          f"{int((nr.quantize_u8_fp64(x[nr.QUANT_EDGES:]) != a[nr.QUANT_EDGES:]).sum())} of "
          f"{x.numel() - nr.QUANT_EDGES} random ones")


def test_input_builders_are_fixed():
    assert torch.equal(nr.quantize_inputs(1000), nr.quantize_inputs(1000))
    assert torch.equal(nr.slab_inputs(5, 3), nr.slab_inputs(5, 3))
    slab = nr.slab_inputs(7, 3, zero_rows=(0, 4))
    assert torch.equal(slab[[0, 4]], torch.zeros(2, 3, 4)) and (slab[[1, 2, 3, 5, 6], :, 0] >= 1).all()
    assert slab[..., 0].max() <= 63
    for t in nr.apply_inputs(2, 3, 8, with_noise=True):
        assert t.dtype == torch.float32
