"""The float64 references of tests/spectral_refs.py against independent statements of the same
operations (the module oracle, explicit DFT matrices, torch.nn layers), to 1e-12: what
test_gpu_spectral_kernels.py compares the kernels with is itself checked here, without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import spectral_refs as sr
from oracle import ffc_oracle as O

TOL = 1e-12


def _close(a, b, tol=TOL):
    e = O.normwise_err(a, b)
    assert e <= tol, e


def _fu_forward(d, relu, up, training, rm=None, rv=None):
    """the ffc_fu_forward composition: fu_stages -> BN (batch statistics through channel_stats /
    bn_finalize, or the running ones) -> fu_out"""
    s, Z, Y = sr.fu_stages(d["t"], d["in_scale"], d["in_shift"], relu, up, d["wmix"])
    if training:
        n, mean, var = sr.channel_stats(Y)
        scale, shift, rm, rv, nbt = sr.bn_finalize(n, mean, var, d["gamma"], d["beta"], running_mean=rm, running_var=rv,
                                                   num_batches_tracked=0)
    else:
        scale = d["gamma"].double() / torch.sqrt(rv.double() + sr.BN_EPS)
        shift = d["beta"].double() - rm.double() * scale
        nbt = 0
    H, W = d["t"].shape[2] * up, d["t"].shape[3] * up
    return s, sr.fu_out(Y, scale, shift, s, False, H, W), rm, rv, nbt


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("C,h,w", [(3, 4, 8), (5, 8, 4)])
def test_fu_composition_matches_module_oracle(training, up, C, h, w):
    d = sr.fu_inputs(2, C, h, w, up, True, True)
    gen = torch.Generator().manual_seed(5)
    rm0 = 0.1 * torch.randn(2 * C, generator=gen, dtype=torch.float64)
    rv0 = 0.5 + torch.rand(2 * C, generator=gen, dtype=torch.float64)
    s, out, rm, rv, nbt = _fu_forward(d, True, up, training, rm0.clone(), rv0.clone())
    sd = {"fu.conv_layer.weight": d["wmix"].double().reshape(2 * C, 2 * C, 1, 1), "fu.bn.weight": d["gamma"].double(),
          "fu.bn.bias": d["beta"].double(), "fu.bn.running_mean": rm0.clone(), "fu.bn.running_var": rv0.clone(),
          "fu.bn.num_batches_tracked": torch.tensor(0)}
    for fft in ("numpy", "torch"):
        sdc = {k: v.clone() for k, v in sd.items()}
        _close(out, O.fourier_unit(s, sdc, "fu.", training, fft))
    if training:
        _close(rm, sdc["fu.bn.running_mean"])
        _close(rv, sdc["fu.bn.running_var"])
        assert nbt == int(sdc["fu.bn.num_batches_tracked"]) == 1


def test_fu_input_transform_and_upsample():
    d = sr.fu_inputs(2, 3, 4, 6, 2, True, True)
    s, _, _ = sr.fu_stages(d["t"], d["in_scale"], d["in_shift"], True, 2, d["wmix"])
    pre = d["t"].double() * d["in_scale"].double()[None, :, None, None] + d["in_shift"].double()[None, :, None, None]
    assert pre.abs().min() >= sr.KINK
    assert torch.equal(s, F.interpolate(F.relu(pre), scale_factor=2, mode="nearest"))
    s1, _, _ = sr.fu_stages(d["t"], None, None, False, 1, d["wmix"])
    assert torch.equal(s1, d["t"].double())


def _dft(n, sign):
    k = torch.arange(n, dtype=torch.float64)
    ang = sign * 2 * math.pi * torch.outer(k, k) / n
    return torch.complex(torch.cos(ang), torch.sin(ang))


def test_Z_matches_dft_matrices_on_a_non_square_plane():
    H, W, C = 4, 8, 3
    d = sr.fu_inputs(2, C, H, W, 1, False, False)
    s, Z, Y = sr.fu_stages(d["t"], None, None, False, 1, d["wmix"])
    X = _dft(H, -1) @ torch.complex(s, torch.zeros_like(s)) @ _dft(W, -1)[:, :W // 2 + 1] / math.sqrt(H * W)
    _close(Z[:, 0::2], X.real)
    _close(Z[:, 1::2], X.imag)
    ref = torch.zeros_like(Y)
    for o in range(2 * C):
        for i in range(2 * C):
            ref[:, o] += d["wmix"][o, i].double() * Z[:, i]
    _close(Y, ref)


def test_fu_out_matches_inverse_dft_matrices():
    """irfftn through explicit matrices: the half spectrum completed by Hermitian symmetry"""
    H, W = 8, 4
    d = sr.fu_case(2, 3, H, W, 1, False, False)
    Yb = sr.spectrum_of(sr.bn_relu(d["Y"], d["bn_scale"], d["bn_shift"]))
    cols = torch.einsum("yk,bckx->bcyx", _dft(H, +1), Yb)          # inverse over H, unnormalised
    out = torch.zeros(2, 3, H, W, dtype=torch.float64)
    for x in range(W):
        for k in range(W // 2 + 1):
            ph = 2 * math.pi * k * x / W
            wgt = 1.0 if k in (0, W // 2) else 2.0
            term = cols[..., k].real * math.cos(ph) - (0.0 if k in (0, W // 2) else 1.0) * cols[..., k].imag * math.sin(ph)
            out[..., x] += wgt * term
    _close(d["out"], out / math.sqrt(H * W))
    _close(d["out_res"], d["out"] + d["s"])


@pytest.mark.parametrize("up", [1, 2])
def test_staged_stages_recombine_to_fu_out(up):
    h = 8
    H = W = h * up
    d = sr.fu_case(2, 3, h, h, up, True, True)
    # T is the unnormalised spectrum of the un-upsampled input: with up = 1 it is Z * sqrt(H W)
    T = sr.fu2d_T(d["t"], d["in_scale"], d["in_shift"], True)
    s0 = sr.fu_input(d["t"], d["in_scale"], d["in_shift"], True)
    X = _dft(h, -1) @ torch.complex(s0, torch.zeros_like(s0)) @ _dft(h, -1)[:, :h // 2 + 1]
    _close(T, torch.view_as_real(X))
    if up == 1:
        _close(T[..., 0], d["Z"][:, 0::2] * math.sqrt(H * W))
        _close(T[..., 1], d["Z"][:, 1::2] * math.sqrt(H * W))
    Y5 = sr.fu2d_Y(d["Y"])
    assert torch.equal(Y5[..., 0], d["Y"][:, 0::2]) and torch.equal(Y5[..., 1], d["Y"][:, 1::2])
    Yc = sr.fu2d_Yc(d["Y"], d["bn_scale"], d["bn_shift"])
    assert Yc.shape == (2, 3, W // 2 + 1, H, 2)
    cols = torch.einsum("yk,bckx->bcxy", _dft(H, +1), sr.spectrum_of(sr.bn_relu(d["Y"], d["bn_scale"], d["bn_shift"])))
    _close(Yc, torch.view_as_real(cols))
    _close(sr.fu2d_rows(Yc, d["s"], False, H, W), d["out"])
    _close(sr.fu2d_rows(Yc, d["s"], True, H, W), d["out_res"])


def test_irfft_ignores_imaginaries_of_bins_0_and_nyquist():
    H = W = 8
    d = sr.fu_case(1, 2, H, W, 1, False, False)
    Yc = sr.fu2d_Yc(d["Y"], d["bn_scale"], d["bn_shift"])
    bent = Yc.clone()
    bent[:, :, 0, :, 1] += 3.0
    bent[:, :, W // 2, :, 1] -= 5.0
    assert torch.equal(sr.fu2d_rows(bent, d["s"], False, H, W), sr.fu2d_rows(Yc, d["s"], False, H, W))
    bent = Yc.clone()
    bent[:, :, 1, :, 1] += 3.0      # any other bin's imaginary counts
    assert O.normwise_err(sr.fu2d_rows(bent, d["s"], False, H, W), d["out"]) > 1e-2
    # the same for the one-step inverse: a purely imaginary change of the ky-symmetric bins of
    # columns 0 and W/2 leaves irfftn's output alone
    Y = d["Y"].clone()
    for ky in (0, H // 2):
        Y[:, 1::2, ky, 0] += 2.0
        Y[:, 1::2, ky, W // 2] -= 1.5
    _close(_irfft_plain(Y, H, W), _irfft_plain(d["Y"], H, W))


def _irfft_plain(Y, H, W):
    return torch.fft.irfftn(sr.spectrum_of(Y), s=(H, W), dim=(-2, -1), norm="ortho")


def test_kink_free_fu_case():
    d = sr.fu_case(3, 5, 8, 4, 2, True, True)
    pre = d["Y"] * d["bn_scale"].double()[None, :, None, None] + d["bn_shift"].double()[None, :, None, None]
    assert pre.abs().min() >= sr.KINK
    # the beta that the case hands to an in-kernel fold reproduces the cleared shift
    n, mean, var = d["stats"]
    scale, shift, _, _, _ = sr.bn_finalize(n, mean, var, d["gamma"], d["beta"])
    assert (d["Y"] * scale[None, :, None, None] + shift[None, :, None, None]).abs().min() >= sr.KINK
    torch.testing.assert_close(shift, d["bn_shift"].double(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("parts", [(), (1,), (7, 7, 100), (5, 64, 65, 300)])
def test_merge_slab_of_a_partition_is_the_direct_statistics(parts):
    x = torch.randn(3, 6, 11, 13, generator=torch.Generator().manual_seed(1)) * 3 + 5
    # exact float64 rows (make_slab rounds to float32: checked at its own tolerance below)
    xd = x.double().transpose(0, 1).reshape(6, -1)
    edges = [0] + list(parts) + [xd.shape[1]]
    rows = []
    for a, b in zip(edges[:-1], edges[1:]):
        seg = xd[:, a:b]
        m = seg.mean(dim=1) if b > a else torch.zeros(6, dtype=torch.float64)
        rows.append(torch.stack((torch.full((6,), float(b - a), dtype=torch.float64), m,
                                 ((seg - m[:, None]) ** 2).sum(dim=1)), dim=1))
    n, mean, var = sr.merge_slab(torch.stack(rows))
    n0, mean0, var0 = sr.channel_stats(x)
    assert torch.equal(n, torch.full((6,), n0, dtype=torch.float64))
    _close(mean, mean0)
    _close(var, var0)
    n32, mean32, var32 = sr.merge_slab(sr.make_slab(x, parts))
    assert torch.equal(n32, n)
    torch.testing.assert_close(mean32, mean0, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(var32, var0, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_bn_finalize_matches_batchnorm2d(momentum):
    C = 5
    bn = torch.nn.BatchNorm2d(C, momentum=momentum).double().train()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=gen, dtype=torch.float64))
    rm = torch.zeros(C, dtype=torch.float64)
    rv = torch.ones(C, dtype=torch.float64)
    nbt = 0
    for step in range(3):
        x = torch.randn(4, C, 3, 5, generator=gen, dtype=torch.float64) * (step + 1) + step
        y = bn(x)
        n, mean, var = sr.channel_stats(x)
        scale, shift, rm, rv, nbt = sr.bn_finalize(n, mean, var, bn.weight.detach(), bn.bias.detach(), bn.eps,
                                                   -1.0 if momentum is None else momentum, 1.0, rm, rv, nbt)
        _close(x * scale[None, :, None, None] + shift[None, :, None, None], y)
        _close(rm, bn.running_mean)
        _close(rv, bn.running_var)
        assert nbt == int(bn.num_batches_tracked)
    # count_mult: the statistics of one shard standing for count_mult equal shards
    _, _, _, rv2, _ = sr.bn_finalize(n, mean, var, None, None, bn.eps, 1.0, 2.0, rm, rv, 0)
    _close(rv2, var * (2 * n) / (2 * n - 1))


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("hidden", [0, 1, 4])
def test_st_prologue_matches_torch_layers(pool, hidden):
    B, Cin, c, H, W = 3, 12, 7, 6, 4
    x, w1, w2, wconv1 = sr.st_inputs(B, Cin, c, H, W, pool, hidden)
    gate, t, (n, mean, var) = sr.st_prologue(x, pool, w1, w2, wconv1)
    xd = torch.nn.AvgPool2d(2, 2)(x.double()) if pool else x.double()
    if hidden:
        fc = torch.nn.Sequential(torch.nn.Linear(Cin, hidden, bias=False), torch.nn.ReLU(),
                                 torch.nn.Linear(hidden, Cin, bias=False), torch.nn.Sigmoid()).double()
        with torch.no_grad():
            fc[0].weight.copy_(w1.double())
            fc[2].weight.copy_(w2.double())
            g = fc(xd.mean(dim=(2, 3)))
            assert (fc[0](xd.mean(dim=(2, 3)))).abs().min() >= sr.KINK
    else:
        g = torch.full((B, Cin), 0.5, dtype=torch.float64)
    _close(gate, g)
    _close(sr.se_gate(x, pool, w1, w2), g)
    tt = F.conv2d(xd * g[:, :, None, None], wconv1.double()[:, :, None, None])
    _close(t, tt)
    _close(sr.pw_gate_conv(xd.reshape(B, Cin, -1), g, wconv1), tt.reshape(B, c, -1))
    _close(sr.pw_gate_conv(xd, None, wconv1), F.conv2d(xd, wconv1.double()[:, :, None, None]))
    assert n == tt.numel() // c
    _close(mean, tt.mean(dim=(0, 2, 3)))
    _close(var, tt.var(dim=(0, 2, 3), unbiased=False))
    # the sd-driven oracle states the same SELayer
    if hidden:
        sd = {"se.fc.0.weight": w1.double(), "se.fc.2.weight": w2.double()}
        _close(xd * gate[:, :, None, None], O.se_layer(xd, sd, "se."))


@pytest.mark.parametrize("act", [0, 2, 5])
def test_dense_matches_linear(act):
    A, Wt, bias = sr.dense_inputs(5, 9, 6, True, act)
    ref = F.linear(A.double(), Wt.double().t(), bias.double())
    if act == 2:
        assert ref.abs().min() >= sr.KINK
    _close(sr.dense(A, Wt, bias, act), O.activation(ref, O.ACTS[act]))
    A, Wt, bias = sr.dense_inputs(2, 3, 4, False, 0)
    assert bias is None
    _close(sr.dense(A, Wt, None, 0), A.double() @ Wt.double())


def test_clear_offset_picks_the_nearest_gap():
    v = torch.tensor([0.0, 0.001, 0.002, 1.0], dtype=torch.float64)
    off = sr.clear_offset(v, 0.0)
    assert (v + off).abs().min() >= 2.4 * sr.KINK and abs(off) <= 5 * sr.KINK
    assert sr.clear_offset(v, 0.5) == 0.5
