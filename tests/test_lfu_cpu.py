"""The local Fourier unit switch (set_lfu / SpectralTransform.run_lfu) and the fp64 restatement the
GPU tests compare against (tests/lfu_refs.py), without a GPU."""
import contextlib
import io

import pytest
import torch

import lfu_refs as R
from oracle import ffc_oracle as O


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_run_lfu_defaults_to_false():
    import fastfourierconvolution_amd as F
    assert F.SpectralTransform(32, 32, enable_lfu=True).run_lfu is False
    assert F.SpectralTransform(32, 32).run_lfu is False
    g = _quiet(F.FFCGenerator, 100, 3, 64)
    sts = [m for m in g.modules() if isinstance(m, F.SpectralTransform)]
    assert sts and not any(m.run_lfu for m in sts)


def test_set_lfu_flips_every_spectral_transform():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd.ffc import set_lfu
    assert set_lfu is F.set_lfu and "set_lfu" in F.__all__
    g = _quiet(F.FFCGenerator, 100, 3, 64)
    sts = [m for m in g.modules() if isinstance(m, F.SpectralTransform)]
    assert len(sts) == 3   # ffc1..ffc3 (ffc0 has no global input, ffc4 no global output)
    assert F.set_lfu(g) is g
    assert all(m.run_lfu is True for m in sts)
    assert F.set_lfu(g, False) is g
    assert not any(m.run_lfu for m in sts)


def test_set_lfu_needs_enable_lfu():
    import fastfourierconvolution_amd as F
    st = F.SpectralTransform(32, 32, enable_lfu=False)
    with pytest.raises(ValueError, match="enable_lfu"):
        F.set_lfu(st)
    assert st.run_lfu is False
    blk = _quiet(F.FFC_BN_ACT, 32, 32, 3, 0.5, 0.5, 1, 1, enable_lfu=False)
    with pytest.raises(ValueError, match="enable_lfu"):
        F.set_lfu(blk)
    F.set_lfu(st, False)   # switching off is always possible


def test_set_lfu_keeps_state_dict_keys():
    import fastfourierconvolution_amd as F
    g = _quiet(F.FFCGenerator, 100, 3, 64)
    before = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    F.set_lfu(g)
    assert {k: tuple(v.shape) for k, v in g.state_dict().items()} == before
    assert any(".lfu." in k for k in before)


def test_run_lfu_is_part_of_the_layer_spec():
    """flipping the switch gives the cached layer ops another spec (another template and plan);
    switched off, the spec is the one from before the switch existed"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import ops
    blk = _quiet(F.FFC_BN_ACT, 32, 32, 3, 0.5, 0.5, 1, 1)
    off = ops.layer_spec(blk)
    assert "run_lfu" not in off
    on = ops.layer_spec(F.set_lfu(blk))
    assert on != off and "run_lfu" in on
    assert ops.layer_spec(F.set_lfu(blk, False)) == off
    tpl = ops.template(on)
    assert tpl.module.ffc.convg2g.run_lfu is True
    assert ops.template(off).module.ffc.convg2g.run_lfu is False
    assert tpl.param_names == ops.template(off).param_names


def test_split_is_the_quadrant_stack():
    s = torch.arange(2 * 8 * 4 * 6, dtype=torch.float64).reshape(2, 8, 4, 6)
    xs = R.lfu_split(s)
    assert xs.shape == (2, 8, 2, 3)
    for q, (r0, c0) in enumerate(((0, 0), (2, 0), (0, 3), (2, 3))):   # TL, BL, TR, BR
        assert torch.equal(xs[:, 2 * q:2 * q + 2], s[:, :2, r0:r0 + 2, c0:c0 + 3])


@pytest.mark.parametrize("stride,upsample,cin,cout,hw", [(1, False, 32, 32, 8), (2, True, 32, 16, 4),
                                                         (2, False, 16, 32, 16)])
@pytest.mark.parametrize("training", [True, False])
def test_restatement_reduces_to_the_oracle(stride, upsample, cin, cout, hw, training):
    """with the lfu mix weight and lfu.bn.bias zero (and, in eval mode, a zero lfu.bn.running_mean:
    the BatchNorm of an all-zero input is then 0), ys = irfft(relu(0)) = 0, so the restatement must
    give the oracle's spectral_transform (self-check of the tests' own reference)"""
    import fastfourierconvolution_amd as F
    st = F.SpectralTransform(cin, cout, stride, enable_lfu=True, upsample=upsample)
    sd = R.to_double(R.random_state(st, seed=11, running=not training))
    sd["lfu.conv_layer.weight"].zero_()
    sd["lfu.bn.bias"].zero_()
    sd["lfu.bn.running_mean"].zero_()
    x = torch.randn(3, cin, hw, hw, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    a, b = R.to_double(sd), R.to_double(sd)
    got = R.spectral_transform_lfu(x, a, "", stride, upsample, training)
    ref = O.spectral_transform(x, b, "", stride, upsample, training)
    assert O.normwise_err(got, ref) <= 1e-12
    for k in b:
        if ".lfu." not in "." + k:
            assert torch.equal(a[k], b[k]), k


def test_entry_points_validate_arguments_without_gpu():
    import ctypes

    from fastfourierconvolution_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)   # never dereferenced: every call below fails its argument check first
    q = ctypes.c_void_p(32)
    assert lib.ffc_lfu_gather(None, 1, 4, 8, 8, 1, None, None, 0, p, None) == -1
    assert b"ffc_lfu_gather" in lib.ffc_last_error()
    assert lib.ffc_lfu_gather(p, 1, 6, 8, 8, 1, None, None, 0, q, None) == -1      # c % 4 != 0
    assert lib.ffc_lfu_gather(p, 1, 4, 7, 8, 1, None, None, 0, q, None) == -1      # odd H
    assert lib.ffc_lfu_gather(p, 1, 4, 8, 8, 3, None, None, 0, q, None) == -1      # up not in {1, 2}
    assert lib.ffc_lfu_tile_add(p, q, 1, 4, 8, 9, p, None) == -1                   # odd W
    assert lib.ffc_lfu_tile_add(p, p, 1, 4, 8, 8, p, None) == -1                   # ys aliases v
    assert b"alias" in lib.ffc_last_error()
    assert lib.ffc_lfu_gather_bwd(p, 0, 4, 8, 8, q, None) == -1                    # B = 0
    assert lib.ffc_lfu_tile_bwd(p, 1, 4, 8, 8, None, None) == -1                   # null output
    assert lib.ffc_abi_version() == 4   # additions only: the ABI version does not move
