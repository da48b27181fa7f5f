"""The SAGAN baseline's host side without a GPU: state_dict keys and shapes against lists written out here (the
reference's, sagan_models.py at image_size = 32), the constructors' refusals, the dim-0 matrix view of a
ConvTranspose2d weight, the ffc_sn_job.flags field, and the exports."""
import ctypes

import pytest
import torch
import torch.nn as nn

import fastfourierconvolution_amd as F
from fastfourierconvolution_amd import _autograd as ag
from fastfourierconvolution_amd import _lib, training


def _bn(pre, c):
    return [(f"{pre}.weight", (c,)), (f"{pre}.bias", (c,)), (f"{pre}.running_mean", (c,)),
            (f"{pre}.running_var", (c,)), (f"{pre}.num_batches_tracked", ())]


def _attn(pre, c):
    return [(f"{pre}.gamma", (1,)), (f"{pre}.query_conv.weight", (c // 8, c, 1, 1)), (f"{pre}.query_conv.bias", (c // 8,)),
            (f"{pre}.key_conv.weight", (c // 8, c, 1, 1)), (f"{pre}.key_conv.bias", (c // 8,)),
            (f"{pre}.value_conv.weight", (c, c, 1, 1)), (f"{pre}.value_conv.bias", (c,))]


G_KEYS = (
    [("l1.0.module.bias", (256,)), ("l1.0.module.weight_u", (128,)), ("l1.0.module.weight_v", (4096,)),
     ("l1.0.module.weight_bar", (128, 256, 4, 4))] + _bn("l1.1", 256) +
    [("l2.0.module.bias", (128,)), ("l2.0.module.weight_u", (256,)), ("l2.0.module.weight_v", (2048,)),
     ("l2.0.module.weight_bar", (256, 128, 4, 4))] + _bn("l2.1", 128) +
    [("l3.0.module.bias", (64,)), ("l3.0.module.weight_u", (128,)), ("l3.0.module.weight_v", (1024,)),
     ("l3.0.module.weight_bar", (128, 64, 4, 4))] + _bn("l3.1", 64) +
    [("last.0.weight", (64, 3, 4, 4)), ("last.0.bias", (3,))] + _attn("attn1", 128) + _attn("attn2", 64))

D_KEYS = (
    [("l1.0.module.bias", (64,)), ("l1.0.module.weight_u", (64,)), ("l1.0.module.weight_v", (48,)),
     ("l1.0.module.weight_bar", (64, 3, 4, 4)),
     ("l2.0.module.bias", (128,)), ("l2.0.module.weight_u", (128,)), ("l2.0.module.weight_v", (1024,)),
     ("l2.0.module.weight_bar", (128, 64, 4, 4)),
     ("l3.0.module.bias", (256,)), ("l3.0.module.weight_u", (256,)), ("l3.0.module.weight_v", (2048,)),
     ("l3.0.module.weight_bar", (256, 128, 4, 4)),
     ("last.0.weight", (1, 256, 4, 4)), ("last.0.bias", (1,))] + _attn("attn1", 256) + _attn("attn2", 512))


def test_state_dict_keys_and_shapes():
    assert len(G_KEYS) == 43 and len(D_KEYS) == 28
    G = F.SAGANGenerator(64, 32, 128, 64)
    D = F.SAGANDiscriminator(64, 32, 64)
    assert [(k, tuple(v.shape)) for k, v in G.state_dict().items()] == G_KEYS
    assert [(k, tuple(v.shape)) for k, v in D.state_dict().items()] == D_KEYS
    assert G.imsize == D.imsize == 32 and isinstance(G.l4, nn.Identity) and isinstance(D.l4, nn.Identity)
    for m in (G, D):
        for k, p in m.named_parameters():
            assert p.requires_grad == (not k.endswith(("weight_u", "weight_v"))), k
        for k, v in m.state_dict().items():
            if k.endswith(("weight_u", "weight_v")):
                assert abs(float(v.norm()) - 1.0) < 1e-5, k
    assert G.need_attention is True and D.need_attention is True


def test_wrapper_registration_follows_the_reference():
    conv = nn.ConvTranspose2d(6, 10, 4, 2, 1)
    w0 = conv.weight.detach().clone()
    sn = F.SAGANSpectralNorm(conv)
    assert list(sn.state_dict()) == ["module.bias", "module.weight_u", "module.weight_v", "module.weight_bar"]
    assert "weight" not in conv._parameters and not hasattr(conv, "weight")
    assert torch.equal(conv.weight_bar, w0) and conv.weight_u.shape == (6,) and conv.weight_v.shape == (160,)
    assert sn.name == "weight" and sn.power_iterations == 1 and sn.module is conv
    u0 = conv.weight_u.detach().clone()
    again = F.SAGANSpectralNorm(conv)              # _made_params: nothing re-registered, nothing redrawn
    assert again._made_params() and torch.equal(conv.weight_u, u0)
    assert ag.sn_view(conv.weight_bar.shape, 0) == (6, 160, 160, 160, 0)      # dim 0 for ConvTranspose2d too
    assert ag.sn_view(conv.weight_bar.shape, 1) == (10, 96, 16, 16, 160)      # what the hook form would take


def test_refusals():
    with pytest.raises(NotImplementedError, match=r"image_size = 64.*Self_Attn\(64\).*128 channels"):
        F.SAGANGenerator(64)                       # the reference's default size
    with pytest.raises(NotImplementedError, match=r"image_size = 64.*Conv2d\(512, 1, 4\).*256 channels"):
        F.SAGANDiscriminator()
    for size in (16, 128):
        with pytest.raises(NotImplementedError, match="image_size"):
            F.SAGANGenerator(8, size, 128, 64)
        with pytest.raises(NotImplementedError, match="image_size"):
            F.SAGANDiscriminator(8, size, 64)
    with pytest.raises(NotImplementedError, match="conv_dim = 32.*hard-coded"):
        F.SAGANGenerator(8, 32, 128, 32)
    with pytest.raises(NotImplementedError, match="conv_dim = 32.*hard-coded"):
        F.SAGANDiscriminator(8, 32, 32)
    with pytest.raises(NotImplementedError, match=r"SAGANSpectralNorm\(Conv2d\).*power_iterations = 2"):
        F.SAGANSpectralNorm(nn.Conv2d(3, 4, 3), power_iterations=2)
    with pytest.raises(NotImplementedError, match=r"SAGANSpectralNorm\(Linear\)"):
        F.SAGANSpectralNorm(nn.Linear(3, 4))
    sn = F.SAGANSpectralNorm(nn.Conv2d(3, 4, 3))
    with pytest.raises(NotImplementedError, match=r"SAGANSpectralNorm\(Conv2d\).*cpu"):
        sn(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match=r"SAGANSpectralNorm\(Conv2d\).*float64"):
        sn.double()(torch.zeros(1, 3, 8, 8, dtype=torch.float64))


def test_wgan_gp_is_refused_before_anything_runs():
    with pytest.raises(NotImplementedError, match="double backward"):
        training.sagan_step(None, None, None, None, None, None, None, adv_loss='wgan-gp')


def test_flags_field_and_exports():
    names = dict(_lib.SnJob._fields_)
    assert "flags" in names and "pad_" not in names
    assert _lib.SnJob.flags.offset == _lib.SnJob.R.offset + 4 and _lib.SnJob.flags.size == 4
    assert _lib.SnJob.stride_m.offset == _lib.SnJob.flags.offset + 4
    out = (ctypes.c_int * 12)()
    assert _lib.load().ffc_struct_sizes(out, 12) == 0 and out[11] == ctypes.sizeof(_lib.SnJob)
    assert ag.SN_EPS_ADD == 1
    for name in ("SAGANSpectralNorm", "SAGANGenerator", "SAGANDiscriminator"):
        assert name in F.__all__ and hasattr(F, name)
    assert callable(training.sagan_step)
