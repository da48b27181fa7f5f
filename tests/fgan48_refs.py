"""The 8*mg family of fgan_complete.py (FGenerator :81-140, Discriminator :142-171, FDiscriminator
:173-214) composed from the oracle's blocks (oracle/ffc_oracle.py) in the state_dict layout of the
reference classes.  Checked against the reference's own fp64 outputs in test_oracle_fgan48.py, so a GPU
test may use these compositions where it has no fixture."""
import torch.nn.functional as F

from oracle.ffc_oracle import (FGAN_D_CONVS, _w, ffc_bn_act, fgan128_layers, noise_injection, resizer,
                               sn_materialize)


def fgan32_layers(ngf=64, g=0.25):
    """fgan_complete.py:97-113: conv2..conv4 (x2) and the conv5 head: the first three trunk layers of
    fgan128_layers at this width and ratio, and its head under the name conv5"""
    ls = fgan128_layers(ngf, g)
    return ls[:3] + [("conv5", ls[-1][1])]


def fgan32_generator(z, sd, training, noises=None, mg=4):
    """FGenerator.forward (:115-134), without the eval-mode uint8 quantization of :136-138"""
    x = F.linear(z, _w(sd, "noise_to_feature.0.weight", z.dtype), _w(sd, "noise_to_feature.0.bias", z.dtype))
    x = x.reshape(x.size(0), -1, mg, mg)
    for i, (name, cfg) in enumerate(fgan32_layers()):
        x = ffc_bn_act(x, sd, name + ".", cfg, training)
        if training and name != "conv5":
            n = int(name[-1])
            x = (noise_injection(x[0], sd, f"lcl_noise{n}.", noises[i][0]),
                 noise_injection(x[1], sd, f"glb_noise{n}.", noises[i][1]))
    return resizer(x)


def fgan32_discriminator(x, sd, training, sn=True, mg=4):
    """Discriminator.forward (:161-171): conv1..conv7 + LeakyReLU(0.1), fc"""
    if sn:
        sn_materialize(sd, {}, training)
    for i, (_, _, k, s) in enumerate(FGAN_D_CONVS[:7], 1):
        x = F.leaky_relu(F.conv2d(x, _w(sd, f"conv{i}.weight", x.dtype), _w(sd, f"conv{i}.bias", x.dtype),
                                  stride=s, padding=1), 0.1)
    return F.linear(x.reshape(-1, mg * mg * 512), _w(sd, "fc.weight", x.dtype), _w(sd, "fc.bias", x.dtype))


def fgan32_fdiscriminator(x, sd, training, sn=True, mg=4):
    """FDiscriminator.forward (:205-214): four local-only FFC_BN_ACT with bias, fc"""
    if sn:
        sn_materialize(sd, {}, training)
    plan = ((3, 64, 3, 1, "Identity"), (64, 128, 4, 2, "BatchNorm2d"), (128, 256, 4, 2, "BatchNorm2d"),
            (256, 512, 4, 2, "BatchNorm2d"))
    for i, (cin, cout, k, s, norm) in enumerate(plan):
        cfg = dict(in_channels=cin, out_channels=cout, kernel_size=k, ratio_gin=0, ratio_gout=0.0, stride=s,
                   padding=1, norm_layer=norm, activation_layer="LeakyReLU")
        x = ffc_bn_act(x, sd, f"main.{i}.", cfg, training)
    x = resizer(x)
    return F.linear(x.reshape(-1, mg * mg * 512), _w(sd, "fc.weight", x.dtype), _w(sd, "fc.bias", x.dtype))
