"""float64 references of the conditional batch norm path (TEST INFRASTRUCTURE ONLY): the oracle's blocks
(oracle/ffc_oracle.py, torch FFTs so that autograd runs through them) plus a ten-line conditional norm
(layers/cond/cond_bn.py:16-24), the conditional FFC_BN_ACT (ffc_bn_act.py:70-83 with labels on bn_l /
bn_g only: what the reference's constructors build), the four models of fgan_cond_complete.py, and the
kernel-level inputs / formulas of csrc/cbn_kernels.hip.  Pinned against the reference's own fp64 runs
by tests/test_cbn_cpu.py (fixtures of tests/golden/gen_golden_cbn.py)."""
import torch
import torch.nn.functional as F

import train_refs as tr
from oracle import ffc_oracle as O


def cond_bn(x, sd, prefix, labels, training, momentum=0.1, eps=1e-5):
    """ConditionalBatchNorm2d.forward: gamma[b, c] * BatchNorm2d(affine=False)(x) + beta[b, c], with
    nn.BatchNorm2d's running-statistics update in training mode"""
    C = x.shape[1]
    rm, rv = sd[prefix + "bn.running_mean"], sd[prefix + "bn.running_var"]
    if training:
        n = x.numel() // C
        mean, var = x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)
        with torch.no_grad():
            rm.mul_(1 - momentum).add_(momentum * mean.to(rm.dtype))
            rv.mul_(1 - momentum).add_(momentum * (var * (n / max(n - 1, 1))).to(rv.dtype))
            sd[prefix + "bn.num_batches_tracked"] += 1
    else:
        mean, var = rm.to(x.dtype), rv.to(x.dtype)
    xh = (x - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
    e = sd[prefix + "embed.weight"].to(x.dtype)[labels.reshape(-1)]
    return e[:, :C, None, None] * xh + e[:, C:, None, None]


def ffc_bn_act_cond(x, sd, prefix, cfg, labels, training, noise=None):
    """FFC_BN_ACT.forward(x, y) with ConditionalBatchNorm2d norms, the labels on bn_l / bn_g only;
    noise: optional {"l" | "g": (weight key, noise)} added after the activation (NoiseInjection)"""
    c2 = dict(cfg)
    c2["transpose"] = cfg.get("upsampling", False)
    outs = O.ffc(x, sd, prefix + "ffc.", c2, training, "torch")
    act = cfg.get("activation_layer", "Identity")
    res = []
    for name, o in zip("lg", outs):
        if isinstance(o, torch.Tensor):
            o = O.activation(cond_bn(o, sd, f"{prefix}bn_{name}.", labels, training), act)
            if noise and name in noise:
                o = o + sd[noise[name][0]].to(o.dtype) * noise[name][1]
        res.append(o)
    return tuple(res)


# --------------------------------------------------------------------------- models (fgan_cond_complete.py)
def gen_layers(K, ngf=64, g=0.25):
    T = lambda i, o, ri: dict(in_channels=i, out_channels=o, kernel_size=4, ratio_gin=ri, ratio_gout=g,  # noqa: E731
                              stride=2, padding=1, activation_layer="GELU", upsampling=True, num_classes=K)
    return [("conv2", T(ngf * 8, ngf * 4, 0.0)), ("conv3", T(ngf * 4, ngf * 2, g)), ("conv4", T(ngf * 2, ngf, g))]


HEAD = dict(in_channels=64, out_channels=3, kernel_size=3, ratio_gin=0.25, ratio_gout=0.0, stride=1, padding=1,
            activation_layer="Tanh", norm_layer="Identity", upsampling=False)


def _plain_bn(x, sd, prefix, training):
    return O.batch_norm(x, sd, prefix, training)


def cond_generator(z, labels, sd, K, training, noises=None, stl_mg=None):
    """FCondGenerator (:91-114) / FCondGeneratorSTL (:158-186, stl_mg = its mg) up to the float image"""
    dt = z.dtype
    if stl_mg is None:
        emb = sd["label_embed.weight"].to(dt)[labels].view(labels.shape[0], -1, 1, 1)
        emb = F.conv_transpose2d(emb, sd["label_conv.0.weight"].to(dt), sd["label_conv.0.bias"].to(dt))
        emb = F.gelu(_plain_bn(emb, sd, "label_conv.1.", training))
        x = F.conv_transpose2d(z.reshape(z.shape[0], -1, 1, 1), sd["input_conv.0.weight"].to(dt),
                               sd["input_conv.0.bias"].to(dt))
        x = F.gelu(_plain_bn(x, sd, "input_conv.1.", training))
        x = torch.cat([x, emb], dim=1)
    else:
        x = torch.cat([z, sd["label_embed.weight"].to(dt)[labels]], dim=1)
        x = F.linear(x, sd["noise_to_feature.weight"].to(dt), sd["noise_to_feature.bias"].to(dt))
        x = x.reshape(x.shape[0], -1, stl_mg, stl_mg)
    for i, (name, cfg) in enumerate(gen_layers(K)):
        nz = None
        if training:
            n = name[-1]
            nz = {"l": (f"lcl_noise{n}.weight", noises[i][0]), "g": (f"glb_noise{n}.weight", noises[i][1])}
        x = ffc_bn_act_cond(x, sd, name + ".", cfg, labels, training, nz)
    return O.resizer(O.ffc_bn_act(x, sd, "conv5.", HEAD, training, "torch"))


D_CONVS = ((4, 64, 3, 1), (64, 64, 4, 2), (64, 128, 3, 1), (128, 128, 4, 2), (128, 256, 3, 1), (256, 256, 4, 2),
           (256, 512, 3, 1))


def cond_discriminator(x, labels, sd, training, mg=4):
    """Discriminator.forward (:211-227); sd's spectral-norm vectors are advanced as the module call does"""
    O.sn_materialize(sd, {}, training)
    B = x.shape[0]
    plane = sd["label_embed.weight"].to(x.dtype)[labels].view(B, 1, 8 * mg, 8 * mg)
    m = torch.cat([x, plane], dim=1)
    for i, (_, _, k, s) in enumerate(D_CONVS, 1):
        m = F.leaky_relu(F.conv2d(m, sd[f"conv{i}.weight"].to(x.dtype), sd[f"conv{i}.bias"].to(x.dtype), stride=s,
                                  padding=1), 0.1)
    return F.linear(m.reshape(-1, mg * mg * 512), sd["fc.weight"].to(x.dtype), sd["fc.bias"].to(x.dtype))


def fdisc_layers(K, g=0.25):
    L = lambda i, o, k, ri, ro, s: dict(in_channels=i, out_channels=o, kernel_size=k, ratio_gin=ri,  # noqa: E731
                                        ratio_gout=ro, stride=s, padding=1, bias=True,
                                        activation_layer="LeakyReLU", num_classes=K)
    return [("conv1", L(4, 64, 3, 0.0, g, 1)), ("conv2", L(64, 128, 4, g, g, 2)), ("conv3", L(128, 256, 4, g, g, 2)),
            ("conv4", L(256, 512, 4, g, 0.0, 2))]


def cond_fdiscriminator(x, labels, sd, K, training, mg=4):
    """FDiscriminator.forward (:253-271) without the GaussianNoise (its stddev is set to 0 in the tests)"""
    O.sn_materialize(sd, {}, training)
    B = x.shape[0]
    plane = sd["label_embed.weight"].to(x.dtype)[labels].view(B, 1, 8 * mg, 8 * mg)
    m = torch.cat([x, plane], dim=1)
    for name, cfg in fdisc_layers(K):
        m = ffc_bn_act_cond(m, sd, name + ".", cfg, labels, training)
    m = O.resizer(m)
    return F.linear(m.reshape(-1, mg * mg * 512), sd["fc.weight"].to(x.dtype), sd["fc.bias"].to(x.dtype))


# --------------------------------------------------------------------------- kernel-level references
KERNEL_SHAPES = [(3, 5, 7), (6, 8, 1), (2, 4, 256), (2, 3, 260), (65, 4, 16)]


def kernel_inputs(shape, K, train, seed=0):
    """fixed-seed float32 inputs of one kernel case: x, dy (B, C, HW), labels (B) covering [0, K) cyclically
    from a random start (K > B leaves classes absent), table (K, 2C), noise (B, HW), noise_w (C), running
    statistics.  Kink-free as train_refs.bn_inputs: an element whose float64 pre-activation is within
    KINK of 0 is moved through x to +-2 KINK on its side, and everything is recomputed, until none is left"""
    B, C, HW = shape
    gen = torch.Generator().manual_seed(7000 + 7 * B + 11 * C + HW + 13 * K + (1 if train else 0) + seed)
    x = torch.randn(B, C, HW, generator=gen)
    dy = torch.randn(B, C, HW, generator=gen)
    labels = (torch.arange(B) * 2 + int(torch.randint(0, K, (1,), generator=gen))) % K
    table = torch.cat(((1.0 + 0.5 * torch.rand(K, C, generator=gen)) * (1 - 2 * (torch.arange(C) % 2)),
                       0.3 * torch.randn(K, C, generator=gen)), dim=1)
    noise = torch.randn(B, HW, generator=gen)
    noise_w = 0.2 * torch.randn(C, generator=gen)
    rmean = 0.2 * torch.randn(C, generator=gen)
    rvar = 0.5 + torch.rand(C, generator=gen)
    inp = dict(x=x, dy=dy, labels=labels, table=table, noise=noise, noise_w=noise_w, rmean=rmean, rvar=rvar)
    for _ in range(100):
        z = kernel_pre(inp, train)
        bad = z.abs() < tr.KINK
        if not bad.any():
            return inp
        _, var = tr.bn_stats(inp["x"], train, rmean, rvar)
        slope = table.double()[labels][:, :C, None] * (var + tr.BN_EPS).rsqrt()[None, :, None]
        target = torch.where(z >= 0, 2 * tr.KINK, -2 * tr.KINK)
        inp["x"] = torch.where(bad, inp["x"].double() + (target - z) / slope.expand_as(z), inp["x"].double()).float()
    raise AssertionError("kink-free builder did not converge")


def kernel_xhat(inp, train, x=None):
    x = inp["x"].double() if x is None else x
    if train:
        mean, var = x.mean(dim=(0, 2)), x.var(dim=(0, 2), unbiased=False)
    else:
        mean, var = inp["rmean"].double(), inp["rvar"].double()
    return (x - mean[None, :, None]) * (var + tr.BN_EPS).rsqrt()[None, :, None]


def kernel_pre(inp, train, x=None, table=None):
    """float64 pre-activation z = xhat * gamma[l_b] + beta[l_b]"""
    C = inp["x"].shape[1]
    e = (inp["table"].double() if table is None else table)[inp["labels"]]
    return kernel_xhat(inp, train, x) * e[:, :C, None] + e[:, C:, None]


def kernel_consts(inp, train):
    """float32 scale0 = 1/sigma, shift0 = -mu/sigma as the affine-less finalize gives them"""
    mean, var = tr.bn_stats(inp["x"], train, inp["rmean"], inp["rvar"])
    inv = (var + tr.BN_EPS).rsqrt()
    return inv.float(), (-mean * inv).float()


def kernel_forward(inp, act, train, with_noise):
    y = tr.act64(kernel_pre(inp, train), act)
    if with_noise:
        y = y + inp["noise_w"].double()[None, :, None] * inp["noise"].double()[:, None, :]
    return y


def kernel_autograd(inp, act, train):
    """float64 autograd of act(cond_bn(x)) under dy -> dx, d table"""
    x = inp["x"].double().requires_grad_(True)
    table = inp["table"].double().requires_grad_(True)
    tr.act64(kernel_pre(inp, train, x, table), act).backward(inp["dy"].double())
    return x.grad, table.grad


def kernel_formulas(inp, act, train):
    """the backward of csrc/cbn_kernels.hip written out in float64: per-sample sums (B, 2C) [s2 | s1], the
    row scatter, the coefficients, dx -> sums, d table, dx"""
    B, C, HW = inp["x"].shape
    K = inp["table"].shape[0]
    xh = kernel_xhat(inp, train)
    z = kernel_pre(inp, train).requires_grad_(True)
    tr.act64(z, act).backward(inp["dy"].double())
    g = z.grad
    s1, s2 = g.sum(dim=2), (g * xh).sum(dim=2)
    sums = torch.cat((s2, s1), dim=1)
    dtable = torch.zeros(K, 2 * C, dtype=torch.float64).index_add_(0, inp["labels"], sums)
    gamma = inp["table"].double()[inp["labels"]][:, :C]
    _, var = tr.bn_stats(inp["x"], train, inp["rmean"], inp["rvar"])
    inv = (var + tr.BN_EPS).rsqrt()[None, :, None]
    if train:
        N = B * HW
        m1, m2 = (gamma * s1).sum(dim=0) / N, (gamma * s2).sum(dim=0) / N
        dx = inv * (gamma[:, :, None] * g - m1[None, :, None] - xh * m2[None, :, None])
    else:
        dx = inv * gamma[:, :, None] * g
    return sums, dtable, dx
