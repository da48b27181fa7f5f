"""The reference's callers of the FFC block, restated over the drop-in layers.

FFCModel (models/ffcmodel.py:12-110), FFCGenerator (models/ffc_generator.py:14-44),
FFCDiscriminator (models/ffc_discriminator.py:11-58), the fgan128 FGenerator
(fgan128_complete.py:442-522, BASELINE config 4) and the fgan128 spectral-norm Discriminator it is
trained against (fgan128_complete.py:525-562).  The layer stacks are identical; the
only change is that the ``inplanes=`` keyword the reference callers pass (and its base class
rejects, models/ffcmodel.py:17) is accepted and ignored.

The 8*mg family of fgan_complete.py (32x32 at mg = 4; 48x48 STL-10 / flowers / CelebA at mg = 6) is
restated as FGenerator32, Discriminator32 and FDiscriminator32: ``FGenerator`` and ``Discriminator``
name the fgan128 classes here.  Its class-conditional variant, fgan_cond_complete.py (conditional batch
norm on bn_l / bn_g of every FFC_BN_ACT), is FCondGenerator32, FCondGeneratorSTL, CondDiscriminator32
and FCondDiscriminator32.

The reference names three more classes ``Generator``: the plain transposed-conv baselines its drivers switch
to by moving a comment.  They are Generator32 (fgan_complete.py:34-79, the 8*mg family), Generator64
(fgan64_complete.py:34-82, 16*mg planes) and DCGenerator32 (sngan_complete.py:82-113, the DCGAN stack on a 1x1
z).
"""
import os

import torch
import torch.nn as nn

from . import _autograd as ag
from . import _runtime as rt
from ._lib import check, ptr
from . import _plan
from .config import Config
from .ffc import FFC_BN_ACT, ConditionalBatchNorm2d, set_cond_bn
from .layers_misc import GaussianNoise, NoiseInjection, Print, Resizer, debug_print

# FGenerator conv6 -> conv7 hand-off with the BN + GELU + noise pass deferred into the head's operand
# staging (FFC_DEFER_HEAD=0: the separate pass, for A/B runs).  The head is VALU-bound, so the
# deferred GELU uses a branch-free erf: B = 512 head 1.36 -> 2.46 ms, BN/act/noise pass 2.36 -> 0.79 ms,
# step 18.11 -> 17.61 ms (with erff the head took 4.05 ms: profiles/r02/ab1, s4)
DEFER_HEAD_INPUT = os.environ.get("FFC_DEFER_HEAD", "1") != "0"


class FFCModel(nn.Module):
    def __init__(self, debug=False, inplanes=None):
        super().__init__()
        self.lfu = True
        self.use_se = False
        self.debug = debug
        self.print_size = Print(debug=Config.shared().DEBUG)
        self.resizer = Resizer()

    def get_lr(self, optimizer):
        for param_group in optimizer.param_groups:
            return param_group["lr"]

    def restore_checkpoint(self, ckpt_file, optimizer=None, scheduler=None):
        """models/ffcmodel.py:31-64 (state_dict keys are the reference's)."""
        if not ckpt_file:
            raise ValueError("No checkpoint file to be restored.")
        ckpt_dict = torch.load(ckpt_file, map_location="cpu", weights_only=True)
        self.load_state_dict(ckpt_dict["model_state_dict"])
        if optimizer:
            optimizer.load_state_dict(ckpt_dict["optimizer_state_dict"])
        if scheduler:
            scheduler.load_state_dict(ckpt_dict["scheduler_state_dict"])
        return ckpt_dict["global_step"]

    def save_checkpoint(self, directory, global_step, optimizer=None, scheduler=None, name=None):
        """models/ffcmodel.py:66-107: '{basename(dir)}_{step}_steps.pth'."""
        os.makedirs(directory, exist_ok=True)
        ckpt_dict = {
            "model_state_dict": self.state_dict(),
            "optimizer_state_dict": optimizer.state_dict() if optimizer is not None else None,
            "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else None,
            "global_step": global_step,
        }
        if name is None:
            name = "{}_{}_steps.pth".format(os.path.basename(directory), global_step)
        torch.save(ckpt_dict, os.path.join(directory, name))

    def forward(self, x):
        pass


class FFCGenerator(FFCModel):
    def __init__(self, nz: int, nc: int, ngf: int, g_factor: float = 0.5, debug: bool = False):
        super().__init__(inplanes=ngf * 8, debug=debug)
        self.ffc0 = FFC_BN_ACT(nz, ngf * 8, 4, 0, g_factor, 1, 0, activation_layer=nn.LeakyReLU, upsampling=True)
        self.ffc1 = FFC_BN_ACT(ngf * 8, ngf * 4, 4, g_factor, g_factor, 2, 1, activation_layer=nn.LeakyReLU,
                               upsampling=True)
        self.ffc2 = FFC_BN_ACT(ngf * 4, ngf * 2, 4, g_factor, g_factor, 2, 1, activation_layer=nn.LeakyReLU,
                               upsampling=True)
        self.ffc3 = FFC_BN_ACT(ngf * 2, ngf * 1, 4, g_factor, g_factor, 2, 1, activation_layer=nn.LeakyReLU,
                               upsampling=True)
        self.ffc4 = FFC_BN_ACT(ngf * 1, nc, 4, g_factor, 0, 2, 1, norm_layer=nn.Identity, activation_layer=nn.Tanh,
                               upsampling=True)

    def forward(self, x):
        debug_print("G --")
        x = self.ffc0(x)
        x = self.print_size(x)
        x = self.ffc1(x)
        x = self.print_size(x)
        x = self.ffc2(x)
        x = self.print_size(x)
        x = self.ffc3(x)
        x = self.print_size(x)
        x = self.ffc4(x)
        x = self.resizer(x)
        debug_print("End G --")
        return x


class FFCDiscriminator(FFCModel):
    def __init__(self, nc: int, ndf: int, debug: bool = False):
        super().__init__(inplanes=ndf, debug=debug)
        self.ffc0 = FFC_BN_ACT(nc, ndf * 2, 4, 0, 0.5, 2, 1, activation_layer=nn.LeakyReLU)
        self.ffc1 = FFC_BN_ACT(ndf * 2, ndf * 4, 4, 0.5, 0.5, 2, 1, activation_layer=nn.LeakyReLU)
        self.ffc2 = FFC_BN_ACT(ndf * 4, ndf * 8, 4, 0.5, 0.5, 2, 1, activation_layer=nn.LeakyReLU)
        self.ffc3 = FFC_BN_ACT(ndf * 8, ndf * 16, 4, 0.5, 0.5, 2, 1, activation_layer=nn.LeakyReLU)
        self.ffc4 = FFC_BN_ACT(ndf * 16, 1, 4, 0.5, 0, 1, 0, norm_layer=nn.Identity, activation_layer=nn.Sigmoid)

    def forward(self, x):
        debug_print("D --")
        x = self.print_size(x)
        x = self.ffc0(x)
        x = self.print_size(x)
        x = self.ffc1(x)
        x = self.print_size(x)
        x = self.ffc2(x)
        x = self.print_size(x)
        x = self.ffc3(x)
        x = self.ffc4(x)
        x = self.resizer(x)
        x = self.print_size(x)
        debug_print("End D --")
        return x


class FGenerator(FFCModel):
    """fgan128_complete.py:442-522: Linear(z, 16*1024) -> (1024, 4, 4) -> five x2 FFC_BN_ACT
    (FFCTranspose, BatchNorm2d + GELU, train-mode NoiseInjection on both branches) -> 3x3 FFC_BN_ACT
    head (Tanh) -> Resizer; eval mode returns the uint8 image of :516-521.

    ``forward(z, noises=None)``: ``noises`` optionally supplies the train-mode noise as
    [(lcl, glb)] * 5 ((B, 1, H, W) each) instead of drawing it (the reference draws it inside
    NoiseInjection with normal_()); the reference's forward(z) is the noises=None call."""

    UPS = (2, 3, 4, 5, 6)   # conv{n}: the x2 FFC_BN_ACT + NoiseInjection layers of the trunk
    HEAD = 7                # conv{HEAD}: the 3x3 Tanh head
    USES_SN = True          # the uses_sn flag the reference passes to its FFC_BN_ACTs (stored, unused)

    def __init__(self, z_size, mg: int = 4):
        super().__init__()
        self.z_size = z_size
        self.ngf = 128
        ratio_g = 0.5
        self.mg = mg
        ngf = self.ngf
        self.noise_to_feature = nn.Sequential(nn.Linear(z_size, (self.mg * self.mg) * self.ngf * 8))
        self._build_trunk(ngf, ratio_g)

    def _build_trunk(self, ngf, ratio_g, **norm):
        """conv2..conv6 (x2 FFC_BN_ACT + NoiseInjection pairs) and the conv7 head at width ngf and global
        ratio ratio_g (fgan128_complete.py:457-488; fgan128_cond_complete.py:43-70 at ngf = 64, 0.25);
        conv2..conv4 and the conv5 head for the 8*mg family (UPS / HEAD; fgan_complete.py:97-113)"""
        T = dict(activation_layer=nn.GELU, norm_layer=nn.BatchNorm2d, upsampling=True, uses_noise=True,
                 uses_sn=self.USES_SN)
        T.update(norm)   # the conditional 8*mg generators: norm_layer=ConditionalBatchNorm2d, num_classes=K
        plan = ((2, ngf * 8, ngf * 4, 0.0), (3, ngf * 4, ngf * 2, ratio_g), (4, ngf * 2, ngf, ratio_g),
                (5, ngf, ngf, ratio_g), (6, ngf, ngf, ratio_g))[:len(self.UPS)]
        for n, cin, cout, rin in plan:
            setattr(self, f"conv{n}", FFC_BN_ACT(cin, cout, 4, rin, ratio_g, stride=2, padding=1, **T))
            setattr(self, f"lcl_noise{n}", NoiseInjection(int(cout * (1 - ratio_g))))
            setattr(self, f"glb_noise{n}", NoiseInjection(int(cout * ratio_g)))
        setattr(self, f"conv{self.HEAD}",
                FFC_BN_ACT(ngf, 3, 3, ratio_g, 0.0, stride=1, padding=1, activation_layer=nn.Tanh,
                           norm_layer=nn.Identity, upsampling=False, uses_noise=True, uses_sn=self.USES_SN))

    def _noise_to_feature(self, z):
        """nn.Linear(z_size, 16*1024) (fgan128_complete.py:453-455) on the HIP dense GEMM"""
        lin = self.noise_to_feature[0]
        z = rt.require(z, "z")
        if z.dim() != 2 or z.shape[1] != lin.in_features:
            raise RuntimeError(f"FGenerator: z must be (B, {lin.in_features}), got {tuple(z.shape)}")
        B = z.shape[0]
        if ag.wants_grad(self.noise_to_feature, z):   # training path: Linear as a 1x1 conv job with autograd
            return ag.linear(lin, z).view(B, -1, self.mg, self.mg)
        return torch.ops.ffc.linear(z, lin.weight, lin.bias).view(B, -1, self.mg, self.mg)

    def _trunk(self, fake, noises=None):
        """conv2..conv7 + Resizer on the (B, C, 4, 4) stem output (:496-515); shared with FCondGenerator"""
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        for i, n in enumerate(self.UPS):                                     # :496-515
            conv = getattr(self, f"conv{n}")
            # conv6 -> conv7: conv6's BN + GELU (+ noise) is applied by the 3x3 head as it stages its
            # input (ffc_conv3x3_smallm_tf), no separate pass over the 128x128 activations
            defer = n == self.UPS[-1] and not grad and DEFER_HEAD_INPUT
            if self.training:   # NoiseInjection fused into conv{n}'s BN + GELU pass
                nl, ng = noises[i] if noises is not None else (None, None)
                nzl, nzg = (getattr(self, f"lcl_noise{n}"), nl), (getattr(self, f"glb_noise{n}"), ng)
                fake = conv.forward_deferred(fake, nzl, nzg) if defer else conv.forward_noise(fake, nzl, nzg)
            else:
                fake = conv.forward_deferred(fake) if defer else conv(fake)
        return self.resizer(getattr(self, f"conv{self.HEAD}")(fake))

    def forward_float(self, z, noises=None):
        """FGenerator.forward up to the float image (:491-515): the eval-mode uint8 quantization of
        :516-521 is left out"""
        return self._trunk(self._noise_to_feature(z), noises)                # :491-494

    def forward(self, z, noises=None):
        fake = self.forward_float(z, noises)
        if self.training:
            return fake
        return torch.ops.ffc.quantize_u8(fake)   # :516-521


class Discriminator(FFCModel):
    """fgan128_complete.py:525-562: the plain-CNN critic FGenerator is trained against (:616, :680-703).
    conv1..conv9 (3x3 s1 / 4x4 s2 Conv2d with bias, spectral norm when ``sn``), LeakyReLU(0.1) after
    each, fc = Linear(mg*mg*512, 1) on the flattened 4x4x512 map, no output activation (the reference
    builds ``last_act`` = Sigmoid and leaves it unused, :545-546, :558).  Module names and the
    state_dict are the reference's.

    Every conv is one implicit-GEMM launch of libffc_amd.so with bias + LeakyReLU in its epilogue
    (the ffc::conv_layer op: data / weight / bias gradients on the HIP kernels too); the spectral-norm
    pre-hook runs before each launch as the reference's module call runs it (one power iteration per
    forward in train mode).  Input: (B, 3, 32*mg, 32*mg) fp32 on the GPU."""

    CONVS = ((3, 64, 3, 1), (64, 64, 4, 2), (64, 128, 3, 1), (128, 128, 4, 2), (128, 256, 3, 1),
             (256, 256, 4, 2), (256, 512, 3, 1), (512, 512, 4, 2), (512, 512, 4, 2))
    SIDE = 32   # input side per unit of mg (the stride-2 convs of CONVS take it down to mg)

    def __init__(self, sn: bool = True, mg: int = 4):
        super().__init__()
        self.mg = mg
        sn_fn = torch.nn.utils.spectral_norm if sn else (lambda m: m)
        for i, (cin, cout, k, s) in enumerate(self.CONVS, 1):
            setattr(self, f"conv{i}", sn_fn(nn.Conv2d(cin, cout, k, stride=s, padding=(1, 1))))
        self.fc = sn_fn(nn.Linear(self.mg * self.mg * 512, 1))
        self.act = nn.LeakyReLU(0.1)
        self.last_act = nn.Sigmoid()

    def forward(self, x):
        x = rt.require(x, "x")
        side = self.SIDE * self.mg
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, side, side):
            raise RuntimeError(f"{type(self).__name__}: x must be (B, 3, {side}, {side}), got {tuple(x.shape)}")
        act, param = rt.act_code(self.act)
        m = x
        with rt.sn_batch(self._sn_layers()):   # set_sn_hip: conv1..convN and fc in one table
            for i in range(1, len(self.CONVS) + 1):
                conv = getattr(self, f"conv{i}")
                B, C, H, W = m.shape
                sg = _plan.Seg("conv", C, H, W, conv.kernel_size[0], conv.stride[0], conv.padding[0])
                (m,) = ag.conv_layer(B, [(conv.out_channels, act, param)], [(0, 0, sg, conv)], [m])
            return ag.linear(self.fc, m.reshape(m.shape[0], -1))   # :556

    def _sn_layers(self):
        return [getattr(self, f"conv{i}") for i in range(1, len(self.CONVS) + 1)] + [self.fc]


FGanDiscriminator = Discriminator


class FGenerator32(FGenerator):
    """fgan_complete.py:81-140, the generator of the 8*mg family (CIFAR-10 at mg = 4, the 48x48 STL-10 /
    flowers / CelebA models at mg = 6): Linear(z, mg*mg*512) -> (512, mg, mg) -> three x2 FFC_BN_ACT
    (FFCTranspose, BatchNorm2d + GELU, train-mode NoiseInjection on both branches) at ngf = 64, global
    ratio 0.25 -> 3x3 FFC_BN_ACT head conv5 (Tanh) -> Resizer; eval mode returns the uint8 image of
    :136-138 (its clamp to [-1, 1] is the identity on a Tanh output).  FGenerator's trunk with three
    layers; constructor, attribute names and state_dict keys are the reference FGenerator's.

    ``forward(z, noises=None)``: ``noises`` as FGenerator, [(lcl, glb)] * 3."""

    UPS = (2, 3, 4)
    HEAD = 5
    USES_SN = False

    def __init__(self, z_size, mg: int = 4):
        FFCModel.__init__(self)
        self.z_size = z_size
        self.ngf = 64
        ratio_g = 0.25
        self.mg = mg
        self.noise_to_feature = nn.Sequential(nn.Linear(z_size, (self.mg * self.mg) * self.ngf * 8))
        self._build_trunk(self.ngf, ratio_g)


class Discriminator32(Discriminator):
    """fgan_complete.py:142-171: the plain spectral-norm critic of the 8*mg family, conv1..conv7 of
    Discriminator (three stride-2 convs: 8*mg -> mg) and fc = Linear(mg*mg*512, 1); no ``last_act``.
    Input: (B, 3, 8*mg, 8*mg) fp32 on the GPU."""

    CONVS = Discriminator.CONVS[:7]
    SIDE = 8

    def __init__(self, sn: bool = True, mg: int = 4):
        super().__init__(sn=sn, mg=mg)
        del self.last_act


def _run_stack(seq, x):
    """a Sequential of ConvTranspose2d / BatchNorm2d + ReLU / Tanh (the baseline generators' ``model`` and
    ``last``) on the HIP ops: every ConvTranspose2d one ffc::conv_layer job with its bias (a following Tanh in
    its epilogue), every BatchNorm2d + ReLU pair one ffc::bn_act (+ the running-statistics update in train
    mode)"""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        if isinstance(m, nn.ConvTranspose2d):
            act = (0, 0.0)
            if isinstance(nxt, nn.Tanh):
                act = rt.act_code(nxt)
                i += 1
            (x,) = ag.conv_layer(x.shape[0], [(m.out_channels,) + tuple(act)], [(0, 0, rt.conv_seg(m, x), m)], [x])
        elif isinstance(m, nn.BatchNorm2d) and isinstance(nxt, nn.ReLU):
            x = ag.bn_act(m, x, rt.act_code(nxt))
            i += 1
        else:
            raise NotImplementedError(f"{type(m).__name__} in a baseline generator stack")
        i += 1
    return x


def _ct_bn_relu(chans):
    """ConvTranspose2d(k4, s2, p1) + BatchNorm2d + ReLU per consecutive channel pair"""
    mods = []
    for cin, cout in zip(chans, chans[1:]):
        mods += [nn.ConvTranspose2d(cin, cout, 4, stride=2, padding=(1, 1)), nn.BatchNorm2d(cout), nn.ReLU()]
    return mods


class Generator32(FFCModel):
    """fgan_complete.py:34-79 (``Generator`` there): the plain transposed-conv baseline the FFC generator of the
    8*mg family (FGenerator32) is compared against.  noise_to_feature = Linear(z, mg*mg*512) -> (512, mg, mg) ->
    ``model``: three ConvTranspose2d(k4, s2, p1) with bias, each + BatchNorm2d + ReLU, 512 -> 256 -> 128 -> 64 ->
    ``attn`` = Self_Attn(64, 'relu') on the 8mg x 8mg plane -> ``last``: ConvTranspose2d(64, 3, 3, s1, p1) +
    Tanh.  Constructor, attribute names and state_dict keys are the reference's.

    Everything runs on the HIP ops (no torch compute): the Linear on ffc::linear / ag.linear, each transposed
    conv as one ffc::conv_layer job, BatchNorm2d + ReLU on ffc::bn_act (running statistics,
    num_batches_tracked and momentum as nn.BatchNorm2d; under distributed.enable_sync_bn the batch moments are
    all-reduced like every other BatchNorm of the package), the head on the direct small-M kernel
    (conv_route 'convT3') with Tanh in its epilogue.

    The reference computes the (B, N, N) attention matrix and drops it (``fake, out = self.attn(fake)``);
    here ``self.attn.need_attention`` is set False in the constructor, so the matrix is never allocated (the
    class default of Self_Attn stays True).

    Eval mode returns the uint8 image of :72-77: the clamp to the batch's own min / max is the identity, so it
    is ffc::quantize_u8 of the float image.  ``forward_float(z)`` stops at the float image."""

    TRUNK = (512, 256, 128, 64)

    def __init__(self, z_size, mg: int = 4):
        super().__init__()
        self.z_size = z_size
        self.mg = mg
        self.ngf = 64
        self.noise_to_feature = nn.Linear(z_size, (self.mg * self.mg) * self.ngf * 8)
        self.model = nn.Sequential(*_ct_bn_relu(self.TRUNK))
        from .attention_layer import Self_Attn
        self.attn = Self_Attn(64, "relu")
        self.attn.need_attention = False
        self.last = nn.Sequential(nn.ConvTranspose2d(64, 3, 3, stride=1, padding=(1, 1)), nn.Tanh())

    def forward_float(self, z):
        lin = self.noise_to_feature
        z = rt.require(z, "z")
        if z.dim() != 2 or z.shape[1] != lin.in_features:
            raise RuntimeError(f"{type(self).__name__}: z must be (B, {lin.in_features}), got {tuple(z.shape)}")
        if ag.wants_grad(lin, z):
            fake = ag.linear(lin, z)
        else:
            fake = torch.ops.ffc.linear(z, lin.weight, lin.bias)
        fake = _run_stack(self.model, fake.reshape(z.shape[0], -1, self.mg, self.mg))
        fake, _ = self.attn(fake)
        return _run_stack(self.last, fake)

    def forward(self, z):
        fake = self.forward_float(z)
        if self.training:
            return fake
        return torch.ops.ffc.quantize_u8(fake)


class Generator64(Generator32):
    """fgan64_complete.py:34-82 (``Generator`` there): Generator32 with a fourth ConvTranspose2d(64, 64, k4, s2,
    p1) + BatchNorm2d + ReLU, so the attention and the head run on the 16mg x 16mg plane (64 x 64 at mg = 4)."""

    TRUNK = (512, 256, 128, 64, 64)


class DCGenerator32(nn.Module):
    """sngan_complete.py:82-113 (``Generator`` there): the DCGAN baseline.  One ``model`` Sequential:
    ConvTranspose2d(z, 512, 4, s1) on the 1x1 z, three ConvTranspose2d(k4, s2, p1), each of the four +
    BatchNorm2d + ReLU, then ConvTranspose2d(64, 3, 3, s1, p1) + Tanh: a 32 x 32 image.  No Linear, no attention;
    ``mg`` is accepted and unused, as in the reference.  The layers run as Generator32's do.  Eval mode returns
    uint8(255 * (clamp(x, -1, 1) * 0.5 + 0.5)) (:109-111): on a Tanh output that clamp is the identity, so it is
    ffc::quantize_u8 too."""

    def __init__(self, z_size, mg):
        super().__init__()
        self.z_size = z_size
        self.print_layer = Print(debug=True)
        self.model = nn.Sequential(nn.ConvTranspose2d(z_size, 512, 4, stride=1), nn.BatchNorm2d(512), nn.ReLU(),
                                   *_ct_bn_relu((512, 256, 128, 64)),
                                   nn.ConvTranspose2d(64, 3, 3, stride=1, padding=(1, 1)), nn.Tanh())

    def forward_float(self, z):
        z = rt.require(z, "z")
        if z.numel() % self.z_size:
            raise RuntimeError(f"DCGenerator32: z must hold (B, {self.z_size}) values, got {tuple(z.shape)}")
        return _run_stack(self.model, z.reshape(-1, self.z_size, 1, 1))

    def forward(self, z):
        fake = self.forward_float(z)
        if self.training:
            return fake
        return torch.ops.ffc.quantize_u8(fake)


class FDiscriminator32(FFCModel):
    """fgan_complete.py:173-214: the FFC critic of the 8*mg family.  ``main`` is four FFC_BN_ACT with
    bias, global ratio 0 (local branch only: a 3x3 s1 conv and three 4x4 s2 convs, one implicit-GEMM
    launch each), LeakyReLU(0.1), BatchNorm2d on the last three; fc = Linear(mg*mg*512, 1) under spectral
    norm when ``sn``.  ``gaus_noise`` is built and, as in the reference (:206), not used by forward.
    Input: (B, 3, 8*mg, 8*mg) fp32 on the GPU."""

    def __init__(self, sn: bool = True, mg: int = 4):
        super().__init__()
        self.mg = mg
        sn_fn = torch.nn.utils.spectral_norm if sn else (lambda m: m)
        L = dict(ratio_gin=0, ratio_gout=0.0, padding=1, bias=True, uses_noise=False, uses_sn=True,
                 activation_layer=nn.LeakyReLU)
        self.main = nn.Sequential(
            FFC_BN_ACT(in_channels=3, out_channels=64, kernel_size=3, stride=1, norm_layer=nn.Identity, **L),
            FFC_BN_ACT(in_channels=64, out_channels=128, kernel_size=4, stride=2, norm_layer=nn.BatchNorm2d, **L),
            FFC_BN_ACT(in_channels=128, out_channels=256, kernel_size=4, stride=2, norm_layer=nn.BatchNorm2d, **L),
            FFC_BN_ACT(in_channels=256, out_channels=512, kernel_size=4, stride=2, norm_layer=nn.BatchNorm2d, **L))
        self.fc = sn_fn(nn.Linear(self.mg * self.mg * 512, 1))
        self.gaus_noise = GaussianNoise(0.05)

    def forward(self, x):
        x = rt.require(x, "x")
        side = 8 * self.mg
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, side, side):
            raise RuntimeError(f"FDiscriminator32: x must be (B, 3, {side}, {side}), got {tuple(x.shape)}")
        self.print_size(x)
        m = self.resizer(self.main(x))                                           # :208-209
        return ag.linear(self.fc, m.reshape(-1, self.mg * self.mg * 512))        # :214


class FCondGenerator(FGenerator):
    """fgan128_cond_complete.py:33-133: the class-conditional fgan128 generator.  The stem is two
    ConvTranspose2d(k4, s1, p0) + BatchNorm2d + GELU branches on 1x1 inputs -- z, and the
    label_embed row of each sample's class -- concatenated on channels (:91-101), one fused launch
    sequence (ffc::cond_stem); conv2..conv7 are FGenerator's trunk at ngf = 64, global ratio 0.25.
    Constructor, attribute names and state_dict keys are the reference's.

    ``forward(z, labels, noises=None)``: labels (B,) int64 on the GPU, read by the kernels (a captured
    forward replays with new labels written into the same tensor); ``noises`` as FGenerator.  A label
    outside [0, num_classes) reads no memory outside the table: that sample's stem values are NaN."""

    def __init__(self, z_size, mg: int = 4, num_classes: int = 10):
        FFCModel.__init__(self)
        self.z_size = z_size
        self.ngf = 64
        ratio_g = 0.25
        self.mg = mg
        self.num_classes = num_classes
        self._build_trunk(self.ngf, ratio_g)
        self.label_conv = nn.Sequential(nn.ConvTranspose2d(num_classes, self.ngf * 4, 4, 1, 0),
                                        nn.BatchNorm2d(self.ngf * 4), nn.GELU())
        self.input_conv = nn.Sequential(nn.ConvTranspose2d(z_size, self.ngf * 4, 4, 1, 0),
                                        nn.BatchNorm2d(self.ngf * 4), nn.GELU())
        self.label_embed = nn.Embedding(num_classes, num_classes)

    def _stem(self, z, labels):
        z = rt.require(z, "z")
        if z.dim() == 4 and tuple(z.shape[2:]) == (1, 1):
            z = z.reshape(z.shape[0], -1)                                     # :97
        if z.dim() != 2 or z.shape[1] != self.z_size:
            raise RuntimeError(f"FCondGenerator: z must be (B, {self.z_size}), got {tuple(z.shape)}")
        return ag.cond_stem(self, z, labels)

    def forward_float(self, z, labels, noises=None):
        """forward up to the float image (:91-125), without the eval-mode uint8 quantization of :127-132"""
        return self._trunk(self._stem(z, labels), noises)

    def forward(self, z, labels, noises=None):
        fake = self.forward_float(z, labels, noises)
        if self.training:
            return fake
        return torch.ops.ffc.quantize_u8(fake)   # :127-132


class _ConvSlice:
    """input channels [c0, c1) of a Conv2d seen by conv_layer as a conv of its own: the weight is a view
    of the (spectral-normalised) weight, so its gradient flows back to the parameter; ``bias`` rides on
    one slice only.  The slice is made contiguous here (a differentiable copy of a few KB): the conv
    plans key their packed weights by the tensor object they are handed, and a strided view would be
    copied anew, unregistered, inside the op -- a later copy at a recycled address could then meet a
    stale pack"""

    def __init__(self, weight, c0, c1, bias):
        self.weight = weight[:, c0:c1].contiguous()
        self.bias = bias
        self.out_channels = weight.shape[0]


class FCondDiscriminator(Discriminator):
    """fgan128_cond_complete.py:136-180 (``Discriminator`` there): the label-conditioned critic.
    label_embed (num_classes, 128*128) gives every class a 128x128 plane that conv1 reads as a fourth
    input channel (:159-169).  The plane is gathered by ffc::embed_rows and conv1 runs as a two-segment
    conv job -- image (3 channels) + plane (1 channel), each with its slice of conv1's weight -- so the
    (B, 4, 128, 128) concatenation is never built.  state_dict keys: conv1..conv9, fc, label_embed."""

    CONVS = ((4, 64, 3, 1),) + Discriminator.CONVS[1:]

    def __init__(self, sn: bool = True, mg: int = 4, num_classes: int = 10):
        super().__init__(sn=sn, mg=mg)
        self.num_classes = num_classes
        self.label_embed = nn.Embedding(num_classes, 128 * 128)

    def forward(self, x, labels):
        x = rt.require(x, "x")
        side = 32 * self.mg
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, side, side) or side != 128:
            raise RuntimeError(f"FCondDiscriminator: x must be (B, 3, 128, 128) with mg = 4, got {tuple(x.shape)}")
        return _label_plane_critic(self, x, labels, side)


def _label_plane_critic(self, x, labels, side):
    """the label-conditioned plain critic on a (B, 3, side, side) image: label_embed's row of each sample's
    class as a fourth input plane of conv1, then conv2.. and fc (fgan128_cond_complete.py:159-178,
    fgan_cond_complete.py:211-227)"""
    with rt.sn_batch(self._sn_layers()):   # set_sn_hip: conv1..convN and fc in one table
        return _label_plane_critic_body(self, x, labels, side)


def _label_plane_critic_body(self, x, labels, side):
    B = x.shape[0]
    act, param = rt.act_code(self.act)
    plane = torch.ops.ffc.embed_rows(self.label_embed.weight, labels).view(B, 1, side, side)
    conv = self.conv1
    rt.sn_refresh_train(conv)   # the slices below must see this call's W / sigma
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    (m,) = ag.conv_layer(B, [(conv.out_channels, act, param)],
                         [(0, 0, _plan.Seg("conv", 3, side, side, k, s, p), _ConvSlice(conv.weight, 0, 3, conv.bias)),
                          (0, 1, _plan.Seg("conv", 1, side, side, k, s, p), _ConvSlice(conv.weight, 3, 4, None))],
                         [x, plane])
    for i in range(2, len(self.CONVS) + 1):
        conv = getattr(self, f"conv{i}")
        B, C, H, W = m.shape
        sg = _plan.Seg("conv", C, H, W, conv.kernel_size[0], conv.stride[0], conv.padding[0])
        (m,) = ag.conv_layer(B, [(conv.out_channels, act, param)], [(0, 0, sg, conv)], [m])
    return ag.linear(self.fc, m.reshape(m.shape[0], -1))


# --------------------------------------------------------------------------- conditional 8*mg family
class FCondGenerator32(FCondGenerator):
    """fgan_cond_complete.py:33-114 (``FCondGenerator`` there): FCondGenerator's (B, 512, 4, 4) label / noise
    stem (ffc::cond_stem), then conv2..conv4 -- x2 FFC_BN_ACT with ConditionalBatchNorm2d on bn_l / bn_g,
    GELU and train-mode NoiseInjection -- and the 3x3 Tanh head conv5: a 32x32 image whatever ``mg`` (the
    stem is 4x4; ``mg`` is stored as the reference stores it).  Built with ``cond_bn_only`` on
    (set_cond_bn): the labels condition bn_l / bn_g only, which is what the reference's constructors
    build; its forward as written raises TypeError in conv3.  Attribute names and state_dict keys are the
    reference's.  ``forward(z, labels, noises=None)`` as FCondGenerator, noises [(lcl, glb)] * 3."""

    UPS = (2, 3, 4)
    HEAD = 5

    def __init__(self, z_size, mg: int = 4, num_classes: int = 10):
        FFCModel.__init__(self)
        self.z_size = z_size
        self.ngf = 64
        self.mg = mg
        self.num_classes = num_classes
        self._build_trunk(self.ngf, 0.25, norm_layer=ConditionalBatchNorm2d, num_classes=num_classes)
        self._build_stem(z_size, num_classes)
        set_cond_bn(self)

    def _build_stem(self, z_size, num_classes):
        self.label_conv = nn.Sequential(nn.ConvTranspose2d(num_classes, self.ngf * 4, 4, 1, 0),
                                        nn.BatchNorm2d(self.ngf * 4), nn.GELU())
        self.input_conv = nn.Sequential(nn.ConvTranspose2d(z_size, self.ngf * 4, 4, 1, 0),
                                        nn.BatchNorm2d(self.ngf * 4), nn.GELU())
        self.label_embed = nn.Embedding(num_classes, num_classes)

    def _trunk_cond(self, fake, labels, noises=None):
        """conv2..conv4 with the labels + the conv5 head + Resizer (:104-114)"""
        for i, n in enumerate(self.UPS):
            conv = getattr(self, f"conv{n}")
            if self.training:   # NoiseInjection fused into the conditional norm + GELU pass
                nl, ng = noises[i] if noises is not None else (None, None)
                fake = conv.forward_noise(fake, (getattr(self, f"lcl_noise{n}"), nl),
                                          (getattr(self, f"glb_noise{n}"), ng), labels)
            else:
                fake = conv(fake, labels)
        return self.resizer(getattr(self, f"conv{self.HEAD}")(fake))

    def forward_float(self, z, labels, noises=None):
        return self._trunk_cond(self._stem(z, labels), labels, noises)


class FCondGeneratorSTL(FCondGenerator32):
    """fgan_cond_complete.py:117-186: the conditional generator of the 8*mg planes (48x48 at mg = 6).
    noise_to_feature = Linear(z_size + num_classes, mg*mg*512) on cat([z, label_embed[labels]]) -- the
    row gather on ffc::embed_rows, the Linear as one two-segment GEMM job over its weight's two column
    blocks (the concatenation is never built) -- viewed (512, mg, mg); then FCondGenerator32's trunk."""

    def _build_stem(self, z_size, num_classes):
        self.label_embed = nn.Embedding(num_classes, num_classes)
        self.noise_to_feature = nn.Linear(z_size + num_classes, (self.mg * self.mg) * self.ngf * 8)

    def _stem(self, z, labels):
        z = rt.require(z, "z")
        if z.dim() != 2 or z.shape[1] != self.z_size:
            raise RuntimeError(f"FCondGeneratorSTL: z must be (B, {self.z_size}), got {tuple(z.shape)}")
        B, K = z.shape[0], self.num_classes
        emb = torch.ops.ffc.embed_rows(self.label_embed.weight, labels)                     # :160
        lin = self.noise_to_feature
        N = lin.out_features
        w = lin.weight.view(N, self.z_size + K, 1, 1)
        (f,) = ag.conv_layer(B, [(N, 0, 0.0)],
                             [(0, 0, _plan.Seg("pw", self.z_size, 1, 1), _ConvSlice(w, 0, self.z_size, lin.bias)),
                              (0, 1, _plan.Seg("pw", K, 1, 1), _ConvSlice(w, self.z_size, self.z_size + K, None))],
                             [z.reshape(B, self.z_size, 1, 1), emb.reshape(B, K, 1, 1)])   # :164-165
        return f.reshape(B, -1, self.mg, self.mg)                                           # :168


class CondDiscriminator32(Discriminator32):
    """fgan_cond_complete.py:189-227 (``Discriminator`` there): Discriminator32 whose conv1 reads a fourth
    input plane, label_embed's (num_classes, 8mg*8mg) row of each sample's class (as FCondDiscriminator).
    Input: (B, 3, 8*mg, 8*mg) fp32 and (B,) int64 labels on the GPU."""

    CONVS = ((4, 64, 3, 1),) + Discriminator32.CONVS[1:]

    def __init__(self, sn: bool = True, mg: int = 4, num_classes: int = 10):
        super().__init__(sn=sn, mg=mg)
        self.num_classes = num_classes
        self.label_embed = nn.Embedding(num_classes, 8 * 8 * self.mg * self.mg)

    def forward(self, x, labels):
        x = rt.require(x, "x")
        side = self.SIDE * self.mg
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, side, side):
            raise RuntimeError(f"CondDiscriminator32: x must be (B, 3, {side}, {side}), got {tuple(x.shape)}")
        return _label_plane_critic(self, x, labels, side)


class FCondDiscriminator32(FFCModel):
    """fgan_cond_complete.py:229-274 (``FDiscriminator`` there): the conditional FFC critic.  conv1..conv4
    are FFC_BN_ACT with bias, global ratio 0.25 (conv4: local output only), LeakyReLU(0.1) and
    ConditionalBatchNorm2d on bn_l / bn_g; the image passes GaussianNoise(0.05) (train mode) and is
    joined by the label plane of label_embed (num_classes, 8mg*8mg) as a fourth channel; fc =
    Linear(mg*mg*512, 1) under spectral norm when ``sn``.  Built with ``cond_bn_only`` on: conv2 and
    conv3 have a SpectralTransform, where the reference's forward as written raises TypeError.
    Input: (B, 3, 8*mg, 8*mg) fp32 and (B,) int64 labels on the GPU."""

    def __init__(self, sn: bool = True, mg: int = 4, num_classes: int = 10):
        super().__init__()
        self.mg = mg
        self.num_classes = num_classes
        sn_fn = torch.nn.utils.spectral_norm if sn else (lambda m: m)
        r = 0.25
        L = dict(padding=1, bias=True, uses_noise=False, uses_sn=True, activation_layer=nn.LeakyReLU,
                 norm_layer=ConditionalBatchNorm2d, num_classes=num_classes)
        self.conv1 = FFC_BN_ACT(in_channels=3 + 1, out_channels=64, kernel_size=3, ratio_gin=0.0, ratio_gout=r,
                                stride=1, **L)
        self.conv2 = FFC_BN_ACT(in_channels=64, out_channels=128, kernel_size=4, ratio_gin=r, ratio_gout=r,
                                stride=2, **L)
        self.conv3 = FFC_BN_ACT(in_channels=128, out_channels=256, kernel_size=4, ratio_gin=r, ratio_gout=r,
                                stride=2, **L)
        self.conv4 = FFC_BN_ACT(in_channels=256, out_channels=512, kernel_size=4, ratio_gin=r, ratio_gout=0.0,
                                stride=2, **L)
        self.label_embed = nn.Embedding(num_classes, 8 * 8 * self.mg * self.mg)
        self.fc = sn_fn(nn.Linear(self.mg * self.mg * 512, 1))
        self.gaus_noise = GaussianNoise(0.05)
        set_cond_bn(self)

    def forward(self, x, labels):
        x = rt.require(x, "x")
        side = 8 * self.mg
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, side, side):
            raise RuntimeError(f"FCondDiscriminator32: x must be (B, 3, {side}, {side}), got {tuple(x.shape)}")
        B = x.shape[0]
        x = self.gaus_noise(x)                                                              # :256
        plane = torch.ops.ffc.embed_rows(self.label_embed.weight, labels).view(B, 1, side, side)   # :258-261
        m = torch.cat([x, plane], dim=1)   # a 4-channel copy of the input image: data movement only
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):                       # :265-268
            m = conv(m, labels)
        m = self.resizer(m)
        return ag.linear(self.fc, m.reshape(-1, self.mg * self.mg * 512))                   # :271
