"""MI355X-native Fast Fourier Convolution: drop-in for the reference's ``layers`` FFC surface.

    from fastfourierconvolution_amd import *      # instead of  `from layers import *`

exports FourierUnitSN, SELayer, SpectralTransform, FFC, FFCTranspose, FFC_BN_ACT, SNFFC, SNFFCTranspose
(layers/snffc), Resizer,
Print, debug_print, NoiseInjection, GaussianNoise, Self_Attn, aw_method (the names layers/__init__.py:2-18 exports for this path)
plus the restated callers FFCModel / FFCGenerator / FFCDiscriminator / FGenerator and Discriminator (fgan128), the
class-conditional FCondGenerator / FCondDiscriminator (fgan128_cond_complete.py) and the 8*mg family
FGenerator32 / Discriminator32 / FDiscriminator32 (fgan_complete.py; 32x32 at mg = 4, 48x48 at mg = 6) with its
conditional-batch-norm variant ConditionalBatchNorm2d / FCondGenerator32 / FCondGeneratorSTL / CondDiscriminator32 /
FCondDiscriminator32 (layers/cond/cond_bn.py, fgan_cond_complete.py; set_cond_bn), and the plain
transposed-conv baselines the FFC generators are compared against: Generator32 (``Generator`` of
fgan_complete.py), Generator64 (``Generator`` of fgan64_complete.py) and DCGenerator32 (``Generator`` of
sngan_complete.py), and the ResNet SNGAN-128 baseline GBlock / DBlock / DBlockOptimized / SNGANGenerator128 /
SNGANDiscriminator128 (fgan128_complete.py:75-438; resnet.py), and the optimizers FusedAdamW / FusedAdam (optim.py:
torch.optim.AdamW / Adam in one HIP pass, with the reference's linear LR decay on the device):

    G = Generator32(z_size=128, mg=4).cuda().eval()      # Generator64 / DCGenerator32 alike
    with torch.no_grad():
        img_u8 = G(torch.randn(64, 128, device="cuda"))  # (64, 3, 32, 32) uint8; G.forward_float(z): the float image

All compute runs in the gfx950 HIP library libffc_amd.so (include/ffc_amd.h); there is no CPU fallback.
"""
from . import ops  # noqa: F401  (registers the torch.ops.ffc.* custom ops)
from .config import Config
from .ffc import (FFC, FFC_BN_ACT, SNFFC, ConditionalBatchNorm2d, FFCTranspose, FourierUnitSN, SELayer,
                  SNFFCTranspose, SpectralTransform, set_cond_bn, set_lfu, set_mix_precision, set_sn_hip,
                  spectral_norm_ffc)
from .attention_layer import Self_Attn
from .aw_loss import aw_method
from .layers_misc import GaussianNoise, NoiseInjection, Print, Resizer, debug_print
from .models import (CondDiscriminator32, DCGenerator32, Discriminator, Discriminator32, FCondDiscriminator, FCondDiscriminator32,
                     FCondGenerator, FCondGenerator32, FCondGeneratorSTL, FDiscriminator32, FFCDiscriminator,
                     FFCGenerator, FFCModel, FGanDiscriminator, FGenerator, FGenerator32, Generator32, Generator64)
from .optim import FusedAdam, FusedAdamW
from .resnet import DBlock, DBlockOptimized, GBlock, SNGANDiscriminator128, SNGANGenerator128
from .sagan import SAGANDiscriminator, SAGANGenerator, SAGANSpectralNorm

__all__ = ["FourierUnitSN", "SELayer", "SpectralTransform", "FFC", "FFCTranspose", "FFC_BN_ACT", "SNFFC",
           "SNFFCTranspose", "spectral_norm_ffc", "set_sn_hip", "set_mix_precision", "set_lfu", "Resizer",
           "Print", "debug_print", "NoiseInjection", "FFCModel", "FFCGenerator", "FFCDiscriminator", "FGenerator",
           "Discriminator", "FGanDiscriminator", "FCondGenerator", "FCondDiscriminator", "FGenerator32",
           "Discriminator32", "FDiscriminator32", "GaussianNoise", "Config", "ConditionalBatchNorm2d", "set_cond_bn",
           "FCondGenerator32", "FCondGeneratorSTL", "CondDiscriminator32", "FCondDiscriminator32", "Self_Attn",
           "Generator32", "Generator64", "DCGenerator32", "aw_method", "GBlock", "DBlock", "DBlockOptimized",
           "SNGANGenerator128", "SNGANDiscriminator128", "FusedAdamW", "FusedAdam", "SAGANSpectralNorm",
           "SAGANGenerator", "SAGANDiscriminator"]
