from .cond_bn import ConditionalBatchNorm2d
from .ffc import FFC
from .ffc_bn_act import FFC_BN_ACT, set_cond_bn
from .ffc_transpose import FFCTranspose
from .fourier_unity import FourierUnitSN
from .snffc import SNFFC, SNFFCTranspose, set_mix_precision, set_sn_hip, spectral_norm_ffc
from .spectral_transform import SELayer, SpectralTransform, set_lfu

__all__ = ["FFC", "FFC_BN_ACT", "FFCTranspose", "FourierUnitSN", "SELayer", "SpectralTransform", "SNFFC",
           "SNFFCTranspose", "spectral_norm_ffc", "set_sn_hip", "set_mix_precision", "set_lfu", "ConditionalBatchNorm2d", "set_cond_bn"]
