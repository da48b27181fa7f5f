"""The reference's third-party SAGAN baseline (benchmark_models/sagan/) on the HIP ops: its SpectralNorm
wrapper (spectral.py:14-68), Generator and Discriminator (sagan_models.py:42-164).  The hinge iteration of
its trainer is training.sagan_step.

The wrapper differs from torch.nn.utils.spectral_norm (the hook form the rest of the package runs, ffc/snffc.py)
in four ways, all kept: it is a module around the layer, so the state_dict keys are ``<wrapper>.module.bias /
weight_u / weight_v / weight_bar``; u and v are Parameters that do not require a gradient; the matrix view is
over dim 0 for ConvTranspose2d too; and one power iteration runs on EVERY forward, in eval mode as in
training, with l2normalize(x) = x / (||x|| + 1e-12).  The iteration, sigma and W = W_bar / sigma run in the
spectral-norm table of csrc/sn_kernels.hip with FFC_SN_EPS_ADD set (three launches for all wrappers of a
model); the gradient is the one ffc::sn_weight_bwd computes (u, v constants).  One more trait of the reference is
kept because its training results depend on it: its graph holds the Parameters u and v themselves, and every later
forward replaces their data, so a backward uses the vectors as they stand WHEN IT RUNS (sigma is the forward's own).
In the trainer's D half the critic runs twice before one backward: the gradient of the first call is taken with the
second call's u and v.  SpectralNormWeight does the same for these wrappers (``live``).

Only ``image_size = 32`` with ``conv_dim = 64`` can run in the reference: the attention widths are hard-coded
(Self_Attn(64) in G, Self_Attn(256) in D), and at 64 G's attn2 meets 128 channels and D's ``last`` =
Conv2d(512, 1, 4) meets 256.  The constructors here refuse what the reference cannot run."""
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _autograd as ag
from . import _runtime as rt
from .attention_layer import Self_Attn


def l2normalize(v, eps=1e-12):
    """spectral.py:10-11"""
    return v / (v.norm() + eps)


def refresh(wrappers):
    """One power iteration, sigma and ``module.<name> = <name>_bar / sigma`` for every SAGANSpectralNorm of
    ``wrappers`` in ONE table: three launches, u and v advanced in place on the device, nothing read back.
    The weight is a differentiable function of <name>_bar (SpectralNormWeight); train and eval mode alike."""
    wrappers = list(wrappers)
    if not wrappers:
        return
    layers, bars = [], []
    for sn in wrappers:
        u, v, w = sn._params()
        label = f"SAGANSpectralNorm({type(sn.module).__name__})"
        for t, what in ((w, "_bar"), (u, "_u"), (v, "_v")):
            if t.dtype != torch.float32:
                raise NotImplementedError(f"{label}: {sn.name}{what} is {t.dtype}; fp32 only")
            if not t.is_cuda:
                raise NotImplementedError(f"{label}: {sn.name}{what} is on {t.device}; the power iteration runs "
                                          "on the GPU only (no CPU fallback)")
        # dim 0, for ConvTranspose2d too (spectral.py:28); live: a backward reads u and v as they then stand
        layers.append(ag.SnLayer(u.data, v.data, 0, flags=ag.SN_EPS_ADD, live=True))
        bars.append(w)
    ws = ag.SpectralNormWeight.apply(layers, True, *bars)
    for sn, w in zip(wrappers, ws):
        setattr(sn.module, sn.name, w)


class sn_table:
    """``with sn_table(wrappers):`` -- refresh(wrappers) on entry, and the wrappers' own refresh inside the block
    a no-op: one iteration per wrapper and forward, as the reference's module calls run it (the iteration does
    not depend on activations, so running it up front changes no result)."""

    def __init__(self, wrappers):
        self.wrappers = list(wrappers)
        self.mine = []

    def __enter__(self):
        self.mine = [w for w in self.wrappers if not w.__dict__.get("_tabled")]   # an outer table's stay its own
        refresh(self.mine)
        for w in self.mine:
            w.__dict__["_tabled"] = True
        return self

    def __exit__(self, *exc):
        for w in self.mine:
            w.__dict__["_tabled"] = False
        return False


class SAGANSpectralNorm(nn.Module):
    """spectral.py:14-68 (``SpectralNorm`` there) around an nn.Conv2d or nn.ConvTranspose2d: constructor,
    parameter registration (``_made_params`` / ``_make_params``), u / v initialisation (normal, then
    l2normalize) and state_dict keys are the reference's, so its checkpoints load with strict=True.

    ``forward(x)``: the refresh above, then the wrapped convolution with its bias as one ffc::conv_layer job.
    ``run(x, act)`` is forward with an activation in the convolution's epilogue (the models use it).
    NotImplementedError: power_iterations != 1, a module other than Conv2d / ConvTranspose2d (at construction);
    non-fp32 or CPU tensors (at the call)."""

    def __init__(self, module, name='weight', power_iterations=1):
        super().__init__()
        if not isinstance(module, (nn.Conv2d, nn.ConvTranspose2d)):
            raise NotImplementedError(f"SAGANSpectralNorm({type(module).__name__}): Conv2d and ConvTranspose2d only")
        if power_iterations != 1:
            raise NotImplementedError(f"SAGANSpectralNorm({type(module).__name__}): power_iterations = "
                                      f"{power_iterations}; the kernels run one")
        self.module = module
        self.name = name
        self.power_iterations = power_iterations
        if not self._made_params():
            self._make_params()

    def _params(self):
        return (getattr(self.module, self.name + "_u"), getattr(self.module, self.name + "_v"),
                getattr(self.module, self.name + "_bar"))

    def _made_params(self):
        try:
            self._params()
            return True
        except AttributeError:
            return False

    def _make_params(self):
        w = getattr(self.module, self.name)
        height = w.data.shape[0]
        width = w.view(height, -1).data.shape[1]
        u = Parameter(w.data.new(height).normal_(0, 1), requires_grad=False)
        v = Parameter(w.data.new(width).normal_(0, 1), requires_grad=False)
        u.data = l2normalize(u.data)
        v.data = l2normalize(v.data)
        w_bar = Parameter(w.data)
        del self.module._parameters[self.name]
        self.module.register_parameter(self.name + "_u", u)
        self.module.register_parameter(self.name + "_v", v)
        self.module.register_parameter(self.name + "_bar", w_bar)

    def _update_u_v(self):
        refresh([self])

    def run(self, x, act=(0, 0.0)):
        if not self.__dict__.get("_tabled"):
            self._update_u_v()
        m = self.module
        x = rt.require(x, "x")
        (y,) = ag.conv_layer(x.shape[0], [(m.out_channels,) + tuple(act)], [(0, 0, rt.conv_seg(m, x), m)], [x])
        return y

    def forward(self, x):
        return self.run(x)


def _wrappers(model):
    return [m for m in model.modules() if isinstance(m, SAGANSpectralNorm)]


def _refuse(cls, image_size, conv_dim, at64):
    if image_size != 32:
        why = at64 if image_size == 64 else "only image_size = 32 builds a stack whose channels meet the hard-coded " \
                                            "attention widths"
        raise NotImplementedError(f"{cls}: image_size = {image_size} does not run in the reference: {why}")
    if conv_dim != 64:
        raise NotImplementedError(f"{cls}: conv_dim = {conv_dim} does not run in the reference: the attention widths "
                                  "are hard-coded (Self_Attn(64) in the generator, Self_Attn(256) in the critic), so "
                                  "conv_dim must be 64")


class SAGANGenerator(nn.Module):
    """sagan_models.py:42-110 (``Generator`` there) at image_size = 32: z (B, z_dim) viewed (B, z_dim, 1, 1) ->
    l1: SN-ConvTranspose2d(z, 256, 4) + BatchNorm2d + ReLU (4 x 4) -> l2: SN-ConvTranspose2d(256, 128, 4, 2, 1) + BN +
    ReLU (8 x 8) -> l3: 128 -> 64 (16 x 16) -> attn2 = Self_Attn(64) (N = 256) -> last: ConvTranspose2d(64, 3, 4, 2,
    1) + Tanh (32 x 32).  l4 is Identity and attn1 = Self_Attn(128) is built and never called, as in the reference;
    signature, attribute names and the 43 state_dict keys are the reference's (``batch_size`` is unused there too).

    Each SN-ConvTranspose2d is one ffc::conv_layer job on the refreshed weight (the three wrappers refreshed in one
    table), BatchNorm2d + ReLU one ffc::bn_act, the head runs on conv_route 'convT' with Tanh in its epilogue.
    Training mode returns (img, p2), p2 (B, 256, 256) the attention matrix (no gradient); ``need_attention =
    False`` returns None in its place and allocates nothing of that size.  Eval mode returns the uint8 image of
    :102-108 -- its clamp to the batch's own min / max is the identity -- as ffc::quantize_u8, with no host read;
    u and v advance in eval mode too.  ``forward_float(z)`` stops at the float image."""

    need_attention = True

    def __init__(self, batch_size, image_size=64, z_dim=100, conv_dim=64):
        super().__init__()
        _refuse("SAGANGenerator", image_size, conv_dim,
                "attn2 = Self_Attn(64) meets the 128 channels l3 leaves (l4 is never called)")
        self.imsize = image_size
        mult = 2 ** (self.imsize.bit_length() - 1 - 3)   # int(log2(imsize)) - 3
        self.l4 = nn.Identity()
        dims = [z_dim, conv_dim * mult, conv_dim * mult // 2, conv_dim * mult // 4]
        geom = [(4,), (4, 2, 1), (4, 2, 1)]
        for i, g in enumerate(geom):
            setattr(self, f"l{i + 1}", nn.Sequential(SAGANSpectralNorm(nn.ConvTranspose2d(dims[i], dims[i + 1], *g)),
                                                     nn.BatchNorm2d(dims[i + 1]), nn.ReLU()))
        self.last = nn.Sequential(nn.ConvTranspose2d(dims[3], 3, 4, 2, 1), nn.Tanh())
        self.attn1 = Self_Attn(128, 'relu')
        self.attn2 = Self_Attn(64, 'relu')

    def _run(self, z, want_matrix):
        from .models import _run_stack
        z = rt.require(z, "z")
        zc = self.l1[0].module.in_channels
        if z.dim() < 2 or z.size(1) != zc or z.numel() != z.size(0) * zc:
            raise RuntimeError(f"SAGANGenerator: z must be (B, {zc}), got {tuple(z.shape)}")
        out = z.view(z.size(0), z.size(1), 1, 1)
        with sn_table(_wrappers(self)):
            for seq in (self.l1, self.l2, self.l3):
                out = ag.bn_act(seq[1], seq[0].run(out), rt.act_code(seq[2]))
        out, p2 = ag.self_attn(self.attn2, out, bool(want_matrix))
        return _run_stack(self.last, out), p2

    def forward_float(self, z):
        return self._run(z, False)[0]

    def forward(self, z):
        if not self.training:
            return torch.ops.ffc.quantize_u8(self._run(z, False)[0])
        return self._run(z, self.need_attention)


class SAGANDiscriminator(nn.Module):
    """sagan_models.py:113-164 (``Discriminator`` there) at image_size = 32: l1: SN-Conv2d(3, 64, 4, 2, 1) +
    LeakyReLU(0.1) (16 x 16) -> l2: 64 -> 128 (8 x 8) -> l3: 128 -> 256 (4 x 4) -> attn1 = Self_Attn(256) -> last:
    Conv2d(256, 1, 4) -> (B, 1, 1, 1) -> squeeze: (B,), 0-dim at B = 1.  l4 is Identity and attn2 = Self_Attn(512) is
    built and never called (it keeps its keys; its forward would be refused).  28 state_dict keys, the reference's.

    Each SN-Conv2d is one implicit-GEMM launch with bias + LeakyReLU in its epilogue (the three wrappers refreshed
    in one table), attn1 runs on the wide attention kernels, ``last`` on conv_route 'full'.  Returns (out, p1), p1
    (B, 16, 16) (no gradient), or None in its place with ``need_attention = False``."""

    need_attention = True

    def __init__(self, batch_size=64, image_size=64, conv_dim=64):
        super().__init__()
        _refuse("SAGANDiscriminator", image_size, conv_dim,
                "last = Conv2d(512, 1, 4) meets the 256 channels l3 leaves (l4 is never called)")
        self.imsize = image_size
        self.l4 = nn.Identity()
        dims = [3, conv_dim, conv_dim * 2, conv_dim * 4]
        for i in range(3):
            setattr(self, f"l{i + 1}", nn.Sequential(SAGANSpectralNorm(nn.Conv2d(dims[i], dims[i + 1], 4, 2, 1)),
                                                     nn.LeakyReLU(0.1)))
        self.last = nn.Sequential(nn.Conv2d(dims[3], 1, 4))
        self.attn1 = Self_Attn(256, 'relu')
        self.attn2 = Self_Attn(512, 'relu')

    def forward(self, x):
        x = rt.require(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.imsize, self.imsize):
            raise RuntimeError(f"SAGANDiscriminator: x must be (B, 3, {self.imsize}, {self.imsize}), got "
                               f"{tuple(x.shape)}")
        out = x
        with sn_table(_wrappers(self)):
            for seq in (self.l1, self.l2, self.l3):
                out = seq[0].run(out, rt.act_code(seq[1]))
        out, p1 = ag.self_attn(self.attn1, out, bool(self.need_attention))
        last = self.last[0]
        (out,) = ag.conv_layer(out.shape[0], [(1, 0, 0.0)], [(0, 0, rt.conv_seg(last, out), last)], [out])
        return out.squeeze(), p1
