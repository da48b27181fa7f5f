"""Drop-in ``FourierUnitSN`` (reference: layers/ffc/fourier_unity.py:17-56).

Same constructor, attribute names (``conv_layer``, ``bn``, ``relu``) and state_dict keys;
forward runs the ffc::fourier_unit custom op -- the fused HIP Fourier unit (csrc/fu_kernels.hip,
csrc/fu2d_kernels.hip) -- instead of rfftn -> 1x1 conv -> BatchNorm2d -> ReLU -> irfftn (the
ffc::rfft2 / conv_layer / bn_act / irfft2 training ops under autograd).
"""
import ctypes

import torch
import torch.nn as nn

from .. import _autograd as ag
from .. import _runtime as rt
from .. import ops
from .._lib import check, ptr


class FourierUnitSN(nn.Module):
    def __init__(self, in_channels, out_channels, groups: int = 1, num_classes: int = 1):
        super().__init__()
        self._ffc_ctor = ["FourierUnitSN", dict(in_channels=in_channels, out_channels=out_channels, groups=groups,
                                                num_classes=num_classes)]
        self.groups = groups
        self.conv_layer = torch.nn.Conv2d(in_channels=in_channels * 2, out_channels=out_channels * 2,
                                          kernel_size=1, stride=1, padding=0, groups=self.groups, bias=False)
        self.bn = torch.nn.BatchNorm2d(out_channels * 2)
        self.relu = torch.nn.ReLU(inplace=True)
        self._packs = rt.PackCache()
        # "fp32" (exact, the reference's arithmetic) or "fp16": fp16 operands on the f16 MFMA with fp32
        # accumulation (BASELINE config 5); fp16 runs the staged FU (C in {16, 32, 64})
        self.mix_precision = "fp32"

    # ------------------------------------------------------------------ internals
    def _check(self, C):
        if self.groups != 1:
            raise NotImplementedError("grouped FourierUnitSN mix (groups != 1) is not on the hot path")
        if self.conv_layer.in_channels != 2 * C or self.conv_layer.out_channels != 2 * C:
            raise NotImplementedError("FourierUnitSN with in_channels != out_channels")

    def _packed_mix(self, device, stream):
        w = rt.require(self.conv_layer.weight.detach(), "conv_layer.weight")

        def build():
            C2 = w.shape[0]
            mixT = torch.empty((C2, -(-C2 // 32) * 32), device=device, dtype=torch.float32)
            check(rt.lib().ffc_fu_pack_mix(ptr(w), C2, ptr(mixT), stream), "ffc_fu_pack_mix")
            return mixT
        return self._packs.get("mix", [w], build)

    def _packed_mix3(self, mixT, device, stream):
        """the mix weight's split bf16 pieces in MFMA fragment order (ffc_fu_pack_mix3), or None when
        C % 8 != 0 (the fused kernel then splits wmixT itself)"""
        w = self.conv_layer.weight
        C = w.shape[0] // 2
        n = rt.lib().ffc_fu_mix3_elems(C)
        if n == 0:
            return None

        def build():
            w3 = torch.empty(int(n), device=device, dtype=torch.int16)
            check(rt.lib().ffc_fu_pack_mix3(ptr(mixT), C, ptr(w3), stream), "ffc_fu_pack_mix3")
            return w3
        return self._packs.get("mix3", [rt.require(w.detach(), "conv_layer.weight")], build)

    def _packed_mix16(self, device, stream):
        w = rt.require(self.conv_layer.weight.detach(), "conv_layer.weight")

        def build():
            C2 = w.shape[0]
            mix16 = torch.empty((-(-C2 // 32) * 32, C2), device=device, dtype=torch.float16)
            check(rt.lib().ffc_fu_pack_mix_f16(ptr(w), C2, ptr(mix16), stream), "ffc_fu_pack_mix_f16")
            return mix16
        return self._packs.get("mix16", [w], build)

    def route(self, B, C, H, W, up, in_bn=None):
        """rt.fu_route of this unit over (B, C, H, W) planes behind the BatchNorm ``in_bn`` (an rt.InBn)"""
        self._check(C)
        return rt.fu_route(B, C, H, W, up, self.mix_precision, rt.bn_mode(self.bn)[0], self.bn.momentum is None, in_bn)

    def _run(self, t, up=1, in_scale=None, in_shift=None, in_relu=False, residual=False, in_fold=None):
        """the Fourier unit over s = transform(t) (include/ffc_amd.h ffc_fu_forward_ex4 / ffc_fu2d_*).  in_fold:
        the input BN as a ready rt.BnFoldDesc, finalized inside the first kernel where the route folds it"""
        B, C, h, w = t.shape
        in_bn = None
        if in_fold is not None:
            in_bn = rt.InBn(in_fold.struct.nrows, in_fold.struct.count_mult, True, in_fold.bn.momentum is None,
                            ready=in_fold.kind)
        r = self.route(B, C, h * up, w * up, up, in_bn)
        if in_fold is not None and r.in_fold is None:
            in_scale, in_shift = in_fold.materialize(rt.stream_of(t))
            in_fold = None
        elif in_fold is not None and r.in_fold != in_fold.kind:   # a whole-slab descriptor, folded by channel
            in_fold = rt.make_bn_fold(in_fold.bn, C, in_fold.slab, in_fold.struct.nrows, in_fold.struct.count_mult,
                                      t.device, r.in_fold)
        return self._launch(r, t, up, in_scale, in_shift, in_relu, residual, in_fold)

    def _launch(self, r, t, up, in_scale, in_shift, in_relu, residual, in_fold):
        """the launches of route ``r`` (an rt.FuRoute).  in_fold: the rt.BnFoldDesc of r.in_fold, which the first
        kernel finalizes into in_fold.scale / in_fold.shift; else the input BN arrives as in_scale / in_shift"""
        B, C, h, w = t.shape
        H, W = h * up, w * up
        L, dev, stream = rt.lib(), t.device, rt.stream_of(t)
        fold_arg = ctypes.byref(in_fold.struct) if in_fold else None
        n_r, n_c = float(B * C * H * W), float(B * C * H * (W // 2 + 1))   # real / complex elements
        n_t = 4.0 * t.numel()                                             # bytes of t (the pre-upsample size)
        sc = sh = slab = rows = None
        if r.path == "fused":
            mixT = self._packed_mix(dev, stream)
            mix3 = self._packed_mix3(mixT, dev, stream)
            mix_fold = yspill = None
            if r.stats:
                rows = L.ffc_fu_slab_rows(B, C, H, W, r.kgroups)
                slab = torch.empty((rows, 2 * C, 4), device=dev, dtype=torch.float32)
                # pass 0 keeps its mix output Y for pass 1 (no second row R2C + column FFT + mix)
                yspill = torch.empty(int(2 * n_c), device=dev, dtype=torch.float32) if r.spill else None
                # bytes: SURVEY.md §8d's algorithmic basis (fused train FU = 12*N_r: x read in each pass,
                # out written once), never more than the kernel moves (t is read at the pre-upsample size);
                # moved: what this kernel pair actually streams (including the Y spill written and read back)
                mv0 = n_t + (8.0 * n_c if r.spill else 0.0)
                with rt.observe("fu_pass0", bytes=min(4.0 * n_r, mv0), moved=mv0):
                    check(L.ffc_fu_forward_ex4(ptr(t), B, C, H, W, up, None if in_fold else ptr(in_scale),
                                               None if in_fold else ptr(in_shift), int(in_relu), ptr(mixT), ptr(mix3), 0,
                                               ptr(slab), None, None, 0, None, fold_arg, None, ptr(yspill), r.kgroups,
                                               stream), "ffc_fu_forward(pass 0)")
                if in_fold is not None:          # pass 0's workgroup 0 wrote the folded bn1 affine
                    in_scale, in_shift = in_fold.scale, in_fold.shift
                if r.mix_fold:
                    mix_fold = rt.make_bn_fold(self.bn, 2 * C, slab, rows, 1.0, dev, r.bn_kind)
            if mix_fold is None:
                sc, sh = rt.bn_scale_shift(self.bn, 2 * C, slab, rows or 0, 1.0, dev, stream)
            out = torch.empty((B, C, H, W), device=dev, dtype=torch.float32)
            mv1 = (8.0 * n_c if yspill is not None else n_t) + n_t * bool(residual) + 4.0 * n_r
            with rt.observe("fu_pass1", bytes=min(8.0 * n_r, mv1), moved=mv1):
                check(L.ffc_fu_forward_ex4(ptr(t), B, C, H, W, up, ptr(in_scale), ptr(in_shift), int(in_relu),
                                           ptr(mixT), ptr(mix3), 1, None, ptr(sc), ptr(sh), int(residual), ptr(out), None,
                                           ctypes.byref(mix_fold.struct) if mix_fold else None, ptr(yspill), r.kgroups,
                                           stream), "ffc_fu_forward(pass 1)")
            return out
        # staged: r2c -> mix (pass 0 stats, pass 1 BN/ReLU) -> c2r
        f16 = self.mix_precision == "fp16"
        mixT = self._packed_mix16(dev, stream) if f16 else self._packed_mix(dev, stream)
        mixfn = L.ffc_fu2d_mix_f16 if f16 else L.ffc_fu2d_mix
        nT = B * C * h * (w // 2 + 1)           # complex bins of T
        mix_flops = 2.0 * (2 * C) ** 2 * (B * H * (W // 2 + 1))   # (2C x 2C) GEMM over every bin
        out = torch.empty((B, C, H, W), device=dev, dtype=torch.float32)
        T = Y = cfold = None
        if not r.r2c_mix:
            # SURVEY.md §8d's R2C bytes, capped at what the kernel moves: with the upsample folded in it
            # reads t (N_r / 4) and writes T (N_c / 4), and counting the full-resolution bytes would credit
            # bytes never transferred
            mvr = n_t + 8.0 * nT
            T = torch.empty((B, C, h, w // 2 + 1, 2), device=dev, dtype=torch.float32)
            with rt.observe("fu2d_r2c", bytes=min(4.0 * n_r + 8.0 * n_c, mvr), moved=mvr):
                check(L.ffc_fu2d_r2c_ex(ptr(t), B, C, h, w, ptr(in_scale), ptr(in_shift), int(in_relu), fold_arg, ptr(T),
                                        stream), "ffc_fu2d_r2c")
        if r.stats:
            rows = L.ffc_fu2d_slab_rows(B, C, H, W)
            slab = torch.empty((rows, 2 * C, 4), device=dev, dtype=torch.float32)
            # spill: pass 0 stores the raw Y and the C2R applies BN + ReLU on load (one mix instead of
            # two, and the statistics are taken from exactly the values they normalise)
            Y = torch.empty((B, C, H, W // 2 + 1, 2), device=dev, dtype=torch.float32) if r.spill else None
            if r.r2c_mix:
                # the R2C inside mix pass 0 (small t planes: every bin-range workgroup recomputes its
                # sample's T in LDS); labelled as the R2C stage, bytes = t in + the spilled Y out
                mv = n_t + 8.0 * n_c
                with rt.observe("fu2d_r2c", flops=mix_flops, bytes=min(4.0 * n_r + 8.0 * n_c, mv), moved=mv):
                    check(L.ffc_fu2d_r2c_mix(ptr(t), B, C, H, W, up, ptr(in_scale), ptr(in_shift), int(in_relu),
                                             fold_arg, ptr(mixT), ptr(slab), ptr(Y), stream), "ffc_fu2d_r2c_mix")
            else:
                with rt.observe("fu2d_mix0", flops=mix_flops, bytes=8.0 * nT + (8.0 * n_c if r.spill else 0.0)):
                    check(mixfn(ptr(T), B, C, H, W, up, ptr(mixT), 0, ptr(slab), None, None, ptr(Y), stream),
                          "ffc_fu2d_mix(pass 0)")
        if in_fold is not None:   # the r2c's (or r2c_mix's) leader workgroups wrote the folded bn1 affine
            in_scale, in_shift = in_fold.scale, in_fold.shift
        if r.c2r == "fold":   # the FU's BN finalized inside the C2R (two channels per plane)
            cfold = rt.make_bn_fold(self.bn, 2 * C, slab, rows, 1.0, dev, r.bn_kind)
        else:
            sc, sh = rt.bn_scale_shift(self.bn, 2 * C, slab, rows or 0, 1.0, dev, stream)
        if r.mix1 == "cols":
            # pass 1 with the inverse column FFT fused in (column-major Yc), then rows-only C2R
            Y = torch.empty((B, C, W // 2 + 1, H, 2), device=dev, dtype=torch.float32)
            with rt.observe("fu2d_mix1", flops=mix_flops, bytes=8.0 * nT + 8.0 * n_c):
                check(L.ffc_fu2d_mix_cols(ptr(T), B, C, H, W, up, ptr(mixT), int(f16), ptr(sc), ptr(sh), ptr(Y),
                                          stream), "ffc_fu2d_mix_cols")
        elif r.mix1 == "plain":
            Y = torch.empty((B, C, H, W // 2 + 1, 2), device=dev, dtype=torch.float32)
            with rt.observe("fu2d_mix1", flops=mix_flops, bytes=8.0 * nT + 8.0 * n_c):
                check(mixfn(ptr(T), B, C, H, W, up, ptr(mixT), 1, None, ptr(sc), ptr(sh), ptr(Y), stream),
                      "ffc_fu2d_mix(pass 1)")
        # the C2R of r.c2r: the whole-plane kernel with the BN on load (folded here, or given) or plain, or
        # the rows-only kernel behind mix_cols
        name = "ffc_fu2d_c2r" + {"fold": "_fold", "bn": "_bn", "rows": "_rows", "plain": ""}[r.c2r]
        tail = (ctypes.byref(cfold.struct),) if r.c2r == "fold" else (ptr(sc), ptr(sh)) if r.c2r == "bn" else ()
        c2r_moved = 8.0 * n_c + 4.0 * out.numel() + (n_t if residual else 0.0)
        with rt.observe("fu2d_c2r", bytes=min(8.0 * n_c + 4.0 * n_r, c2r_moved), moved=c2r_moved):   # §8d C2R pass
            check(getattr(L, name)(ptr(Y), B, C, H, W, ptr(t), up, ptr(in_scale), ptr(in_shift), int(in_relu),
                                   int(residual), *tail, ptr(out), stream), name)
        return out

    def forward(self, x, y=None):
        if y is not None:
            # reference: self.bn(ffted, y) -> BatchNorm2d.forward() takes 1 input (fourier_unity.py:46-47)
            raise TypeError("FourierUnitSN: the conditional (y) path is not supported (the reference raises here)")
        x = rt.require(x, "x")
        if ag.wants_grad(self, x):
            return ag.fourier_unit(self, x, residual=False)
        return ops.fu_forward(self, x)
