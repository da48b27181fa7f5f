"""Kernel-level parity of the forward spectral branch on the GPU -- the fused Fourier unit
(csrc/fu_kernels.hip), the staged large-plane Fourier unit (fu2d_kernels.hip), the SpectralTransform
prologue (st_prologue.hip, st_pw.hip), the SE gate and ffc_dense_forward -- each called through the C
ABI against a float64 CPU reference of the same operation (tests/spectral_refs.py, itself checked in
test_spectral_refs_cpu.py), at the shapes where the host code changes path.

Every output and slab is prefilled with NaN and must come back NaN-free.  Every returned tensor is
compared normwise (oracle.ffc_oracle.normwise_err), bound 1e-5 (exact-fp32 and fp32-accurate
split-bf16 kernels).  Slabs are merged in float64: n exact, mean and variance at rtol 1e-5 / atol 1e-6.
The fp16 mix is bound elementwise by |got - ref| <= 1.001 * 2^-10 * (|W| . |Z|) + 1e-5 * max|ref|: two
fp16 roundings per product (2 * 2^-11 + 2^-22 relative), fp32 accumulation inside the 1e-5 term; BN + ReLU
is 1-Lipschitz up to |scale|, and a column FFT sums the bounds of its column.

Observed maxima per family on the first MI355X run (normwise error, bound 1e-5 each; statistics as
max |mean - ref| / max relative variance error; 123 tests in 2.9 s, the bin-group cases under
FFC_FU_KGROUPS=2 in 2.1 s; the fp16 figures from the run that added its H 64 / 128 cases):
  fused FU   spill 4.5e-07  out 3.1e-07  stats 1.4e-07 / 4.6e-07
             folds: scale / shift / running statistics 2.5e-07  spill 1.4e-07  out 1.3e-07  stats 3.7e-08 / 3.7e-07
             bin groups: spill 3.0e-07  out 1.7e-07  stats 6.0e-08 / 6.6e-07
  staged FU  r2c 1.5e-07  mix pass 0 1.8e-07 (stats 1.7e-08 / 3.6e-07)  mix pass 1 4.6e-07  c2r 1.3e-07
             c2r_bn 8.9e-08  mix_cols 1.6e-07  c2r_rows 1.1e-07  r2c_mix 2.1e-07 (stats 1.7e-08 / 4.0e-07)
  fp16 mix   largest |got - ref| / limit: pass 0 0.40  pass 1 0.42  mix_cols 0.045 (normwise 5.4e-04,
             8.5e-04, 5.1e-04); statistics against the spilled Y 1.2e-08 / 2.6e-07
  prologue   gate 1.0e-07  t 1.5e-07  stats 4.8e-08 / 2.2e-07     pw_gate 1.7e-07  stats 4.1e-08 / 9.4e-08
  se_gate 1.4e-07   dense 5.2e-07

Case -> branch it is there for
  fused FU (C, H, W); `f32` = ffc_fu_forward_ex (f32-input MFMA), `split` = _ex3 with wmix3 (C % 8 == 0)
  (1, 4, 4)     smallest: 2C = 2, one partly filled M-tile; the full cross up x residual x affine x ReLU
  (5, 8, 32) (24, 32, 8)  non-square both ways, no split pass 1; C = 5 has no wmix3
  (40, 16, 16)  near the 160 KiB limit, scratch behind the planes; f32 weight in LDS, split weight in L2;
                split pass 1 (one wave per 4 channels); MT = 3: one M-group
  (96, 8, 8)    weight in L2 for both; MT = 6: two M-groups (2B <= CUs)
  (32, 16, 32) (16, 32, 32)  plane >= FU_SCRATCH: scratch in the Y-imaginary plane ((32, 16, 32) split: L2)
  (128, 4, 4)   no 4x4 split instance: pass 1 from the spill inside fu_kernel
  (32, 4, 4)    B = 130 (2B > CUs: one M-group) and its first two samples at B = 2 (two M-groups)
  (12, 8, 8)    C % 8 != 0: no wmix3; C % (64 / H) != 0: no split pass 1
  fold          in_fold on pass 0, mix_fold on pass 1 (whole-slab folds): (32, 4, 4) momentum 0.1,
                (16, 8, 16) momentum -1 (cumulative); planes >= the fold scratch, no split pass 1
  bin_group     ffc_fu_forward_ex4 kgroups = 2 (FFC_FU_KGROUPS=2: tests/test_gpu_fu_kg_env.py's child)
  staged FU
  r2c h = 8..64 (B 2, C 3), 128 (B 1): every line-FFT instance; input affine x ReLU, all four
  mix (3, 16, 2) h = 8; C 3 / 16 / 17 / 32 / 64 -> Mpad 32 / 32 / 64 / 64 / 128, 2C = 6, 34 ragged tiles;
                H 16 / 32 / 64; C = 3 cases at B = 1 and the smallest B whose mix_nsplit differs
  c2r / c2r_bn  H 16..64 up 1 / 2, 128 at B = 1;  mix_cols + c2r_rows H 32 / 64 / 128, C 16 / 32
  r2c_mix       (C, h) in {16, 32} x {8, 16}, explicit in_scale / in_shift
  f16           mix_f16 pass 0 / 1 at C 16 / 32 / 64, H 16..128; the cases marked `cols` (C 16 / 32 / 64 at
                H 32, C 16 at H 64, C 32 at H 128) must also reach the f16 mix_cols
  prologue (Cin, c, H): (16, 8, 8) hidden 0 / 1 / 4, ex and ex3; (24, 40, 6) c and h*w not multiples of
                32, 4 tiles: split 1 / 2 / 4; (64, 32, 16) pooled; (17, 5, 5) Cin*H*W % 4 != 0: x_dma off
  pw_gate       M 5 / 32 / 48 / 128 -> pw_gate_kernel<1 / 2 / 4>; HW 255 / 256 / 257 / 4096; gate and
                slab NULL or given; Cin 6, 7, 13
  se_gate       HW 1, 9, 4096 (wide), pool, hidden 0, C = 300
  dense         K 3 / 100 / 128 (KH 64), 129 / 256 (KH 128); N % 4 != 0 or K % 4 != 0 scalar staging;
                N0 < N; B 1 / 33; bias NULL; act 0 / 2 / 5; K = 257 rejected
"""
import ctypes
import functools
import os

import pytest
import torch

import spectral_refs as sr
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-5
NAN = float("nan")
FU_SCRATCH = 8 * 32 * 33      # csrc/fu_kernels.hip
LDS_MAX = 160 * 1024


def _lib():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _runtime as rt
    return rt.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(status, what):
    from fastfourierconvolution_amd._lib import check
    check(status, what)


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


_LIVE = []


def _dev(t):
    """a device copy that stays alive until the test ends (the ABI takes raw pointers: a temporary freed
    before the launch could be handed to the next allocation)"""
    if t is None:
        return None
    _LIVE.append(t.to(DEV).contiguous())
    return _LIVE[-1]


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def _padded(n):
    """a zeroed device buffer of n floats rounded up to the kernels' 256-float DMA groups"""
    return torch.zeros((n + 255) // 256 * 256, device=DEV, dtype=torch.float32)


def _err(family, what, out, ref):
    """print, then return, the normwise error of a returned tensor (which must hold no NaN)"""
    assert not torch.isnan(out).any(), f"{what}: unwritten (NaN) elements"
    e = normwise_err(out.detach().cpu().double().reshape(ref.shape), ref)
    print(f"OBS {family} {what} {e:.3e}")
    return e


def _check_slab(family, what, slab, stats):
    """merge the {n, mean, M2} rows in float64 and compare with (n, mean, var)"""
    assert not torch.isnan(slab).any(), f"{what}: unwritten slab rows"
    n, mean, var = sr.merge_slab(slab.cpu())
    n0, mean0, var0 = stats
    assert torch.equal(n, torch.full_like(n, float(n0))), (what, n, n0)
    print(f"OBS {family}_stats {what} mean {(mean - mean0).abs().max():.3e} var {((var - var0).abs() / var0).max():.3e}")
    torch.testing.assert_close(mean, mean0, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} mean: {m}")
    torch.testing.assert_close(var, var0, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} var: {m}")


# --------------------------------------------------------------------------- fused Fourier unit
def _fu_layout(C, H, W, packed):
    """fu_layout of csrc/fu_kernels.hip: the LDS bytes of the weight-in-LDS and weight-in-L2 candidates,
    and whether the statistics scratch lives in the Y-imaginary plane"""
    plane = C * H * (W // 2 + 1)
    in_y = plane >= FU_SCRATCH
    Mpad = (2 * C + 31) // 32 * 32
    wfl = ((Mpad // 32) * (C // 8) * 768 + 255) // 256 * 256 if packed else (2 * C * Mpad + 255) // 256 * 256
    base = 4 * plane + (0 if in_y else FU_SCRATCH) + 6 * C
    return 4 * (base + wfl), 4 * base, in_y


def _assert_fu_branch(C, H, W, wm_f32, wm_split, in_y):
    """the case takes the LDS branches it is there for (weight placement for the f32 and the pre-split
    weight, scratch placement).  Only the f32 layout is pinned by the library's own byte count
    (ffc_fu_lds_bytes); the library has no query for the pre-split weight's layout, so wm_split is checked
    against this file's restatement of fu_wm3_floats alone: if that formula changes in fu_kernels.hip,
    _fu_layout has to follow it by hand."""
    lds, l2, y = _fu_layout(C, H, W, False)
    assert y == in_y
    assert (lds <= LDS_MAX) == wm_f32 and l2 <= LDS_MAX
    assert _lib().ffc_fu_lds_bytes(C, H, W) == (lds if wm_f32 else l2)
    if wm_split is not None:
        assert C % 8 == 0 and _lib().ffc_fu_mix3_elems(C) > 0
        assert (_fu_layout(C, H, W, True)[0] <= LDS_MAX) == wm_split
    else:
        assert C % 8 != 0 and _lib().ffc_fu_mix3_elems(C) == 0


def _split_pass1(C, H, W):
    """the host rule for the one-wave-per-channel-group pass 1 (pick_split and its caller in fu_kernels.hip),
    restated: the library offers no query for this choice, so a change of the rule there is not noticed here"""
    return H == W and H in (8, 16, 32) and C % (64 // H) == 0


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


_fu_case = functools.lru_cache(maxsize=None)(sr.fu_case)


def _pack_mix(wmix, C, split):
    L = _lib()
    Mpad = (2 * C + 31) // 32 * 32
    wmixT = _padded(2 * C * Mpad)
    wd = _dev(wmix)
    _ok(L.ffc_fu_pack_mix(_ptr(wd), 2 * C, _ptr(wmixT), _stream()), "ffc_fu_pack_mix")
    w3 = None
    if split:
        n = L.ffc_fu_mix3_elems(C)
        assert n > 0
        w3 = torch.zeros(int(n), device=DEV, dtype=torch.int16)
        _ok(L.ffc_fu_pack_mix3(_ptr(wmixT), C, _ptr(w3), _stream()), "ffc_fu_pack_mix3")
    torch.cuda.synchronize()
    return wmixT, w3


def _fold(slab, C, gamma, beta, momentum, rm, rv, nbt, scale_out, shift_out, count_mult=1.0):
    from fastfourierconvolution_amd._lib import BnFold
    f = BnFold(_ptr(slab), slab.shape[0], C, _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(nbt), 1, momentum,
               sr.BN_EPS, count_mult, _ptr(scale_out), _ptr(shift_out), None)
    f.keep = (slab, gamma, beta, rm, rv, nbt, scale_out, shift_out)    # the struct holds raw pointers only
    return f


def _fu_launch(d, t, up, relu, residual, wmixT, w3, use_ex3, yspill_in=None, in_scale=None, in_shift=None,
               in_fold=None, mix_fold=None, bn=True, kgroups=None):
    """pass 0 (yspill_in is None) or pass 1 (from yspill_in, or recomputing when it is False)"""
    L = _lib()
    B, C, h, w = t.shape
    H, W = h * up, w * up
    pass1 = yspill_in is not None
    slab = spill = out = None
    if not pass1:
        rows = B * (2 if kgroups == 2 else 1)
        slab, spill = _nan((rows, 2 * C, 4)), _nan((B, 2 * C, H, W // 2 + 1))
        ys = spill
    else:
        out = _nan((B, C, H, W))
        ys = None if yspill_in is False else yspill_in
    sc = _dev(d["bn_scale"]) if pass1 and bn else None
    sh = _dev(d["bn_shift"]) if pass1 and bn else None
    head = (_ptr(t), B, C, H, W, up, _ptr(in_scale), _ptr(in_shift), int(relu), _ptr(wmixT))
    tail = (int(pass1), _ptr(slab), _ptr(sc), _ptr(sh), int(residual), _ptr(out),
            ctypes.byref(in_fold) if in_fold is not None else None,
            ctypes.byref(mix_fold) if mix_fold is not None else None, _ptr(ys))
    if kgroups is not None:
        rc = L.ffc_fu_forward_ex4(*head, _ptr(w3), *tail, kgroups, _stream())
    elif use_ex3:
        rc = L.ffc_fu_forward_ex3(*head, _ptr(w3), *tail, _stream())
    else:
        rc = L.ffc_fu_forward_ex(*head, *tail, _stream())
    _ok(rc, "ffc_fu_forward")
    torch.cuda.synchronize()
    return (slab, spill) if not pass1 else out


def _fu_check(B, C, h, w, up, affine, relu, residual, variant, nb=None, family="fu"):
    """pass 0 with a spill, pass 1 from the spill and recomputing, each against fp64; nb: run the first
    nb samples of the case only"""
    d = _fu_case(B, C, h, w, up, affine, relu)
    nb = nb or B
    split = variant == "split"
    wmixT, w3 = _pack_mix(d["wmix"], C, split)
    t, isc, ish = _dev(d["t"][:nb]), _dev(d["in_scale"]), _dev(d["in_shift"])
    what = f"({C},{h * up},{w * up}) B={nb} up={up} aff={int(affine)} relu={int(relu)} res={int(residual)} {variant}"
    slab, spill = _fu_launch(d, t, up, relu, residual, wmixT, w3, split, in_scale=isc, in_shift=ish)
    Y = d["Y"][:nb]
    errs = [_err(family + "_spill", what, spill, Y)]
    _check_slab(family, what, slab, sr.channel_stats(Y) if nb != B else d["stats"])
    ref = (d["out_res"] if residual else d["out"])[:nb]
    for ys, name in ((spill, "from spill"), (False, "recompute")):
        out = _fu_launch(d, t, up, relu, residual, wmixT, w3, split, yspill_in=ys, in_scale=isc, in_shift=ish)
        errs.append(_err(family + "_out", f"{what} {name}", out, ref))
    assert max(errs) <= TOL, errs


_CROSS = [(up, res, aff, relu) for up in (1, 2) for res in (0, 1) for aff in (0, 1) for relu in (0, 1)]


@pytest.mark.parametrize("up,residual,affine,relu", _CROSS)
def test_fu_smallest_full_cross(up, residual, affine, relu):
    _assert_fu_branch(1, 4, 4, True, None, False)
    _fu_check(3, 1, 4 // up, 4 // up, up, bool(affine), bool(relu), bool(residual), "f32")


# (C, H, W): B, up, weight in LDS (f32), weight in LDS (split; None: no wmix3), scratch in Y-imaginary
_FU_SHAPES = {
    (5, 8, 32): (3, 1, True, None, False),
    (24, 32, 8): (2, 2, True, True, False),
    (40, 16, 16): (3, 2, True, False, False),
    (96, 8, 8): (3, 1, False, False, False),
    (32, 16, 32): (2, 1, True, False, True),
    (16, 32, 32): (2, 2, True, True, True),
    (128, 4, 4): (3, 1, False, False, False),
    (12, 8, 8): (4, 2, True, None, False),
}
_FU_RUNS = [(k, v) for k, s in _FU_SHAPES.items() for v in (("f32", "split") if s[3] is not None else ("f32",))]


@pytest.mark.parametrize("shape,variant", _FU_RUNS, ids=[f"{k[0]}x{k[1]}x{k[2]}-{v}" for k, v in _FU_RUNS])
def test_fu_shapes_match_fp64(shape, variant):
    C, H, W = shape
    B, up, wm_f32, wm_split, in_y = _FU_SHAPES[shape]
    _assert_fu_branch(C, H, W, wm_f32, wm_split, in_y)
    MT = (2 * C + 31) // 32
    assert _split_pass1(C, H, W) == (shape in ((40, 16, 16), (96, 8, 8), (16, 32, 32)))
    if shape == (40, 16, 16):
        assert MT == 3                                     # odd: one M-group
    if shape == (96, 8, 8):
        assert MT == 6 and 2 * B <= _cus()                 # two M-groups
    _fu_check(B, C, H // up, W // up, up, True, True, True, variant)


@pytest.mark.parametrize("variant", ["f32", "split"])
@pytest.mark.parametrize("nb", [130, 2])
def test_fu_mgroups_switch(nb, variant):
    """(32, 4, 4): MT = 2, so pass 0 runs two M-groups per sample at B = 2 and one at B = 130 (2B > CUs); the
    B = 2 run is the first two samples of the same data"""
    _assert_fu_branch(32, 4, 4, True, True, False)
    assert (2 * nb <= _cus()) == (nb == 2)
    _fu_check(130, 32, 4, 4, 1, True, True, True, variant, nb=nb)


@pytest.mark.parametrize("C,h,w,up,B,momentum", [(32, 4, 4, 1, 3, 0.1), (16, 4, 8, 2, 2, -1.0)])
def test_fu_folds_match_fp64(C, h, w, up, B, momentum):
    """in_fold (bn1 from a slab, pass 0) and mix_fold (the FU's BN from pass 0's slab, pass 1): scale_out /
    shift_out, running statistics and num_batches_tracked against bn_finalize, out against fp64"""
    H, W = h * up, w * up
    assert 16 * C * H * (W // 2 + 1) >= 8 * (3 * 512 // 4)      # plane holds the in-kernel fold's scratch
    assert not _split_pass1(C, H, W)                            # whole-slab mix fold inside fu_kernel
    gen = torch.Generator().manual_seed(11 + C)
    # bn1: a slab of 5 uneven rows over some pre-BN tensor u; its fold gives (in_scale, in_shift)
    u = torch.randn(4, C, 3, 5, generator=gen) * 1.5 + 0.4
    slab1 = sr.make_slab(u, (7, 8, 30, 31))
    g1 = 0.5 + torch.rand(C, generator=gen)
    b1 = 0.2 * torch.randn(C, generator=gen)
    rm1, rv1 = 0.1 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    n1, m1, v1 = sr.merge_slab(slab1)
    nbt0 = 3
    isc64, ish64, rm1_ref, rv1_ref, _ = sr.bn_finalize(n1[0].item(), m1, v1, g1, b1, sr.BN_EPS, momentum, 2.0, rm1, rv1,
                                                      nbt0)
    t = sr.clear_input(torch.randn(B, C, h, w, generator=gen), isc64, ish64)
    wmix = torch.randn(2 * C, 2 * C, generator=gen) / (2 * C) ** 0.5
    s, _, Y = sr.fu_stages(t, isc64, ish64, True, up, wmix)
    stats = sr.channel_stats(Y)
    g2 = (0.5 + torch.rand(2 * C, generator=gen)) * (1 - 2 * (torch.arange(2 * C) % 2)).float()
    sc2, sh2, _, _, _ = sr.bn_finalize(*stats, g2, torch.zeros(2 * C))
    b2 = (sr.clear_shifts(Y, sc2.float(), 0.2 * torch.randn(2 * C, generator=gen)).double() + stats[1] * sc2).float()
    rm2, rv2 = 0.1 * torch.randn(2 * C, generator=gen), 0.5 + torch.rand(2 * C, generator=gen)
    sc2, sh2, rm2_ref, rv2_ref, _ = sr.bn_finalize(*stats, g2, b2, sr.BN_EPS, momentum, 1.0, rm2, rv2, nbt0)
    assert (Y * sc2[None, :, None, None] + sh2[None, :, None, None]).abs().min() >= sr.KINK
    ref = sr.fu_out(Y, sc2, sh2, s, True, H, W)

    wmixT, w3 = _pack_mix(wmix, C, True)
    td = _dev(t)
    d_rm1, d_rv1, d_nbt1 = _dev(rm1), _dev(rv1), torch.tensor([nbt0], device=DEV, dtype=torch.int64)
    isc, ish = _nan((C,)), _nan((C,))
    f1 = _fold(_dev(slab1), C, _dev(g1), _dev(b1), momentum, d_rm1, d_rv1, d_nbt1, isc, ish, count_mult=2.0)
    keep = [f1]
    slab, spill = _fu_launch(None, td, up, True, True, wmixT, w3, True, in_fold=f1)
    what = f"fold ({C},{H},{W}) momentum={momentum}"
    errs = [_err("fu_fold", what + " in_scale", isc, isc64), _err("fu_fold", what + " in_shift", ish, ish64),
            _err("fu_fold", what + " bn1 running_mean", d_rm1, rm1_ref),
            _err("fu_fold", what + " bn1 running_var", d_rv1, rv1_ref),
            _err("fu_fold_spill", what, spill, Y)]
    assert int(d_nbt1) == nbt0 + 1
    _check_slab("fu_fold", what, slab, stats)
    for ys in (spill, False):
        d_rm2, d_rv2, d_nbt2 = _dev(rm2), _dev(rv2), torch.tensor([nbt0], device=DEV, dtype=torch.int64)
        so, sho = _nan((2 * C,)), _nan((2 * C,))
        f2 = _fold(slab, 2 * C, _dev(g2), _dev(b2), momentum, d_rm2, d_rv2, d_nbt2, so, sho)
        keep.append(f2)
        out = _fu_launch(None, td, up, True, True, wmixT, w3, True, yspill_in=ys, in_scale=isc, in_shift=ish,
                         mix_fold=f2, bn=False)
        errs += [_err("fu_fold_out", what, out, ref), _err("fu_fold", what + " scale_out", so, sc2),
                 _err("fu_fold", what + " shift_out", sho, sh2),
                 _err("fu_fold", what + " running_mean", d_rm2, rm2_ref),
                 _err("fu_fold", what + " running_var", d_rv2, rv2_ref)]
        assert int(d_nbt2) == nbt0 + 1
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("C,H,up,B", [(16, 16, 2, 3), (32, 8, 1, 5), (16, 32, 2, 2), (128, 8, 2, 2)])
def test_fu_bin_group_pass0_matches_fp64(C, H, up, B):
    """ffc_fu_forward_ex4 with kgroups = 2: 2B slab rows (row g B + b: the bins of group g), the spill in
    [group][row][column in group] order, and pass 1 from that spill"""
    L = _lib()
    if os.environ.get("FFC_FU_KGROUPS") == "2":
        # in tests/test_gpu_fu_kg_env.py's child every case must qualify: none may skip unnoticed there
        assert L.ffc_fu_kgroups(B, C, H, H) == 2, "case no longer takes the bin-group pass 0"
    if L.ffc_fu_kgroups(B, C, H, H) != 2:
        pytest.skip("bin groups off (FFC_FU_KGROUPS=2 turns them on; tests/test_gpu_fu_kg_env.py runs them)")
    assert L.ffc_fu_slab_rows(B, C, H, H, 2) == 2 * B
    d = _fu_case(B, C, H // up, H // up, up, True, True)
    wmixT, w3 = _pack_mix(d["wmix"], C, True)
    t, isc, ish = _dev(d["t"]), _dev(d["in_scale"]), _dev(d["in_shift"])
    slab, spill = _fu_launch(d, t, up, True, True, wmixT, w3, True, in_scale=isc, in_shift=ish, kgroups=2)
    WP = H // 2 + 1
    KW0 = (WP + 1) // 2
    Y = d["Y"]
    ordered = torch.cat((Y[..., :KW0].reshape(B, 2 * C, -1), Y[..., KW0:].reshape(B, 2 * C, -1)), dim=2)
    what = f"bin_group ({C},{H},{H}) B={B} up={up}"
    errs = [_err("fu_kg_spill", what, spill, ordered)]
    _check_slab("fu_kg", what, slab, d["stats"])
    n_rows = slab[..., 0].cpu()
    assert torch.equal(n_rows[:B], torch.full((B, 2 * C), float(H * KW0)))
    assert torch.equal(n_rows[B:], torch.full((B, 2 * C), float(H * (WP - KW0))))
    for b in range(B):     # each row holds its own sample and group
        for g, cols in ((0, slice(0, KW0)), (1, slice(KW0, WP))):
            mean = Y[b, :, :, cols].mean(dim=(1, 2))
            torch.testing.assert_close(slab[g * B + b, :, 1].cpu().double(), mean, rtol=1e-5, atol=1e-6)
    out = _fu_launch(d, t, up, True, True, wmixT, w3, True, yspill_in=spill, in_scale=isc, in_shift=ish, kgroups=2)
    errs.append(_err("fu_kg_out", what, out, d["out_res"]))
    assert max(errs) <= TOL, errs


# --------------------------------------------------------------------------- staged Fourier unit
def _nsplit(B, H, W):
    """mix_nsplit of csrc/fu2d_kernels.hip (MIX_TILES_PER_WG = 32, fill target 512)"""
    ntiles = (H * (W // 2 + 1) + 31) // 32
    return max(1, min(ntiles, max(ntiles // 32, (512 + B - 1) // B)))


def _other_b(H):
    """the smallest B whose mix_nsplit differs from B = 1's"""
    return next(B for B in range(2, 1025) if _nsplit(B, H, H) != _nsplit(1, H, H))


@pytest.mark.parametrize("affine,relu", [(True, True), (False, False), (False, True), (True, False)])
@pytest.mark.parametrize("B,C,h", [(2, 3, 8), (2, 3, 16), (2, 3, 32), (2, 3, 64), (1, 3, 128)])
def test_fu2d_r2c_matches_fp64(B, C, h, affine, relu):
    d = _fu_case(B, C, h, h, 1, affine, relu)
    T = _nan((B, C, h, h // 2 + 1, 2))
    _ok(_lib().ffc_fu2d_r2c(_ptr(_dev(d["t"])), B, C, h, h, _ptr(_dev(d["in_scale"])), _ptr(_dev(d["in_shift"])),
                            int(relu), _ptr(T), _stream()), "ffc_fu2d_r2c")
    torch.cuda.synchronize()
    ref = sr.fu2d_T(d["t"], d["in_scale"], d["in_shift"], relu)
    assert _err("fu2d_r2c", f"h={h} affine={int(affine)} relu={int(relu)}", T, ref) <= TOL


def _mix_ops(d, nb, C, H, up):
    """device operands of a staged mix on the first nb samples: the float32 rounding of the fp64 T, wmixT"""
    T = _dev(sr.fu2d_T(d["t"][:nb], d["in_scale"], d["in_shift"], True).float())
    wmixT, _ = _pack_mix(d["wmix"], C, False)
    return T, wmixT


_MIX = [(3, 16, 2, "other"), (3, 32, 1, "other"), (3, 64, 1, "other"), (16, 16, 1, 2), (17, 32, 2, 2), (32, 32, 1, 2),
        (64, 16, 1, 2), (16, 64, 2, 2)]


@pytest.mark.parametrize("C,H,up,B", _MIX)
def test_fu2d_mix_matches_fp64(C, H, up, B):
    """pass 0 (slab with ffc_fu2d_slab_rows rows + raw Y) and pass 1, from the fp64 T; at B = 1 too (the
    first sample of the same data) where B is the smallest batch with another mix_nsplit"""
    L = _lib()
    assert L.ffc_fu2d_supported(C, H, H, up)
    Bs = [B]
    if B == "other":
        B = _other_b(H)
        Bs = [1, B]
        assert L.ffc_fu2d_slab_rows(1, C, H, H) == _nsplit(1, H, H)
        assert L.ffc_fu2d_slab_rows(B, C, H, H) == B * _nsplit(B, H, H) != B * _nsplit(1, H, H)
    d = _fu_case(B, C, H // up, H // up, up, True, True)
    errs = []
    for nb in Bs:
        T, wmixT = _mix_ops(d, nb, C, H, up)
        rows = L.ffc_fu2d_slab_rows(nb, C, H, H)
        slab, Y = _nan((rows, 2 * C, 4)), _nan((nb, C, H, H // 2 + 1, 2))
        _ok(L.ffc_fu2d_mix(_ptr(T), nb, C, H, H, up, _ptr(wmixT), 0, _ptr(slab), None, None, _ptr(Y), _stream()),
            "ffc_fu2d_mix(pass 0)")
        what = f"({C},{H}) up={up} B={nb}"
        torch.cuda.synchronize()
        errs.append(_err("fu2d_mix0", what, Y, sr.fu2d_Y(d["Y"][:nb])))
        _check_slab("fu2d_mix0", what, slab, sr.channel_stats(d["Y"][:nb]))
        Y1 = _nan((nb, C, H, H // 2 + 1, 2))
        _ok(L.ffc_fu2d_mix(_ptr(T), nb, C, H, H, up, _ptr(wmixT), 1, None, _ptr(_dev(d["bn_scale"])),
                           _ptr(_dev(d["bn_shift"])), _ptr(Y1), _stream()), "ffc_fu2d_mix(pass 1)")
        torch.cuda.synchronize()
        errs.append(_err("fu2d_mix1", what, Y1, sr.fu2d_Y(sr.bn_relu(d["Y"][:nb], d["bn_scale"], d["bn_shift"]))))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("B,C,H,up", [(2, 3, 16, 1), (2, 3, 16, 2), (2, 3, 32, 2), (2, 3, 64, 1), (2, 3, 64, 2),
                                      (1, 3, 128, 1), (1, 3, 128, 2)])
def test_fu2d_c2r_matches_fp64(B, C, H, up):
    """ffc_fu2d_c2r from the BN + ReLU'd spectrum and ffc_fu2d_c2r_bn from the raw one, with the residual
    rebuilt from t (input affine + ReLU, upsample)"""
    L = _lib()
    d = _fu_case(B, C, H // up, H // up, up, True, True)
    t, isc, ish = _dev(d["t"]), _dev(d["in_scale"]), _dev(d["in_shift"])
    Yraw = _dev(sr.fu2d_Y(d["Y"]).float())
    Ybn = _dev(sr.fu2d_Y(sr.bn_relu(d["Y"], d["bn_scale"], d["bn_shift"])).float())
    errs = []
    for res in (0, 1):
        ref = d["out_res"] if res else d["out"]
        out = _nan((B, C, H, H))
        _ok(L.ffc_fu2d_c2r(_ptr(Ybn), B, C, H, H, _ptr(t), up, _ptr(isc), _ptr(ish), 1, res, _ptr(out), _stream()),
            "ffc_fu2d_c2r")
        torch.cuda.synchronize()
        errs.append(_err("fu2d_c2r", f"H={H} up={up} res={res}", out, ref))
        out = _nan((B, C, H, H))
        _ok(L.ffc_fu2d_c2r_bn(_ptr(Yraw), B, C, H, H, _ptr(t), up, _ptr(isc), _ptr(ish), 1, res,
                              _ptr(_dev(d["bn_scale"])), _ptr(_dev(d["bn_shift"])), _ptr(out), _stream()),
            "ffc_fu2d_c2r_bn")
        torch.cuda.synchronize()
        errs.append(_err("fu2d_c2r_bn", f"H={H} up={up} res={res}", out, ref))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("B,C,H,up", [(2, 16, 32, 1), (2, 32, 32, 2), (2, 16, 64, 2), (1, 32, 64, 1), (1, 16, 128, 2)])
def test_fu2d_cols_and_rows_match_fp64(B, C, H, up):
    """ffc_fu2d_mix_cols (Yc: inverse column FFT of the BN + ReLU'd mix, column-major) from the fp64 T, and
    ffc_fu2d_c2r_rows from the fp64 Yc"""
    L = _lib()
    assert L.ffc_fu2d_cols_supported(C, H, H, up, 0)
    d = _fu_case(B, C, H // up, H // up, up, True, True)
    T, wmixT = _mix_ops(d, B, C, H, up)
    Yc = _nan((B, C, H // 2 + 1, H, 2))
    _ok(L.ffc_fu2d_mix_cols(_ptr(T), B, C, H, H, up, _ptr(wmixT), 0, _ptr(_dev(d["bn_scale"])),
                            _ptr(_dev(d["bn_shift"])), _ptr(Yc), _stream()), "ffc_fu2d_mix_cols")
    torch.cuda.synchronize()
    ref = sr.fu2d_Yc(d["Y"], d["bn_scale"], d["bn_shift"])
    errs = [_err("fu2d_cols", f"({C},{H}) up={up}", Yc, ref)]
    t, isc, ish = _dev(d["t"]), _dev(d["in_scale"]), _dev(d["in_shift"])
    Ycd = _dev(ref.float())
    for res in (0, 1):
        out = _nan((B, C, H, H))
        _ok(L.ffc_fu2d_c2r_rows(_ptr(Ycd), B, C, H, H, _ptr(t), up, _ptr(isc), _ptr(ish), 1, res, _ptr(out),
                                _stream()), "ffc_fu2d_c2r_rows")
        torch.cuda.synchronize()
        errs.append(_err("fu2d_rows", f"({C},{H}) up={up} res={res}", out, d["out_res"] if res else d["out"]))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("B,C,H,up", [(2, 16, 16, 2), (3, 32, 32, 2), (2, 16, 16, 1), (2, 32, 16, 2)])
def test_fu2d_r2c_mix_matches_fp64(B, C, H, up):
    """the R2C inside mix pass 0 with explicit in_scale / in_shift: slab and raw Y from t"""
    L = _lib()
    assert L.ffc_fu2d_r2c_mix_supported(C, H, H, up)
    d = _fu_case(B, C, H // up, H // up, up, True, True)
    wmixT, _ = _pack_mix(d["wmix"], C, False)
    rows = L.ffc_fu2d_slab_rows(B, C, H, H)
    slab, Y = _nan((rows, 2 * C, 4)), _nan((B, C, H, H // 2 + 1, 2))
    _ok(L.ffc_fu2d_r2c_mix(_ptr(_dev(d["t"])), B, C, H, H, up, _ptr(_dev(d["in_scale"])), _ptr(_dev(d["in_shift"])), 1,
                           None, _ptr(wmixT), _ptr(slab), _ptr(Y), _stream()), "ffc_fu2d_r2c_mix")
    torch.cuda.synchronize()
    what = f"({C},{H}) up={up}"
    e = _err("fu2d_r2c_mix", what, Y, sr.fu2d_Y(d["Y"]))
    _check_slab("fu2d_r2c_mix", what, slab, d["stats"])
    assert e <= TOL


def _f16_bound(d, scale=None):
    """elementwise bound of the fp16 mix in the staged (B, C, H, WP, 2) layout: 1.001 * 2^-10 * (|W| . |Z|)
    (times |scale| behind BN + ReLU), without the 1e-5 * max|ref| term"""
    C2 = d["wmix"].shape[0]
    b = 1.001 * 2.0 ** -10 * torch.einsum("oi,bihw->bohw", d["wmix"].double().abs().reshape(C2, C2), d["Z"].abs())
    if scale is not None:
        b = b * scale.double().abs()[None, :, None, None]
    return sr.fu2d_Y(b)


def _assert_within(family, what, got, ref, bound):
    assert not torch.isnan(got).any(), f"{what}: unwritten (NaN) elements"
    diff = (got.cpu().double().reshape(ref.shape) - ref).abs()
    lim = bound + TOL * ref.abs().max()
    print(f"OBS {family} {what} max diff / limit {(diff / lim).max():.3e}  normwise {diff.max() / ref.abs().max():.3e}")
    assert (diff <= lim).all(), (what, float((diff / lim).max()))


# cols: the case must also reach the f16 ffc_fu2d_mix_cols (H >= 32); C 16 / 32 / 64 each do, H 32 / 64 / 128
@pytest.mark.parametrize("B,C,H,up,cols", [(2, 16, 16, 1, False), (2, 16, 32, 1, True), (2, 32, 32, 2, True),
                                           (1, 64, 32, 1, True), (2, 64, 16, 2, False), (1, 16, 64, 2, True),
                                           (1, 32, 128, 1, True)])
def test_fu2d_mix_f16_within_derived_bound(B, C, H, up, cols):
    L = _lib()
    assert bool(L.ffc_fu2d_cols_supported(C, H, H, up, 1)) == cols
    d = _fu_case(B, C, H // up, H // up, up, True, True)
    T, _ = _mix_ops(d, B, C, H, up)
    Mpad = (2 * C + 31) // 32 * 32
    w16 = torch.zeros((Mpad, 2 * C), device=DEV, dtype=torch.float16)
    _ok(L.ffc_fu_pack_mix_f16(_ptr(_dev(d["wmix"])), 2 * C, _ptr(w16), _stream()), "ffc_fu_pack_mix_f16")
    rows = L.ffc_fu2d_slab_rows(B, C, H, H)
    slab, Y = _nan((rows, 2 * C, 4)), _nan((B, C, H, H // 2 + 1, 2))
    _ok(L.ffc_fu2d_mix_f16(_ptr(T), B, C, H, H, up, _ptr(w16), 0, _ptr(slab), None, None, _ptr(Y), _stream()),
        "ffc_fu2d_mix_f16(pass 0)")
    torch.cuda.synchronize()
    what = f"({C},{H}) up={up}"
    _assert_within("fu2d_f16_mix0", what, Y, sr.fu2d_Y(d["Y"]), _f16_bound(d))
    # the statistics are those of the spilled Y itself: the same numbers
    own = torch.view_as_complex(Y.cpu().double())
    own = torch.stack((own.real, own.imag), dim=2).reshape(B, 2 * C, H, H // 2 + 1)
    _check_slab("fu2d_f16_mix0", what, slab, sr.channel_stats(own))
    Y1 = _nan((B, C, H, H // 2 + 1, 2))
    _ok(L.ffc_fu2d_mix_f16(_ptr(T), B, C, H, H, up, _ptr(w16), 1, None, _ptr(_dev(d["bn_scale"])),
                           _ptr(_dev(d["bn_shift"])), _ptr(Y1), _stream()), "ffc_fu2d_mix_f16(pass 1)")
    torch.cuda.synchronize()
    _assert_within("fu2d_f16_mix1", what, Y1, sr.fu2d_Y(sr.bn_relu(d["Y"], d["bn_scale"], d["bn_shift"])),
                   _f16_bound(d, d["bn_scale"]))
    if cols:
        Yc = _nan((B, C, H // 2 + 1, H, 2))
        _ok(L.ffc_fu2d_mix_cols(_ptr(T), B, C, H, H, up, _ptr(w16), 1, _ptr(_dev(d["bn_scale"])),
                                _ptr(_dev(d["bn_shift"])), _ptr(Yc), _stream()), "ffc_fu2d_mix_cols(f16)")
        torch.cuda.synchronize()
        b = _f16_bound(d, d["bn_scale"])                              # (B, C, H, WP, 2)
        col = (b[..., 0] + b[..., 1]).sum(dim=2)                       # a column FFT sums its column's bounds
        bound = col[:, :, :, None, None].expand(B, C, H // 2 + 1, H, 2)
        _assert_within("fu2d_f16_cols", what, Yc, sr.fu2d_Yc(d["Y"], d["bn_scale"], d["bn_shift"]), bound)


# --------------------------------------------------------------------------- SpectralTransform prologue
def _st_splits(B, Cin, c, H, W, pool):
    h, w = (H // 2, W // 2) if pool else (H, W)
    tiles = ((c + 31) // 32) * ((h * w + 31) // 32)
    s = {1, _lib().ffc_st_prologue_split(B, Cin, H, W, pool, c)}
    s |= {p for p in (2, 4, 8) if tiles % p == 0}
    return sorted(s), tiles


_ST = [(3, 16, 8, 8, 0, 0), (3, 16, 8, 8, 0, 1), (3, 16, 8, 8, 0, 4), (2, 24, 40, 6, 0, 4), (2, 64, 32, 16, 1, 4),
       (3, 17, 5, 5, 0, 0), (3, 17, 5, 5, 0, 1), (4, 32, 8, 4, 1, 0)]


_ST_RUNS = [(*s, ex3) for s in _ST for ex3 in (False, True) if not ex3 or s[1] % 16 == 0]   # ex3: Cin % 16 == 0


@pytest.mark.parametrize("B,Cin,c,H,pool,hidden,ex3", _ST_RUNS)
def test_st_prologue_matches_fp64(B, Cin, c, H, pool, hidden, ex3):
    L = _lib()
    assert L.ffc_st_prologue_lds_bytes(Cin, H, H, pool, hidden, c) > 0
    assert (L.ffc_st_pack_a3_elems(c, Cin) > 0) == (Cin % 16 == 0)
    if (Cin, H) == (17, 5):
        assert (Cin * H * H) % 4 != 0                     # x_dma off
    x, w1, w2, wconv1 = sr.st_inputs(B, Cin, c, H, H, pool, hidden)
    gate_ref, t_ref, stats = sr.st_prologue(x, pool, w1, w2, wconv1)
    h = H // 2 if pool else H
    Mpad = (c + 31) // 32 * 32
    wT = _padded(Cin * Mpad)
    wd = _dev(wconv1)
    _ok(L.ffc_pack_transpose(_ptr(wd), c, Cin, _ptr(wT), _stream()), "ffc_pack_transpose")
    wc3 = None
    if ex3:
        wc3 = torch.zeros(int(L.ffc_st_pack_a3_elems(c, Cin)), device=DEV, dtype=torch.int16)
        _ok(L.ffc_st_pack_a3(_ptr(wd), c, Cin, _ptr(wc3), _stream()), "ffc_st_pack_a3")
    xd, w1d, w2d = _dev(x), _padded(hidden * Cin), _padded(hidden * Cin)
    if hidden:
        w1d[:hidden * Cin] = _dev(w1).reshape(-1)
        w2d[:hidden * Cin] = _dev(w2).reshape(-1)
    splits, tiles = _st_splits(B, Cin, c, H, H, pool)
    errs = []
    for split in splits:
        t, slab, gate = _nan((B, c, h, h)), _nan((B * split, c, 4)), _nan((B, Cin))
        args = (_ptr(xd), B, Cin, H, H, pool, _ptr(w1d) if hidden else None, _ptr(w2d) if hidden else None, hidden,
                _ptr(wT))
        tail = (c, split, _ptr(t), _ptr(slab), _ptr(gate), _stream())
        rc = L.ffc_st_prologue_ex3(*args, _ptr(wc3), *tail) if ex3 else L.ffc_st_prologue_ex(*args, *tail)
        _ok(rc, "ffc_st_prologue")
        torch.cuda.synchronize()
        what = f"({Cin},{c},{H}) pool={pool} hid={hidden} split={split}/{tiles} ex3={int(ex3)}"
        errs += [_err("st_gate", what, gate, gate_ref), _err("st_t", what, t, t_ref)]
        _check_slab("st", what, slab, stats)
        rows = slab.cpu()
        empty = rows[..., 0] == 0
        assert torch.equal(rows[empty][:, :3], torch.zeros_like(rows[empty][:, :3]))   # untouched: exactly {0, 0, 0}
        if (Cin, c, H, split) == (24, 40, 6, 4):
            # M-tile 1 (channels 32..39) belongs to two of the four workgroups: the other two leave them untouched
            assert empty[:, 32:].any() and not empty[:, 32:].all()
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("B,Cin,M,HW,with_gate,with_slab", [(2, 6, 5, 255, 1, 1), (2, 16, 32, 256, 0, 1),
                                                            (2, 7, 48, 257, 1, 0), (1, 8, 128, 4096, 1, 1),
                                                            (3, 13, 128, 257, 0, 1), (2, 6, 5, 4096, 0, 0)])
def test_pw_gate_conv_matches_fp64(B, Cin, M, HW, with_gate, with_slab):
    L = _lib()
    assert L.ffc_pw_gate_lds_bytes(Cin, M) > 0
    gen = torch.Generator().manual_seed(600 + M + HW)
    x = torch.randn(B, Cin, HW, generator=gen) + 0.25
    gate = torch.rand(B, Cin, generator=gen) if with_gate else None
    w = torch.randn(M, Cin, generator=gen) / Cin ** 0.5
    ref = sr.pw_gate_conv(x, gate, w)
    nblk = L.ffc_pw_gate_blocks(HW)
    assert nblk == (HW + 255) // 256
    t = _nan((B, M, HW))
    slab = _nan((B * nblk, M, 4)) if with_slab else None
    _ok(L.ffc_pw_gate_conv(_ptr(_dev(x)), _ptr(_dev(gate)), _ptr(_dev(w)), B, Cin, M, HW, _ptr(t), _ptr(slab),
                           _stream()), "ffc_pw_gate_conv")
    torch.cuda.synchronize()
    what = f"Cin={Cin} M={M} HW={HW} gate={with_gate}"
    e = _err("pw_gate", what, t, ref)
    if with_slab:
        _check_slab("pw_gate", what, slab, sr.channel_stats(ref))
    assert e <= TOL


@pytest.mark.parametrize("B,C,H,W,pool,hidden", [(2, 16, 1, 1, 0, 1), (3, 5, 3, 3, 0, 2), (2, 300, 2, 2, 0, 4),
                                                 (1, 8, 64, 64, 0, 2), (2, 16, 64, 64, 1, 1), (2, 8, 6, 6, 1, 0),
                                                 (2, 12, 16, 16, 1, 3), (2, 300, 8, 8, 0, 0)])
def test_se_gate_matches_fp64(B, C, H, W, pool, hidden):
    gen = torch.Generator().manual_seed(700 + C + H + hidden)
    x = torch.randn(B, C, H, W, generator=gen) + 0.5
    w1, w2 = sr.se_weights(x, pool, hidden, gen)
    gate = _nan((B, C))
    _ok(_lib().ffc_se_gate(_ptr(_dev(x)), B, C, H, W, pool, _ptr(_dev(w1)), _ptr(_dev(w2)), hidden, _ptr(gate),
                           _stream()), "ffc_se_gate")
    torch.cuda.synchronize()
    assert _err("se_gate", f"C={C} {H}x{W} pool={pool} hid={hidden}", gate, sr.se_gate(x, pool, w1, w2)) <= TOL


@pytest.mark.parametrize("B,K,N,N0,with_bias,act", [(1, 3, 70, 70, 1, 0), (33, 100, 260, 128, 1, 2),
                                                    (33, 128, 1024, 1024, 0, 5), (1, 129, 70, 30, 1, 2),
                                                    (33, 256, 260, 260, 1, 0), (33, 100, 66, 66, 0, 0),
                                                    (2, 256, 1024, 512, 1, 5), (1, 100, 260, 260, 1, 2)])
def test_dense_matches_fp64(B, K, N, N0, with_bias, act):
    A, Wt, bias = sr.dense_inputs(B, K, N, bool(with_bias), act)
    ref = sr.dense(A, Wt, bias, act)
    out0 = _nan((B, N0))
    out1 = _nan((B, N - N0)) if N0 < N else None
    _ok(_lib().ffc_dense_forward(_ptr(_dev(A)), _ptr(_dev(Wt)), _ptr(_dev(bias)), B, K, N, N0, _ptr(out0), _ptr(out1),
                                 act, sr.SLOPE, _stream()), "ffc_dense_forward")
    torch.cuda.synchronize()
    what = f"B={B} K={K} N={N} N0={N0} bias={with_bias} act={act}"
    errs = [_err("dense", what + " out0", out0, ref[:, :N0])]
    if out1 is not None:
        errs.append(_err("dense", what + " out1", out1, ref[:, N0:]))
    assert max(errs) <= TOL, errs


def test_dense_rejects_k_above_256():
    """K = 257 is an error status: nothing is launched, the output stays untouched"""
    A, Wt, _ = sr.dense_inputs(2, 257, 8, False, 0)
    out = _nan((2, 8))
    rc = _lib().ffc_dense_forward(_ptr(_dev(A)), _ptr(_dev(Wt)), None, 2, 257, 8, 8, _ptr(out), None, 0, 0.0, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"K > 256" in _lib().ffc_last_error()
    assert torch.isnan(out).all()
