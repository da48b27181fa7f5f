"""Kernel-level parity of the fused Fourier unit (csrc/fu_kernels.hip) on the 3 * 2^k planes of the
mg = 6 models -- square 24 at up 1 and 2 and square 48 at up = 2, whose row and column FFTs run one radix-3 stage under the
radix-2 stages (csrc/fft_reg.h) -- through the C ABI against the float64 references of
tests/spectral_refs.py.  Harness, bounds and checks are those of tests/test_gpu_spectral_kernels.py
(imported): outputs, spills and slabs prefilled with NaN and NaN-free afterwards, 1e-5 normwise,
slab statistics at rtol 1e-5 / atol 1e-6; spectral_refs.fu_case keeps every ReLU pre-activation away
from 0.  Every case runs pass 0 with a spill, pass 1 from the spill and pass 1 recomputing.

12 x 12 planes and up = 1 on the 48 plane are not built: tests/test_abi_cpu.py,
tests/native/abi_sanitize.cpp and tests/test_gpu_parity.py pin that the library refuses a 12 x 12 plane
and that FourierUnitSN refuses a direct (up = 1) 48 x 48 input.  The refusals are checked here too.

Case (C, H = W) -> branch it is there for
  (1, 24)   B 1: 2C = 2, one partly filled M-tile, NB = 312 (ten bin tiles, the last of 24 bins);
            the full cross up {1, 2} x residual x affine x ReLU (up 1: 24-float rows, up 2: 12-float rows)
  (3, 24)   up 1: odd C, no wmix3
  (8, 24)   up 1: split-bf16 mix; (16, 24) up 2: the model's conv3 shape
  (8, 48)   up 2: the model's conv4 shape, 155 840 B of LDS (the 160 KiB edge), statistics scratch in the
            Y-imaginary plane, NB = 1200
  (5, 48)   up 2, B 3: ragged M-tile and bin tiles, scratch behind the planes
  fold      in_fold + mix_fold at (8, 24) up 2
  repeat    five fresh forwards of (2, 8, 48) up 2 return identical bytes
The split pass 1, the bin-group pass 0 and the lane-shuffle columns do not exist for these planes:
the library's queries must say so.

Observed maxima on the first MI355X run (normwise, bound 1e-5 each; statistics as max |mean - ref| /
max relative variance error; 30 tests in 2.4 s):
  spill 1.4e-07  out 1.5e-07  stats 1.4e-08 / 2.6e-07
  folds: scale / shift / running statistics 1.3e-07  spill 9.0e-08  out 1.2e-07  stats 6.0e-09 / 2.4e-07
"""
import pytest
import torch

import spectral_refs as sr
import test_gpu_spectral_kernels as K

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    torch.cuda.synchronize()
    K._LIVE.clear()


@pytest.mark.parametrize("up,residual,affine,relu", K._CROSS)
def test_fu24_smallest_full_cross(up, residual, affine, relu):
    K._assert_fu_branch(1, 24, 24, True, None, False)
    K._fu_check(1, 1, 24 // up, 24 // up, up, bool(affine), bool(relu), bool(residual), "f32", family="fu3")


# (C, H): B, up, weight in LDS (f32), weight in LDS (split; None: no wmix3), scratch in Y-imaginary
_SHAPES = {
    (3, 24): (2, 1, True, None, False),
    (8, 24): (2, 1, True, True, False),
    (16, 24): (2, 2, True, True, False),
    (8, 48): (2, 2, True, True, True),
    (5, 48): (3, 2, True, None, False),
}
_RUNS = [(k, v) for k, s in _SHAPES.items() for v in (("f32", "split") if s[3] is not None else ("f32",))]


@pytest.mark.parametrize("shape,variant", _RUNS, ids=[f"{k[0]}x{k[1]}x{k[1]}-{v}" for k, v in _RUNS])
def test_fu_mixed_shapes_match_fp64(shape, variant):
    C, H = shape
    B, up, wm_f32, wm_split, in_y = _SHAPES[shape]
    K._assert_fu_branch(C, H, H, wm_f32, wm_split, in_y)
    assert not K._split_pass1(C, H, H)
    K._fu_check(B, C, H // up, H // up, up, True, True, True, variant, family="fu3")


def test_fu_mixed_lds_edge():
    """(8, 48, 48): four planes of 8 * 48 * 25 floats = 153 600 B, + mix weight + BN region <= 160 KiB in
    both weight forms; one more channel pair does not fit"""
    L = K._lib()
    assert L.ffc_fu_lds_bytes(8, 48, 48) == 4 * (4 * 9600 + 512 + 48) == 155840
    assert K._fu_layout(8, 48, 48, True)[0] == 4 * (4 * 9600 + 768 + 48) <= K.LDS_MAX
    assert L.ffc_fu_lds_bytes(9, 48, 48) == 0


def _refused(C, H, W, up, kgroups, what):
    """ffc_fu_forward_ex4 pass 0 with valid buffers must fail, name the reason and launch nothing"""
    L = K._lib()
    d = K._fu_case(2, C, H // up, W // up, up, True, True)
    wmixT, w3 = K._pack_mix(d["wmix"], C, True)
    t = K._dev(d["t"])
    slab, spill = K._nan((4, 2 * C, 4)), K._nan((2, 2 * C, H, W // 2 + 1))
    rc = L.ffc_fu_forward_ex4(K._ptr(t), 2, C, H, W, up, None, None, 1, K._ptr(wmixT), K._ptr(w3), 0, K._ptr(slab),
                              None, None, 0, None, None, None, K._ptr(spill), kgroups, K._stream())
    assert rc != 0 and what in L.ffc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(slab).all() and torch.isnan(spill).all()


@pytest.mark.parametrize("H", [24, 48])
def test_fu_mixed_variants_are_refused(H):
    """no bin-group pass 0 for these planes (whatever FFC_FU_KGROUPS says), no up = 1 at 48, no non-square mixes"""
    L = K._lib()
    for C in (8, 16):
        assert L.ffc_fu_kgroups(64, C, H, H) == 1
        assert L.ffc_fu_slab_rows(64, C, H, H, 1) == 64
    assert L.ffc_fu_supported(8, H, H, 2) == 1 and L.ffc_fu_supported(8, H, H, 1) == (H == 24)
    assert L.ffc_fu_lds_bytes(8, H, 2 * H) == 0 and L.ffc_fu_lds_bytes(8, H, 16) == 0
    _refused(8, H, H, 2, 2, b"kgroups")
    _refused(8, H, H, 1, 2, b"kgroups")
    if H == 48:
        _refused(8, H, H, 1, 1, b"unsupported")


def test_fu12_is_refused():
    """12 x 12 stays outside the fused kernel (pinned by tests/test_abi_cpu.py)"""
    L = K._lib()
    assert L.ffc_fu_lds_bytes(8, 12, 12) == 0 and L.ffc_fu_supported(8, 12, 12, 2) == 0
    _refused(8, 12, 12, 2, 1, b"unsupported")


def test_fu_mixed_folds_match_fp64():
    """in_fold on pass 0 and mix_fold on pass 1 inside fu_kernel at (8, 24, 24) up 2 (the planes hold the
    fold scratch; no split pass 1): the fold test of test_gpu_spectral_kernels.py at this shape"""
    K.test_fu_folds_match_fp64(8, 12, 12, 2, 2, 0.1)


def test_fu48_bitwise_repeat():
    """five fresh forwards (pass 0 with spill, pass 1 from it) of (2, 8, 48, 48) up 2: identical bytes"""
    d = K._fu_case(2, 8, 24, 24, 2, True, True)
    wmixT, w3 = K._pack_mix(d["wmix"], 8, True)
    t, isc, ish = K._dev(d["t"]), K._dev(d["in_scale"]), K._dev(d["in_shift"])
    runs = []
    for _ in range(5):
        slab, spill = K._fu_launch(d, t, 2, True, True, wmixT, w3, True, in_scale=isc, in_shift=ish)
        out = K._fu_launch(d, t, 2, True, True, wmixT, w3, True, yspill_in=spill, in_scale=isc, in_shift=ish)
        assert not torch.isnan(out).any() and not torch.isnan(slab).any()
        runs.append((slab.cpu(), spill.cpu(), out.cpu()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    assert K.normwise_err(runs[0][2].double(), d["out_res"]) <= K.TOL
