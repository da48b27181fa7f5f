"""Host-side checks for the mg = 6 models (48x48 images): the conv planner on their conv jobs (emulated
with the kernel's index math against torch in fp64, as tests/test_plan_cpu.py does), the state_dict keys
of FGenerator32 / Discriminator32 / FDiscriminator32 against the key lists recorded from the reference
classes (tests/golden/manifest_fgan48.json), the exported names, and the fused Fourier unit's LDS query
for the two planes the generator needs.  No GPU."""
import contextlib
import io
import json
import os

import pytest
import torch

import test_plan_cpu as P
from conftest import GOLDEN
from fastfourierconvolution_amd import _plan

S = _plan.Seg
# job -> (M of the models, segments at the models' sizes): FGenerator32 conv2..conv5 local / global branches,
# the critics' convs at 48, 24, 12 (6 is the fc's input)
JOBS = {
    "g_conv2_l_6to12": (192, [S("convT", 512, 6, 6, 4, 2, 1)]),
    "g_conv3_l_12to24": (96, [S("convT", 192, 12, 12, 4, 2, 1), S("convT", 64, 12, 12, 4, 2, 1)]),
    "g_conv3_g_12to24": (32, [S("convT", 192, 12, 12, 4, 2, 1), S("pw", 16, 24, 24)]),
    "g_conv4_l_24to48": (48, [S("convT", 96, 24, 24, 4, 2, 1), S("convT", 32, 24, 24, 4, 2, 1)]),
    "g_conv4_g_24to48": (16, [S("convT", 96, 24, 24, 4, 2, 1), S("pw", 8, 48, 48)]),
    "g_head_48": (3, [S("conv", 48, 48, 48, 3, 1, 1), S("conv", 16, 48, 48, 3, 1, 1)]),
    "d_conv1_48": (64, [S("conv", 3, 48, 48, 3, 1, 1)]),
    "d_conv2_48to24": (64, [S("conv", 64, 48, 48, 4, 2, 1)]),
    "d_conv3_24": (128, [S("conv", 64, 24, 24, 3, 1, 1)]),
    "d_conv4_24to12": (128, [S("conv", 128, 24, 24, 4, 2, 1)]),
    "d_conv5_12": (256, [S("conv", 128, 12, 12, 3, 1, 1)]),
    "d_conv6_12to6": (256, [S("conv", 256, 12, 12, 4, 2, 1)]),
    "d_conv7_6": (512, [S("conv", 256, 6, 6, 3, 1, 1)]),
    "fd_main1_48to24": (128, [S("conv", 64, 48, 48, 4, 2, 1)]),
    "fd_main3_12to6": (512, [S("conv", 256, 12, 12, 4, 2, 1)]),
}


@pytest.mark.parametrize("name", sorted(JOBS))
def test_mg6_job_plans(name):
    """the job plans at the models' channel counts (B = 64), and computes torch's result at the same
    spatial sizes with the channels cut to at most 3 per segment and M = 5"""
    M, segs = JOBS[name]
    plan = _plan.plan_job(64, M, segs)
    oh = {"convT": lambda s: 2 * s.IH, "pw": lambda s: s.IH}.get(segs[0].kind, lambda s: s.IH // segs[0].s)(segs[0])
    assert (plan.OH, plan.OW) == (oh, oh)
    for pi, ph in enumerate(plan.phases):
        assert ph.Kpad % _plan.BK == 0 and ph.Kpad >= ph.K
    tiles, nslots = _plan.build_tiles([plan], _plan.pick_tile_cfg([M]))
    assert len(tiles) > 0
    small = [S(s.kind, min(s.C, 3), s.IH, s.IW, s.k, s.s, s.p) if s.kind != "pw" else S("pw", min(s.C, 3), s.IH, s.IW)
             for s in segs]
    gen = torch.Generator().manual_seed(3)
    sp = _plan.plan_job(2, 5, small)
    xs, ws, lays, ref = [], [], [], 0
    for sg in small:
        x, w, lay = P.make(sg, 2, 5, gen)
        xs.append(x)
        ws.append(w)
        lays.append(lay)
        ref = ref + P.ref_out(sg, x, w)
    got = P.emulate(sp, xs, ws, lays)
    assert got.shape == ref.shape and torch.allclose(got, ref, atol=1e-10, rtol=1e-10)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.parametrize("kind,ctor", [("FGenerator32", dict(z_size=16, mg=6)), ("Discriminator32", dict(sn=True, mg=6)),
                                       ("FDiscriminator32", dict(sn=True, mg=6))])
def test_state_dict_keys_are_the_references(kind, ctor):
    import fastfourierconvolution_amd as F
    with open(os.path.join(GOLDEN, "manifest_fgan48.json")) as f:
        man = json.load(f)
    mod = _quiet(getattr(F, kind), **ctor)
    assert list(mod.state_dict()) == man["state_dict_keys"][kind]
    case = next(c for c in man["cases"] if c["kind"] == kind)
    for k, v in mod.state_dict().items():
        assert list(v.shape) == case["specs"][k][0], k
    assert mod.mg == 6 and _quiet(getattr(F, kind), *(([16]) if kind == "FGenerator32" else [])).mg == 4


def test_family_attributes_and_exports():
    import fastfourierconvolution_amd as F
    for n in ("FGenerator32", "Discriminator32", "FDiscriminator32", "GaussianNoise"):
        assert n in F.__all__ and hasattr(F, n)
    fd = _quiet(F.FDiscriminator32)
    assert isinstance(fd.gaus_noise, F.GaussianNoise) and fd.gaus_noise.stddev == 0.05
    g = _quiet(F.FGenerator32, 8)
    assert g.ngf == 64 and g.z_size == 8 and not g.conv2.uses_sn and hasattr(g, "conv5") and not hasattr(g, "conv6")
    d = F.Discriminator32(sn=False)
    assert not hasattr(d, "last_act") and not hasattr(d, "conv8") and list(d.state_dict())[0] == "conv1.weight"
    x = torch.randn(2, 3, 4, 4)
    gn = F.GaussianNoise(0.05).eval()
    assert gn(x) is x                                 # identity in eval mode (layers/gaussian_noise.py:11-15)
    # the fgan128 classes keep their layers
    assert hasattr(_quiet(F.FGenerator, 8), "conv7")


def test_fused_fu_serves_the_generator_planes():
    """ffc_fu_lds_bytes > 0 for (16, 24, 24) and (8, 48, 48): both run the fused kernel"""
    from fastfourierconvolution_amd import _lib
    L = _lib.load()
    assert 0 < L.ffc_fu_lds_bytes(16, 24, 24) <= 160 * 1024
    assert 0 < L.ffc_fu_lds_bytes(8, 48, 48) <= 160 * 1024
    assert L.ffc_fu_supported(16, 24, 24, 2) == 1 and L.ffc_fu_supported(8, 48, 48, 2) == 1
    for H in (24, 48):
        assert L.ffc_fu_kgroups(256, 8, H, H) == 1
    assert L.ffc_fu_supported(8, 24, 24, 1) == 1
    assert L.ffc_fu_supported(8, 48, 48, 1) == 0       # 48 x 48 exists as a x2-upsampled output only
    assert L.ffc_fu_supported(16, 32, 32, 1) == 1 and L.ffc_fu_supported(16, 32, 32, 2) == 1
    assert L.ffc_fu_supported(16, 32, 32, 3) == 0 and L.ffc_fu_supported(16, 64, 64, 1) == 0
    # planes no instance exists for
    for hw in ((6, 6), (12, 12), (96, 96), (24, 48)):
        assert L.ffc_fu_lds_bytes(8, *hw) == 0 and L.ffc_fu_supported(8, *hw, 2) == 0
