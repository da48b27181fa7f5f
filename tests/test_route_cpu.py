"""rt.conv_route, the one rule that sends a convolution job to a direct kernel ('convT', 'full', 'conv3',
'dense') or to the implicit-GEMM kernels (None), for the inference caller (_FFCExec) and the training
caller (_autograd.conv_forward).

The expected routes of every row under the kernels' channel caps are the answers of the two predicates
this function replaced (the inference executor's small-M and outer-product tests; the training path's
small-M test and the dense test inside conv_forward), taken by running them on these jobs at the commit
before the change.  The rows over a cap expect None: those jobs used to end in the kernels' argument
checks.  The last tests hold the weight-derived packs of both callers to a constant count.
"""
import os
import re

import pytest
import torch

from fastfourierconvolution_amd import _plan
from fastfourierconvolution_amd import _runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = "n/a"   # the training caller has no such job (BatchNorm is an op of its own there)


def ct(C, H=8, W=None):          # ConvTranspose2d k4 s2 p1: (Seg, layout)
    return _plan.Seg("convT", C, H, W or H, 4, 2, 1), 1


def c3(C, H=8, W=None):          # Conv2d k3 s1 p1
    return _plan.Seg("conv", C, H, W or H, 3, 1, 1), 0


def full(C, k=4, lay=0):         # Conv2d k = plane, p0: a 1x1 output
    return _plan.Seg("conv", C, k, k, k, 1, 0), lay


def ct1(C, k=4):                 # ConvTranspose2d k s1 p0 on a 1x1 input
    return _plan.Seg("convT", C, 1, 1, k, 1, 0), 1


# id: (segments, M, bias per segment, addend, bn, switches off, inference route, training route)
JOBS = {
    "convT_M4": ([ct(64)], 4, [0], 0, 0, (), "convT", "convT"),
    "convT_M5": ([ct(64)], 5, [0], 0, 0, (), None, None),
    "convT_2seg": ([ct(32), ct(16)], 3, [0, 0], 0, 0, (), "convT", "convT"),
    "convT_1bias": ([ct(32), ct(16)], 3, [1, 0], 0, 0, (), "convT", "convT"),
    "convT_2bias": ([ct(32), ct(16)], 3, [1, 1], 0, 0, (), None, None),
    "convT_planes": ([ct(32, 8), ct(16, 4)], 3, [0, 0], 0, 0, (), None, None),
    "convT_C256": ([ct(128), ct(128)], 3, [0, 0], 0, 0, (), "convT", "convT"),
    "convT_C257": ([ct(128), ct(129)], 3, [0, 0], 0, 0, (), None, None),
    "convT_1seg_C257": ([ct(257)], 3, [0], 0, 0, (), None, None),
    "convT_addend": ([ct(64)], 3, [0], 1, 0, (), None, None),
    "convT_bn": ([ct(64)], 3, [0], 0, 1, (), None, NA),
    "convT_smallm_off": ([ct(64)], 3, [0], 0, 0, ("USE_SMALLM",), None, None),
    "conv3_M3": ([c3(64)], 3, [0], 0, 0, (), "conv3", None),
    "conv3_M5": ([c3(64)], 5, [0], 0, 0, (), None, None),
    "conv3_2seg_bias": ([c3(48), c3(16)], 3, [0, 1], 0, 0, (), "conv3", None),
    "conv3_2bias": ([c3(48), c3(16)], 3, [1, 1], 0, 0, (), None, None),
    "conv3_planes": ([c3(48, 8), c3(16, 16)], 3, [0, 0], 0, 0, (), None, None),
    "conv3_C256": ([c3(192), c3(64)], 3, [0, 0], 0, 0, (), "conv3", None),
    "conv3_C257": ([c3(192), c3(65)], 3, [0, 0], 0, 0, (), None, None),
    "conv3_IW6": ([c3(64, 8, 6)], 3, [0], 0, 0, (), None, None),
    "conv3_addend": ([c3(64)], 3, [0], 1, 0, (), None, None),
    "conv3_bn": ([c3(64)], 3, [0], 0, 1, (), None, NA),
    "conv3_smallm_off": ([c3(64)], 3, [0], 0, 0, ("USE_SMALLM",), None, None),
    "full_M1": ([full(64), full(64)], 1, [0, 1], 0, 0, (), "full", "full"),
    "full_M5": ([full(64)], 5, [0], 0, 0, (), None, None),
    "full_layout1": ([full(64, lay=1)], 1, [0], 0, 0, (), None, None),
    "full_mixed_layout": ([full(64), full(64, lay=1)], 1, [0, 0], 0, 0, (), None, None),
    "full_planes": ([full(64, 4), full(64, 2)], 1, [0, 0], 0, 0, (), None, "full"),
    "full_2bias": ([full(64), full(64)], 1, [1, 1], 0, 0, (), None, None),
    "full_smallm_off": ([full(64)], 1, [0], 0, 0, ("USE_SMALLM",), None, None),
    "dense_C256": ([ct1(256)], 64, [0], 0, 0, (), "dense", "dense"),
    "dense_C257": ([ct1(257)], 64, [0], 0, 0, (), None, None),
    "dense_C256_bias": ([ct1(256)], 64, [1], 0, 0, (), "dense", None),
    "dense_C257_bias": ([ct1(257)], 64, [1], 0, 0, (), None, None),
    "dense_2seg": ([ct1(100), ct1(28)], 64, [0, 0], 0, 0, (), None, None),
    "dense_M3": ([ct1(100)], 3, [0], 0, 0, (), "dense", "dense"),
    "dense_addend": ([ct1(100)], 64, [0], 1, 0, (), None, None),
    "dense_bn": ([ct1(100)], 64, [0], 0, 1, (), None, NA),
    "dense_outer_off": ([ct1(100)], 64, [0], 0, 0, ("USE_OUTER",), None, "dense"),
    "dense_smallm_off": ([ct1(100)], 64, [0], 0, 0, ("USE_SMALLM",), "dense", "dense"),
}


def job_weights(segs, M, biases):
    """ConvWeight per (Seg, layout): weight of the module's shape, bias where flagged (CPU tensors)"""
    out = []
    for (sg, lay), b in zip(segs, biases):
        shape = (sg.C, M, sg.k, sg.k) if lay == 1 else (M, sg.C, sg.k, sg.k)
        out.append(rt.ConvWeight(torch.zeros(shape), lay, sg.k, sg.k, torch.zeros(M) if b else None))
    return out


@pytest.mark.parametrize("name", list(JOBS))
def test_route_table(name, monkeypatch):
    segs, M, biases, addend, bn, off, want_inf, want_train = JOBS[name]
    for knob in off:
        monkeypatch.setattr(rt, knob, False)
    sgs = [sg for sg, _ in segs]
    w = job_weights(segs, M, biases)
    assert rt.conv_route(sgs, w, M, bool(addend), bool(bn), rt.INFER_ROUTES) == want_inf
    if want_train != NA:
        assert rt.conv_route(sgs, w, M, bool(addend), bool(bn), rt.TRAIN_ROUTES, training=True) == want_train


def test_route_accepts_only_what_the_caller_takes():
    (sg, lay), = [c3(64)]
    w = job_weights([(sg, lay)], 3, [0])
    assert rt.conv_route([sg], w, 3, False, False, frozenset(("conv3",))) == "conv3"
    assert rt.conv_route([sg], w, 3, False, False, frozenset(("convT", "full"))) is None


def test_router_caps_are_the_kernels():
    """the router's caps against the constants the kernels' argument checks use"""
    def const(path, name):
        with open(os.path.join(ROOT, "fastfourierconvolution_amd", "csrc", path)) as f:
            m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", f.read())
        assert m is not None, f"{name} not found in {path}"
        return int(m.group(1))
    assert rt.RouteCaps.CONVT_SMALLM_CMAX == const("convt_smallm.hip", "CT_CMAX")
    assert rt.RouteCaps.CONV3_SMALLM_CMAX == const("convt_smallm.hip", "CMAX3")
    assert rt.RouteCaps.DENSE_KMAX == const("dense.hip", "DN_KMAX")


def test_pack_cache_replaces_in_place():
    """a source at a new version re-builds into its slot; a fresh tensor each step needs a named slot"""
    packs, built = rt.PackCache(8), []
    w = torch.zeros(4, 4)
    for step in range(5):
        w.add_(1.0)                                     # an optimizer step: same tensor, new version
        for _ in range(2):
            assert packs.get("t", [w, None], lambda: built.append(step) or step) == step
        assert len(packs.d) == 1
    assert built == [0, 1, 2, 3, 4]
    keep = []
    for step in range(5):
        keep.append(torch.zeros(4, 4))                  # W / sigma: a new tensor at a new address every step
        assert packs.get("sn", [keep[-1]], lambda: step, slot=("job", 0)) == step
        assert len(packs.d) == 2


def test_outer_and_dense_packs_stay_constant_when_weights_change(monkeypatch):
    """the inference executor's ConvT-on-1x1 chain (outer-product form, then the dense launch's concatenated
    matrix) over weight updates: one pack per weight and one per launch, however often the weights change"""
    from fastfourierconvolution_amd.ffc.ffc import Branch, _FFCExec

    class Exec(_FFCExec):
        pass
    launches = []
    monkeypatch.setattr(rt, "dense_forward", lambda x, Wt, bias, *a: launches.append((Wt, bias)))
    ex, B, C, M, k = Exec(), 2, 12, 8, 4
    sg = _plan.Seg("convT", C, 1, 1, k, 1, 0)
    x = torch.zeros(B, C, 1, 1)
    ws = [rt.ConvWeight(torch.randn(C, M, k, k), 1, k, k, b) for b in (None, torch.randn(M))]
    for step in range(6):
        for w in ws:
            w.w.mul_(0.5)                               # new version, same tensor
        branches = [Branch(n, [sg], [w], [x], [], (0, 0.0), None, M) for n, w in zip("lg", ws)]
        outs = {}
        ex._plan_branches(branches, ["dense", "dense"], B, x.device, 0, outs)
        Wt, bias = launches[-1]                         # both branches in one launch, built from the new weights
        assert len(launches) == step + 1 and tuple(Wt.shape) == (C, 2 * M * k * k)
        assert torch.equal(Wt[:, :M * k * k], ws[0].w.reshape(C, -1))
        assert torch.equal(bias[M * k * k:], ws[1].bias.repeat_interleave(k * k))
        tags = sorted(slot[0] for slot in rt.packs_of(ex._ffc_cache()).d)
        assert tags == ["dense", "outer", "outer"], (step, tags)


def test_training_convt_pack_is_one_per_job_under_fresh_weights(monkeypatch):
    """_autograd.conv_forward's small-M ConvT job when the weight is a new tensor every step (W / sigma
    under spectral norm): the packed weights are re-made each step into the job's one slot"""
    from fastfourierconvolution_amd import _autograd as ag
    calls = []

    class FakeLib:
        def __getattr__(self, name):
            return lambda *a: calls.append(name) or 0
    monkeypatch.setattr(rt, "lib", lambda: FakeLib())
    monkeypatch.setattr(ag, "_stream", lambda t: 0)
    (sg, lay), B, M = ct(16), 2, 3
    cache, keep = {}, []
    for step in range(5):
        keep.append(torch.zeros(sg.C, M, 4, 4))
        out = ag.conv_forward(cache, ("fwd", "spec", 0), B, M, (sg,), [rt.ConvWeight(keep[-1], lay, 4, 4, None)],
                              [torch.zeros(B, sg.C, sg.IH, sg.IW)])
        assert tuple(out.shape) == (B, M, 2 * sg.IH, 2 * sg.IW)
        assert calls.count("ffc_convt_smallm_pack") == step + 1 == calls.count("ffc_convt_k4s2_smallm")
        assert len(rt.packs_of(cache).d) == 1
