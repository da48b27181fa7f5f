"""tests/convlayer_refs.py without a GPU:
1. every case takes the branch it is there for, from shapes alone: adjoint_seg(...).op, whether _plan.plan_job
   raises on the joined adjoint segments of a fan-out input, rt.conv_route's answer on the training path (and
   _is_convt3_job for the data gradient of the 'convT3' head);
2. the host's backward mirrored in float64 (convlayer_refs.mirror_backward: conv_refs.conv_job_ref over adjoint_seg
   with the layout flipped to 1 - layout, chained through the addend where plan_job refuses; wgrad in conv_wgrad's
   operand order) equals autograd's dx / dW / db to fp64 round-off;
3. float32 CPU torch on the same graph stays within a quarter of every bound at TOL and not at TOL / 10, and no
   ReLU / LeakyReLU pre-activation lies within its forward bound of zero;
4. six planted defects each exceed the bound on at least one case.
"""
import pytest
import torch

import convlayer_refs as clr
from fastfourierconvolution_amd import _autograd as ag
from fastfourierconvolution_amd import _plan
from fastfourierconvolution_amd import _runtime as rt

NAMES = list(clr.CASES)
F64_RTOL = 1e-12    # float64 round-off of sums of <= 10^4 O(1) terms, relative to the magnitude (bound / TOL)


def _segs(case):
    return [ag._edge_seg(ed, torch.empty((case.B,) + case.inputs[ed[1]], device="meta")) for ed in case.edges]


def _weights(case, es):
    """ConvWeight per edge of ``es``, shapes only (conv_route looks at layout and whether a bias is there)"""
    return [rt.ConvWeight(torch.empty(clr.w_shape(case, e), device="meta"), case.edges[e][8], case.edges[e][3],
                          case.edges[e][3], torch.empty(0, device="meta") if case.edges[e][9] >= 0 else None)
            for e in es]


def _adjoints(case, i):
    """[(edge, adjoint segment)] of input i, as conv_layer_backward_impl builds them"""
    segs, out = _segs(case), []
    for e, ed in enumerate(case.edges):
        if ed[1] == i:
            OH, OW = clr.out_hw(ed, *case.inputs[i][1:])
            out.append((e, ag.adjoint_seg(segs[e], case.outs[ed[0]][0], OH, OW)))
    return out


def test_case_table_covers_the_issue():
    assert set(NAMES) == {"c3", "c3s2_even", "c4s2_odd", "cdil", "ct3seg", "dense", "dense_bias", "fan_share",
                          "fan_stride", "fan_mix", "addend_a0", "addend_a1", "shortcut", "headT", "full", "full2",
                          "headT3"}
    assert all(c.B in (2, 3) for c in clr.CASES.values())
    assert len({c.seed for c in clr.CASES.values()}) == len(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_spec_is_the_packages(name):
    c = clr.CASES[name]
    edges = [(ed[0], ed[1], sg, ed[8], ed[9]) for ed, sg in zip(c.edges, _segs(c))]
    assert clr.spec_of(c) == ag.conv_spec(c.outs, edges, c.adds)
    outs_s, parsed = ag.parse_conv_spec(clr.spec_of(c))
    assert parsed == list(c.edges) and outs_s == [tuple(o) for o in c.outs]
    assert ag.parse_conv_adds(clr.spec_of(c)) == dict(c.adds)
    data = clr.inputs(name)
    for j, (M, _, _) in enumerate(c.outs):   # every edge of an output (and its addend) agrees on the output's shape
        for ed in c.edges:
            if ed[0] == j:
                assert tuple(ag.conv_layer_out_shape(ed, data.xs[ed[1]], M)) == tuple(data.gouts[j].shape)


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_its_branch(name):
    c = clr.CASES[name]
    segs = _segs(c)
    for i in range(len(c.inputs)):
        if i in {a[1] for a in c.adds}:
            assert not any(ed[1] == i for ed in c.edges) and c.chained[i] is None
            continue
        adj = _adjoints(c, i)
        for e, a in adj:
            if c.edges[e][2] == "conv":
                assert a.kind == "convT" and a.op == c.ops[e], (name, e, a)
            else:
                assert c.ops[e] is None and a.kind == ("conv" if c.edges[e][2] == "convT" else "pw")
        if len(adj) < 2:
            assert c.chained[i] is None
            continue
        try:
            _plan.plan_job(c.B, c.inputs[i][0], tuple(a for _, a in adj))
            raised = False
        except ValueError:
            raised = True
        assert raised == c.chained[i], (name, i)
    adds = dict(c.adds)
    for j, (M, _, _) in enumerate(c.outs):
        es = [e for e, ed in enumerate(c.edges) if ed[0] == j]
        route = rt.conv_route(tuple(segs[e] for e in es), _weights(c, es), M, j in adds, False, rt.TRAIN_ROUTES,
                              training=True)
        assert route == c.routes[j], (name, j, route)


def test_branches_named_in_the_table():
    """the facts the one-line branch descriptions lean on, beyond ops / chained / routes"""
    C = clr.CASES
    assert [a.s for _, a in _adjoints(C["fan_stride"], 0)] == [1, 2]
    assert [a.kind for _, a in _adjoints(C["fan_mix"], 0)] == ["conv", "convT"]
    assert [(a.kind, a.s) for i in range(3) for _, a in _adjoints(C["ct3seg"], i)] == \
        [("conv", 2), ("conv", 2), ("pw", 1)]
    assert _adjoints(C["cdil"], 0)[0][1].d == 2
    # the small-M switch moves headT / full / full2 / headT3 to the implicit GEMM; 'dense' does not look at it
    prev = rt.USE_SMALLM
    try:
        rt.USE_SMALLM = False
        for name in clr.SMALLM_CASES:
            c, segs = C[name], _segs(C[name])
            es = list(range(len(c.edges)))
            route = rt.conv_route(tuple(segs), _weights(c, es), c.outs[0][0], False, False, rt.TRAIN_ROUTES, training=True)
            assert route == ("dense" if name == "dense" else None)
    finally:
        rt.USE_SMALLM = prev
    c = C["dense"]
    assert rt.conv_route(tuple(_segs(c)), _weights(c, [0]), 70, False, False, rt.TRAIN_ROUTES - {"dense"},
                         training=True) is None
    # headT3's data gradient runs on the direct kernel; headT's adjoints (M 9 / 8) on the implicit GEMM
    c = C["headT3"]
    x = torch.empty((c.B,) + c.inputs[0], device="meta")
    w = [torch.empty(clr.w_shape(c, 0), device="meta")]
    assert ag._is_convt3_job([tuple(o) for o in c.outs], list(c.edges), 0, x, w)
    c = C["headT"]
    for i in range(2):
        (e, a), = _adjoints(c, i)
        wt = [rt.ConvWeight(torch.empty(clr.w_shape(c, e), device="meta"), 0, 4, 4, None)]
        assert rt.conv_route((a,), wt, c.inputs[i][0], False, False, rt.TRAIN_ROUTES, training=True) is None
    # the critic head's adjoint (ConvT k4 s1 p0 on the 1x1 gradient, no bias) is a 'dense' job
    c = C["full"]
    (e, a), = _adjoints(c, 0)
    wt = [rt.ConvWeight(torch.empty(clr.w_shape(c, e), device="meta"), 1, 4, 4, None)]
    assert rt.conv_route((a,), wt, 7, False, False, rt.TRAIN_ROUTES, training=True) == "dense"


def test_adjoint_seg_refusals():
    for kw in (dict(pool=True), dict(gate=True)):
        with pytest.raises(NotImplementedError):
            ag.adjoint_seg(_plan.Seg("pw", 6, 4, 4, **kw), 8, 4, 4)
    with pytest.raises(NotImplementedError):   # k3 s3 p0 on 8x8 -> 2x2 would need output_padding 2 on a 7-high plane
        ag.adjoint_seg(_plan.Seg("conv", 3, 8, 7, 3, 3, 0), 4, 2, 2)


@pytest.mark.parametrize("name", NAMES)
def test_mirror_equals_autograd_in_fp64(name):
    c, data = clr.CASES[name], clr.inputs(name)
    ref, bnd = clr.reference(name)
    dx, dW, db, chained = clr.mirror_backward(c, data, ref.g_pre, _plan.Seg, ag.adjoint_seg, _plan.plan_job)
    assert tuple(chained) == c.chained
    for fam, got, want, lim in (("dx", dx, ref.dx, bnd.dx), ("dW", dW, ref.dW, bnd.dW), ("db", db, ref.db, bnd.db)):
        for k, (g, r, b) in enumerate(zip(got, want, lim)):
            assert g.shape == r.shape
            worst = clr.share(g, r, b) * clr.TOL
            assert worst <= F64_RTOL, (name, fam, k, worst)


def _f32_shares(tol):
    """worst share per family of float32 CPU torch, on one thread and on the default thread count"""
    worst = {}
    default = torch.get_num_threads()
    try:
        for threads in sorted({1, default}):
            torch.set_num_threads(threads)
            for name in NAMES:
                c, data = clr.CASES[name], clr.inputs(name)
                ref, _ = clr.reference(name)
                bnd = clr.bounds(c, data, ref, tol)
                for (fam, lab), s in clr.shares(c, clr.graph(c, data, torch.float32), ref, bnd).items():
                    if s > worst.get(fam, (0.0,))[0]:
                        worst[fam] = (s, name, f"{lab}, {threads} thread(s)")
    finally:
        torch.set_num_threads(default)
    return worst


def test_tol_rule():
    """TOL is the smallest power of ten at which fp32 CPU torch stays within a quarter of every bound"""
    at, tenth = _f32_shares(clr.TOL), _f32_shares(clr.TOL / 10)
    for fam in clr.FAMILIES:
        print(f"OBS fp32-torch share {fam}: {at[fam][0]:.3f} ({at[fam][1]} {at[fam][2]}) at TOL, "
              f"{tenth[fam][0]:.3f} ({tenth[fam][1]} {tenth[fam][2]}) at TOL / 10")
    assert max(v[0] for v in at.values()) <= clr.ROOM
    assert max(v[0] for v in tenth.values()) > clr.ROOM, "TOL is not the smallest power of ten"


@pytest.mark.parametrize("name", NAMES)
def test_no_kink_within_the_forward_bound(name):
    c = clr.CASES[name]
    ref, bnd = clr.reference(name)
    m = clr.kink_margin(c, ref, bnd)
    print(f"OBS kink margin {name}: {m:.3g}")
    assert m > 1.0


# --------------------------------------------------------------------------- planted defects
def _mirror_shares(name, defect):
    c, data = clr.CASES[name], clr.inputs(name)
    ref, bnd = clr.reference(name)
    dx, dW, db, _ = clr.mirror_backward(c, data, ref.g_pre, _plan.Seg, ag.adjoint_seg, _plan.plan_job, defect=defect)
    got = clr.Result(ref.outs, ref.pres, ref.g_pre, dx, dW, db)
    return clr.shares(c, got, ref, bnd)


@pytest.mark.parametrize("defect,name,hit", [
    ("op", "c3s2_even", ("dx", "dx0")),
    ("op", "c4s2_odd", ("dx", "dx0")),
    ("wgrad_swap", "ct3seg", ("dW", "dW0")),
    ("wgrad_swap", "headT", ("dW", "dW1")),
    ("addend", "addend_a0", ("dx", "dx1")),
    ("addend", "addend_a1", ("dx", "dx1")),
    ("db_post", "c3", ("db", "db0")),
    ("db_post", "headT", ("db", "db0")),
    ("chain", "fan_stride", ("dx", "dx0")),
    ("chain", "fan_mix", ("dx", "dx0")),
])
def test_planted_defect_exceeds_the_bound(defect, name, hit):
    s = _mirror_shares(name, defect)
    assert s[hit] > 1.0, (defect, name, s[hit])
    assert all(v <= F64_RTOL / clr.TOL for k, v in s.items() if k[0] != hit[0]), "the defect touched another family"


def test_op_defect_leaves_the_last_row_and_column_zero():
    c, data = clr.CASES["c3s2_even"], clr.inputs("c3s2_even")
    ref, _ = clr.reference("c3s2_even")
    dx, *_ = clr.mirror_backward(c, data, ref.g_pre, _plan.Seg, ag.adjoint_seg, _plan.plan_job, defect="op")
    assert not dx[0][:, :, -1, :].any() and not dx[0][:, :, :, -1].any()
    assert torch.allclose(dx[0][:, :, :-1, :-1], ref.dx[0][:, :, :-1, :-1], rtol=0, atol=1e-12)


def test_gelu_backward_from_the_output_exceeds_the_bound():
    c, data = clr.CASES["fan_share"], clr.inputs("fan_share")
    ref, bnd = clr.reference("fan_share")
    s = clr.shares(c, clr.graph(c, data, gelu_from_output=True), ref, bnd)
    assert s[("dx", "dx0")] > 1.0 and s[("dW", "dW0")] > 1.0 and s[("db", "db0")] > 1.0, s
    assert s[("dW", "dW1")] == 0.0 and s[("forward", "out0")] == 0.0
