"""torch.ops.ffc.conv_layer and torch.ops.ffc.conv_layer_backward on the GPU against the float64 reference and the
per-element bounds of tests/convlayer_refs.py (cases, bound and TOL are explained and checked without a GPU there and
in test_convlayer_refs_cpu.py): every host branch of _autograd.conv_layer_impl / conv_layer_backward_impl that
composes the kernels, which test_gpu_conv_kernels.py, test_gpu_train_kernels.py and test_gpu_convt3_kernels.py test
one by one through the C ABI.

  every case        forward + backward through the op with requires_grad inputs, weights and biases and random
                    cotangents; every returned tensor (outputs, appended GELU pre-activations, dx, dW, db) element
                    by element, nothing excluded
  dead outputs      conv_layer_backward with gouts [None, g] / [g, None] (fan_share) and [None] (shortcut)
  needs             every single entry false in turn: an empty slot, the others bit-equal to the all-true call
  refusals          addend that feeds an edge, addend of the wrong shape, pooled / gated adjoint: nothing launched
  routes            headT / full / full2 / headT3 with rt.USE_SMALLM off, dense with 'dense' taken out of
                    rt.TRAIN_ROUTES (the training launcher's dense route looks at no switch): conv_route answers
                    differently, both runs within the same bound
  determinism       two calls of a case are bit-equal, with another case run between them through _CL_POOL
"""
import pytest
import torch

import abi_bufs
import convlayer_refs as clr

pytestmark = pytest.mark.gpu
DEV = abi_bufs.DEV
NAMES = list(clr.CASES)


@pytest.fixture(autouse=True)
def _end_of_test():
    yield
    abi_bufs.end_of_test()


def _mods():
    import fastfourierconvolution_amd  # noqa: F401  (registers torch.ops.ffc.*)
    from fastfourierconvolution_amd import _autograd as ag, _plan, _runtime as rt
    return ag, _plan, rt


def _dev(ts, grad=False):
    return [t.to(DEV).requires_grad_(grad) for t in ts]


def _run(name):
    """forward and backward of a case through the op -> convlayer_refs.Result of device tensors (g_pre unused)"""
    _mods()
    c, data = clr.CASES[name], clr.inputs(name)
    xs, ws, bs = _dev(data.xs, True), _dev(data.ws, True), _dev(data.bs, True)
    ys = torch.ops.ffc.conv_layer(xs, ws, bs, clr.spec_of(c))
    no = len(c.outs)
    pres, it = [None] * no, iter(ys[no:])
    for j, (_, act, _) in enumerate(c.outs):
        if act == clr.GELU:
            pres[j] = next(it)
    assert next(it, None) is None and len(ys) == no + sum(p is not None for p in pres)
    grads = torch.autograd.grad(list(ys[:no]), xs + ws + bs, _dev(data.gouts))
    n, m = len(xs), len(xs) + len(ws)
    return clr.Result(list(ys[:no]), pres, [], list(grads[:n]), list(grads[n:m]), list(grads[m:]))


def _check(name, got, what="", ref=None, bnd=None):
    """print every tensor's share of its bound, then assert each <= 1"""
    c = clr.CASES[name]
    if ref is None:
        ref, bnd = clr.reference(name)
    for (_, lab, g), (_, _, r) in zip(clr.tensors(c, got), clr.tensors(c, ref)):
        assert tuple(g.shape) == tuple(r.shape), (name, lab, g.shape)
        assert bool(torch.isfinite(g).all()), f"{name} {lab}: non-finite elements"
    s = clr.shares(c, got, ref, bnd)
    for (fam, lab), v in s.items():
        print(f"OBS share {fam} {name}{what} {lab} {v:.4f}")
    bad = {k: v for k, v in s.items() if not v <= 1.0}
    assert not bad, (name, what, bad)


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_fp64(name):
    _check(name, _run(name))


# --------------------------------------------------------------------------- conv_layer_backward, called directly
def _backward_args(name):
    """(xs, ws, ts, gouts, n_in, ne, nb, spec) of a direct conv_layer_backward call: ts from the op's own forward"""
    _mods()
    c, data = clr.CASES[name], clr.inputs(name)
    xs, ws, bs = _dev(data.xs), _dev(data.ws), _dev(data.bs)
    spec = clr.spec_of(c)
    ys = torch.ops.ffc.conv_layer(xs, ws, bs, spec)
    no = len(c.outs)
    it = iter(ys[no:])
    ts = [next(it) if act == clr.GELU else ys[j] for j, (_, act, _) in enumerate(c.outs)]
    return xs, ws, ts, _dev(data.gouts), len(xs), len(ws), len(bs), spec


def _as_result(c, res, n_in, ne):
    return clr.Result([], [], [], list(res[:n_in]), list(res[n_in:n_in + ne]), list(res[n_in + ne:]))


def _check_grads(name, res, gouts, what):
    """dx / dW / db of a direct call against the reference with the dead outputs' cotangents zero"""
    c, data = clr.CASES[name], clr.inputs(name)
    ref = clr.graph(c, data, gouts=gouts)
    bnd = clr.bounds(c, data, ref, gouts=gouts)
    for fam, got, want, lim in (("dx", res.dx, ref.dx, bnd.dx), ("dW", res.dW, ref.dW, bnd.dW),
                                ("db", res.db, ref.db, bnd.db)):
        for k, (g, r, b) in enumerate(zip(got, want, lim)):
            assert tuple(g.shape) == tuple(r.shape)
            v = clr.share(g, r, b)
            print(f"OBS share {fam} {name} {what} {k} {v:.4f}")
            assert v <= 1.0, (name, what, fam, k, v)


@pytest.mark.parametrize("dead", [0, 1])
def test_dead_output_contributes_exactly_zero(dead):
    c, data = clr.CASES["fan_share"], clr.inputs("fan_share")
    xs, ws, ts, gouts, n_in, ne, nb, spec = _backward_args("fan_share")
    gl = [None if j == dead else g for j, g in enumerate(gouts)]
    res = torch.ops.ffc.conv_layer_backward(xs, ws, ts, gl, [True] * (n_in + ne + nb), spec)
    got = _as_result(c, res, n_in, ne)
    # the bound of the dead output's share of dx is zero: only the live output's rounding is allowed
    _check_grads("fan_share", got, [None if j == dead else g for j, g in enumerate(data.gouts)], f"dead={dead}")
    for e, ed in enumerate(c.edges):
        if ed[0] == dead:
            assert got.dW[e].shape == ws[e].shape and not got.dW[e].any(), "weight of a dead output: exact zeros"
            if ed[9] >= 0:
                assert got.db[ed[9]].shape == (c.outs[dead][0],) and not got.db[ed[9]].any()
    # dx is the live edge's adjoint alone: bit-equal to the same call on a spec that holds only that edge
    live = 1 - dead
    e_live = next(e for e, ed in enumerate(c.edges) if ed[0] == live)
    ed = c.edges[e_live]
    one = c._replace(outs=(c.outs[live],), edges=((0,) + ed[1:9] + (-1,),))
    alone = torch.ops.ffc.conv_layer_backward(xs, [ws[e_live]], [ts[live]], [gouts[live]], [True, True],
                                              clr.spec_of(one))
    assert torch.equal(alone[0], got.dx[0]) and torch.equal(alone[1], got.dW[e_live])


def test_all_outputs_dead_gives_exact_zeros():
    c = clr.CASES["shortcut"]
    xs, ws, ts, gouts, n_in, ne, nb, spec = _backward_args("shortcut")
    res = torch.ops.ffc.conv_layer_backward(xs, ws, ts, [None], [True] * (n_in + ne + nb), spec)
    for r, like in zip(res, xs + ws + [torch.empty(c.outs[0][0])] * nb):
        assert r.shape == like.shape and not r.any()


@pytest.mark.parametrize("name", ["fan_share", "shortcut"])
def test_each_needs_entry_false_in_turn(name):
    xs, ws, ts, gouts, n_in, ne, nb, spec = _backward_args(name)
    n = n_in + ne + nb
    full = torch.ops.ffc.conv_layer_backward(xs, ws, ts, gouts, [True] * n, spec)
    _check_grads(name, _as_result(clr.CASES[name], full, n_in, ne), clr.inputs(name).gouts, "needs all")
    for k in range(n):
        res = torch.ops.ffc.conv_layer_backward(xs, ws, ts, gouts, [q != k for q in range(n)], spec)
        assert len(res) == n and res[k].numel() == 0
        for q in range(n):
            if q != k:
                assert torch.equal(res[q], full[q]), (name, k, q)


# --------------------------------------------------------------------------- refusals
def _launches(fn, exc):
    """run fn, which must raise exc, under a launch observer -> the launches it recorded"""
    _, _, rt = _mods()
    obs = rt.LaunchObserver()
    rt.set_observer(obs)
    try:
        with pytest.raises(exc):
            fn()
    finally:
        rt.set_observer(None)
    return obs.records


def test_refusals_launch_nothing():
    ag, _plan, _ = _mods()
    c, data = clr.CASES["addend_a0"], clr.inputs("addend_a0")
    xs, ws, bs = _dev(data.xs), _dev(data.ws), _dev(data.bs)
    feeds = c._replace(adds=((0, 0),))      # input 0 is the addend and feeds the edge
    assert _launches(lambda: torch.ops.ffc.conv_layer(xs, ws, bs, clr.spec_of(feeds)), NotImplementedError) == []
    short = [xs[0], xs[1][:, :, :, :-1].contiguous()]
    assert _launches(lambda: torch.ops.ffc.conv_layer(short, ws, bs, clr.spec_of(c)), RuntimeError) == []
    for kw in (dict(pool=True), dict(gate=True)):
        assert _launches(lambda: ag.adjoint_seg(_plan.Seg("pw", 6, 4, 4, **kw), 8, 4, 4), NotImplementedError) == []


# --------------------------------------------------------------------------- the route switch
@pytest.mark.parametrize("name", clr.SMALLM_CASES)
def test_both_routes_within_the_bound(name):
    ag, _, rt = _mods()
    c, data = clr.CASES[name], clr.inputs(name)
    segs = tuple(ag._edge_seg(ed, x) for ed, x in ((ed, data.xs[ed[1]]) for ed in c.edges))
    wts = [rt.ConvWeight(data.ws[e], ed[8], ed[3], ed[3], data.bs[ed[9]] if ed[9] >= 0 else None)
           for e, ed in enumerate(c.edges)]

    def route():
        return rt.conv_route(segs, wts, c.outs[0][0], False, False, rt.TRAIN_ROUTES, training=True)

    first = route()
    assert first == c.routes[0] and first is not None
    _check(name, _run(name), f" [{first}]")
    prev = rt.USE_SMALLM, rt.TRAIN_ROUTES
    try:
        if name == "dense":
            rt.TRAIN_ROUTES = rt.TRAIN_ROUTES - {"dense"}
        else:
            rt.USE_SMALLM = False
        second = route()
        assert second is None, (name, second)
        got = _run(name)
    finally:
        rt.USE_SMALLM, rt.TRAIN_ROUTES = prev
    assert route() == first
    _check(name, got, " [implicit GEMM]")


# --------------------------------------------------------------------------- determinism through the shared cache
@pytest.mark.parametrize("name,between", [("ct3seg", "fan_stride"), ("fan_stride", "ct3seg"), ("headT", "full2")])
def test_two_calls_are_bit_equal(name, between):
    c = clr.CASES[name]
    a = _run(name)
    _run(between)
    b = _run(name)
    for (_, lab, x), (_, _, y) in zip(clr.tensors(c, a), clr.tensors(c, b)):
        assert torch.equal(x, y), (name, lab)
