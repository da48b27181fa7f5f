"""The wide Self_Attn kernels (72 <= C <= 256) on the GPU: through the layer (stacked projection, ffc::self_attn,
ffc::self_attn_matrix, ffc::self_attn_bwd, routed to ffc_attnw_*) and through the raw ffc_attnw_* entry points,
against the float64 references of tests/attn_refs.py on the inputs of tests/attn_wide_cases.py.

Bounds: attn_wide_cases.layer_bounds / core_bounds -- 1e-5 normwise, or four times what plain float32 leaves on
the same input where that passes a quarter of 1e-5 (tests/test_attn_wide_refs_cpu.py prints and proves them).
Raw outputs and the workspace are prefilled with NaN with guard bands behind them (tests/abi_bufs.py).

The memory test departs from "peak below B N N floats" as it holds at C << N: at 16 x 16 and C = 256 the output
alone is B C N = B N N floats, so the test bounds what the forward allocates beyond its stacked projection, its
output and L, and that is what has to stay below one attention matrix.
"""
import pytest
import torch

import abi_bufs as A
import attn_refs as R
import attn_wide_cases as W
import fastfourierconvolution_amd as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _end_of_test():
    yield
    A.end_of_test()


def _layer(p, need_attention=True):
    mod = F.Self_Attn(p["value_conv.weight"].shape[0], "relu")
    mod.load_state_dict(p)
    mod.need_attention = need_attention
    return mod.to(DEV)


def _run(p, x, dy, need_attention=True):
    mod = _layer(p, need_attention)
    xd = x.to(DEV).requires_grad_(True)
    out, attention = mod(xd)
    (out * dy.to(DEV)).sum().backward()
    got = {k: v.grad for k, v in mod.named_parameters()}
    got.update(x=xd.grad, out=out.detach())
    if attention is not None:
        got["attention"] = attention
    return got


def _check(name, errs, bounds):
    print("OBS", name, {k: f"{e:.2e}" for k, e in errs.items()})
    bad = {k: (e, bounds[k]) for k, e in errs.items() if not e <= bounds[k]}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(W.SHAPES))
def test_layer_against_fp64(name):
    c = W.case(name)
    got = _run(c["p"], c["x"], c["dy"])
    assert got["attention"].shape == c["ref"]["attention"].shape and not got["attention"].requires_grad
    assert set(got) == set(W.LAYER_OUTPUTS)
    _check(name, W.layer_errors(c, got), W.layer_bounds(name))


def _raw(c, with_o=True):
    """ffc_attnw_forward, _matrix and _backward on NaN-prefilled guarded buffers -> {output: CPU tensor}"""
    B, C, H, Wd = c["shape"]
    N, d = H * Wd, C // 8
    M = (2 * d + C) * N
    L = A.lib()
    qkv = A.Buf(B * M, fill=torch.cat([c["q"], c["k"], c["v"]], 1))
    q, k, v = qkv.ptr(), qkv.ptr(d * N), qkv.ptr(2 * d * N)
    x, dy = A.Buf(B * C * N, fill=c["x"]), A.Buf(B * C * N, fill=c["dy"])
    gamma = A.keep(torch.full((1,), float(c["gamma"]), device=A.DEV))
    y, Lb, o, P = A.Buf(B * C * N), A.Buf(B * N), A.Buf(B * C * N), A.Buf(B * N * N)
    A.ok(L.ffc_attnw_forward(q, k, v, M, x.ptr(), gamma.data_ptr(), y.ptr(), Lb.ptr(), o.ptr() if with_o else None, B, C,
                             H, Wd, A.stream()), "ffc_attnw_forward")
    got = dict(y=y.get("y").reshape(B, C, N), L=Lb.get("L").reshape(B, N))
    if not with_o:
        assert o.untouched()
        return got
    got["o"] = o.get("o").reshape(B, C, N)
    A.ok(L.ffc_attnw_matrix(q, k, M, Lb.ptr(), P.ptr(), B, C, H, Wd, A.stream()), "ffc_attnw_matrix")
    got["P"] = P.get("P").reshape(B, N, N)
    nws = L.ffc_attnw_ws_floats(B, C, H, Wd)
    assert nws == B * N + B * ((N + 255) // 256)
    g, dgamma, ws = A.Buf(B * M), A.Buf(1), A.Buf(nws)
    A.ok(L.ffc_attnw_backward(dy.ptr(), q, k, v, M, o.ptr(), Lb.ptr(), gamma.data_ptr(), g.ptr(), g.ptr(d * N),
                              g.ptr(2 * d * N), M, dgamma.ptr(), ws.ptr(), B, C, H, Wd, A.stream()), "ffc_attnw_backward")
    dqkv = g.get("dqkv").reshape(B, 2 * d + C, N)
    ws.get("ws")
    got.update(dq=dqkv[:, :d], dk=dqkv[:, d:2 * d], dv=dqkv[:, 2 * d:], dgamma=dgamma.get("dgamma").reshape(()))
    return got


@pytest.mark.parametrize("name", W.CORE_ALL)
def test_entry_points_against_fp64(name):
    c = W.core_case(name)
    got = _raw(c)
    assert set(got) == set(W.CORE_OUTPUTS)
    _check(name, W.core_errors(c, got), W.core_bounds(name))
    if name == "gamma_zero":
        assert torch.equal(got["y"], c["x"])
        assert all(float(got[k].abs().max()) == 0.0 for k in ("dq", "dk", "dv"))
    if name == "3x256x3x11":     # without o the forward writes the same y and L and leaves o alone
        again = _raw(c, with_o=False)
        assert torch.equal(again["y"], got["y"]) and torch.equal(again["L"], got["L"])


def test_entry_points_refuse_before_a_launch():
    c = W.core_case("1x256x4x4")
    B, C, H, Wd = c["shape"]
    N, d = H * Wd, C // 8
    M = (2 * d + C) * N
    L = A.lib()
    qkv, x = A.Buf(B * M, fill=torch.cat([c["q"], c["k"], c["v"]], 1)), A.Buf(B * C * N, fill=c["x"])
    gamma = A.keep(torch.full((1,), 0.7, device=A.DEV))
    y, Lb = A.Buf(B * C * N), A.Buf(B * N)
    args = (qkv.ptr(), qkv.ptr(d * N), qkv.ptr(2 * d * N))
    A.rejected(L.ffc_attnw_forward(*args, M - 1, x.ptr(), gamma.data_ptr(), y.ptr(), Lb.ptr(), None, B, C, H, Wd,
                                   A.stream()), "ffc_attnw_forward", "stride")
    A.rejected(L.ffc_attnw_forward(*args, M, x.ptr(), gamma.data_ptr(), None, Lb.ptr(), None, B, C, H, Wd, A.stream()),
               "ffc_attnw_forward", "null")
    for Cbad in (64, 100, 264):
        A.rejected(L.ffc_attnw_forward(*args, M, x.ptr(), gamma.data_ptr(), y.ptr(), Lb.ptr(), None, B, Cbad, H, Wd,
                                       A.stream()), "ffc_attnw_forward", "unsupported")
    assert y.untouched() and Lb.untouched()


def test_gamma_zero_returns_x_bit_for_bit():
    c = W.case("b3_c256_4x4")
    p = dict(c["p"], gamma=torch.zeros(1))
    got = _run(p, c["x"], c["dy"])
    assert torch.equal(got["out"].cpu(), c["x"])
    assert torch.equal(got["x"].cpu(), c["dy"])
    for k in R.NAMES[:-1]:
        assert float(got[k].abs().max()) == 0.0, k
    e = W.layer_errors(c, {"attention": got["attention"]})
    _check("gamma0", e, W.layer_bounds("b3_c256_4x4"))


def test_backward_is_deterministic():
    c = W.case("b3_c256_10x16")
    g1 = _run(c["p"], c["x"], c["dy"], need_attention=False)
    g2 = _run(c["p"], c["x"], c["dy"], need_attention=False)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    print("deterministic:", sorted(g1))


def test_without_attention_nothing_n_by_n_is_allocated():
    B, C, H, Wd = 4, 256, 16, 16
    N, d = H * Wd, C // 8
    gen = torch.Generator().manual_seed(901)
    p = R._random_params(C, gen)
    mod = _layer(p, need_attention=False)
    xd = torch.randn(B, C, H, Wd, generator=gen).to(DEV)
    with torch.no_grad():
        mod(xd)                      # the stacked weights and the packed forms are made once
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with torch.no_grad():
        out, attention = mod(xd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    needed = 4 * B * N * ((2 * d + C) + C + 1)      # qkv, out, L
    print(f"need_attention off: peak rose by {rise} bytes; qkv + out + L {needed}; one matrix {4 * B * N * N}")
    assert attention is None
    assert rise - needed < 4 * B * N * N
    mod.need_attention = True
    with torch.no_grad():
        out2, attention = mod(xd)
    assert tuple(attention.shape) == (B, N, N) and torch.equal(out, out2)


def test_no_grad_forward_captures_into_a_graph():
    c = W.case("b3_c256_4x4")
    mod = _layer(c["p"], need_attention=False)
    static_x = c["x"].to(DEV).clone()
    x2 = c["x"].flip(0).flip(3).contiguous()      # other samples and pixel order, the same score range
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out, _ = mod(static_x)
        graph.replay()
        e0 = R.normwise(static_out, c["ref"]["out"])
        static_x.copy_(x2.to(DEV))
        mod.gamma.fill_(-1.3)
        graph.replay()
        e1 = R.normwise(static_out, R.attn_ref(x2, dict(c["p"], gamma=torch.full((1,), -1.3)))["out"])
    print(f"graph replay: {e0:.2e}; with a changed x and gamma: {e1:.2e}")
    assert max(e0, e1) <= W.TOL_K


@pytest.mark.parametrize("C", [264, 100])
def test_unsupported_channels_raise_not_implemented(C):
    mod = F.Self_Attn(264, "relu").to(DEV)
    mod.chanel_in = C
    with pytest.raises(NotImplementedError, match=rf"\(1, {C}, 4, 4\)"):
        mod(torch.zeros(1, C, 4, 4, device=DEV))


@pytest.mark.parametrize("name", ["b2_c64_8x8", "b3_c16_6x6"])
def test_narrow_layers_still_run_the_narrow_entry_points(name):
    """Self_Attn(64) and Self_Attn(16): what the layer returns is bit for bit what ffc_attn_forward, ffc_attn_matrix
    and ffc_attn_backward return when called directly on the layer's own stacked projection"""
    from fastfourierconvolution_amd import _autograd as ag
    from fastfourierconvolution_amd import _plan
    c = R.case(name)
    B, C, H, Wd = c["x"].shape
    N, d = H * Wd, C // 8
    M = (2 * d + C) * N
    got = _run(c["p"], c["x"], c["dy"])
    mod = _layer(c["p"])
    xd, dyd = c["x"].to(DEV), c["dy"].to(DEV).contiguous()
    L = A.lib()
    with torch.no_grad():
        (qkv,) = ag.conv_layer(B, [(2 * d + C, 0, 0.0)], [(0, 0, _plan.Seg("pw", C, H, Wd), ag._StackedQKV(mod, False))],
                               [xd])
        q, k, v = (qkv.data_ptr() + 4 * r * N for r in (0, d, 2 * d))
        y, Lb, o, P = A.Buf(B * C * N), A.Buf(B * N), A.Buf(B * C * N), A.Buf(B * N * N)
        A.ok(L.ffc_attn_forward(q, k, v, M, xd.data_ptr(), mod.gamma.data_ptr(), y.ptr(), Lb.ptr(), o.ptr(), B, C, H, Wd,
                                A.stream()), "ffc_attn_forward")
        A.ok(L.ffc_attn_matrix(q, k, M, Lb.ptr(), P.ptr(), B, C, H, Wd, A.stream()), "ffc_attn_matrix")
        g, dgamma, ws = A.Buf(B * M), A.Buf(1), A.Buf(L.ffc_attn_ws_floats(B, C, H, Wd))
        A.ok(L.ffc_attn_backward(dyd.data_ptr(), q, k, v, M, o.ptr(), Lb.ptr(), mod.gamma.data_ptr(), g.ptr(),
                                 g.ptr(d * N), g.ptr(2 * d * N), M, dgamma.ptr(), ws.ptr(), B, C, H, Wd, A.stream()),
             "ffc_attn_backward")
        dqkv_op, dgamma_op = torch.ops.ffc.self_attn_bwd(dyd, qkv, o.get("o").reshape(B, C, N).to(DEV),
                                                         Lb.get("L").reshape(B, N).to(DEV), mod.gamma)
    assert torch.equal(got["out"].cpu().reshape(-1), y.get("y"))
    assert torch.equal(got["attention"].cpu().reshape(-1), P.get("P"))
    assert torch.equal(dqkv_op.cpu().reshape(-1), g.get("dqkv"))
    assert torch.equal(dgamma_op.cpu(), dgamma.get("dgamma")) and torch.equal(got["gamma"].cpu(), dgamma.get("dgamma"))
