"""Cases, float64 reference and per-element bounds of ffc::conv_layer and ffc::conv_layer_backward
(_autograd.conv_layer_impl / conv_layer_backward_impl and what they compose: conv_forward, adjoint_seg, conv_wgrad,
channel_sum), shared by test_gpu_conv_layer.py (the ops on the GPU) and test_convlayer_refs_cpu.py (branches, the
fp64 mirror of the host's data gradient, the rule that fixes TOL, planted defects).

Reference.  Plain torch.nn.functional.conv2d / conv_transpose2d in float64 on the CPU: per output the sum over its
edges, + bias, + addend, then conv_refs.act64; gradients by torch.autograd.grad with the given (random) cotangents.
A 'pw' edge is a 1x1 conv2d.  Weight layouts as in the op's spec: 0 = (M, C, k, k), 1 = (C, M, k, k).  Nothing here
imports the package under test: the mirror takes adjoint_seg, plan_job and Seg as arguments.

Bound, per element: |got - ref| <= TOL * magnitude (+ the activation terms below), the magnitude being the same
expression on absolute values:
  forward   pre: TOL * P,  P = sum conv(|x|, |w|) + |b| + |addend|;  out: the same for Identity / ReLU / LeakyReLU
            (Lipschitz 1; the slope product is one more rounding inside TOL)
  dx        sum adj(G, |w|), + G for an addend input           }  G = TOL * |g_pre| + D |gout|,
  dW        the weight-gradient correlation of G and |x|       }  g_pre = act'(t) gout in fp64,
  db        sum G                                              }  D = 0 for Identity / ReLU / LeakyReLU
so for the piecewise-linear activations every bound is exactly TOL times the magnitude the issue names.

The term added for Tanh / Sigmoid / GELU (after test_gpu_convq_kernels.py, which charges a transcendental epilogue
its Lipschitz constant times the linear bound plus 4 * 2^-23 * max(1, |pre|) for the device function, absolute
because GELU's 1 + erf cancels for negative arguments; test_gpu_train_kernels.py / test_gpu_norm_kernels.py hold
act_bwd and the apply kernels to a normwise 1e-5 for the same reason):
  out       L * TOL * P + A * max(1, |pre|),  L = 1 (Tanh), 1/4 (Sigmoid), 1.13 (GELU: sup |gelu'|),  A = 4 * 2^-23
  act'      the backward evaluates act' in fp32 at what the forward stored, which is off by the forward bound:
            D = L2 * (forward bound of the stored tensor) + A,  the stored tensor being the output for Tanh
            (act' = 1 - y^2, L2 = 2 |y| <= 2) and Sigmoid (act' = y (1 - y), L2 = |1 - 2 y| <= 1) and the
            pre-activation for GELU (L2 = sup |gelu''| = 2 pdf(0) < 0.8); A covers erff / expf / tanhf and the few
            roundings of an O(1) derivative.  D |gout| is pushed through the same linear maps as |g_pre|.

TOL = 1e-5: the smallest power of ten for which float32 CPU torch, running the same graph (graph(...,
torch.float32)) on one thread and on the default thread count (its sums change order with the thread count), stays
within a quarter of the bound on every case and every tensor.  Worst fp32-torch share per family at 1e-5: forward
0.019 (dense), dx 0.024 (ct3seg dx2), dW 0.028 (ct3seg dW1), db 0.005 (dense_bias); at 1e-6 the worst is 0.279
(ct3seg dW1, one thread), above the quarter (test_convlayer_refs_cpu.py::test_tol_rule computes and asserts both).
TOL was fixed on the CPU before the first GPU run.

Largest share of the bound on one MI355X (max over cases and elements of |got - ref| / bound):
  forward 0.025 (fan_mix out0)   dx 0.025 (ct3seg dx0)   dW 0.032 (ct3seg dW0)   db 0.0024 (full2)
the direct calls, both routes of the small-M cases and the split-bf16 weight gradient included: no family needs a
coefficient of its own, and the GPU's error is of the size of fp32 torch's.

Kinks: the seeds are such that no pre-activation of a ReLU / LeakyReLU output lies within its forward bound of zero
(asserted on the CPU for every case: the smallest |pre| / bound is 4.9, c3), so no element is excluded from any
comparison.  A case's seed is its position in the table; ct3seg's (5, then 25) left an element within 1e-5 of its
magnitude of zero and the next integer, 26, was taken.

Case -> branch: CASES below (Case.branch; the CPU file asserts ops / chained / routes from shapes alone).
"""
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

import conv_refs as cr

TOL = 1e-5
ROOM = 0.25                 # the share of the bound plain fp32 torch may use
ACT_ABS = 4 * 2.0 ** -23    # a transcendental device function's own error (docstring)
SLOPE = cr.SLOPE
IDENT, RELU, LEAKY, TANH, SIGMOID, GELU = (cr.ACT[n] for n in ("IDENTITY", "RELU", "LEAKY_RELU", "TANH", "SIGMOID",
                                                                "GELU"))
LIP = {TANH: 1.0, SIGMOID: 0.25, GELU: 1.13}    # sup |act'|
LIP2 = {TANH: 2.0, SIGMOID: 1.0, GELU: 0.8}     # sup |d act' / d (stored tensor)|
FAMILIES = ("forward", "dx", "dW", "db")


class Case(NamedTuple):
    """inputs: (C, H, W) per input; outs: (M, act, param); edges: the spec's tuples (j, i, kind, k, s, p, d, op,
    layout, bias index or -1); adds: (j, i).  Expected branches: ops[e] = output_padding of edge e's adjoint (None:
    not a Conv2d edge); chained[i] = the adjoint segments of input i cannot share a job (None: fewer than two);
    routes[j] = rt.conv_route's answer for output j's forward job on the training path"""
    B: int
    inputs: tuple
    outs: tuple
    edges: tuple
    adds: tuple
    seed: int
    ops: tuple
    chained: tuple
    routes: tuple
    branch: str


def _conv(j, i, k, s=1, p=0, d=1, bias=-1):
    return (j, i, "conv", k, s, p, d, 0, 0, bias)


def _convT(j, i, k, s=1, p=0, d=1, op=0, bias=-1):
    return (j, i, "convT", k, s, p, d, op, 1, bias)


def _pw(j, i, bias=-1):
    return (j, i, "pw", 1, 1, 0, 1, 0, 0, bias)


CASES = {
    "c3": Case(2, ((7, 5, 7),), ((36, RELU, 0.0),), (_conv(0, 0, 3, 1, 1, bias=0),), (), 1, (0,), (None,), (None,),
               "plain conv; adjoint convT s1"),
    "c3s2_even": Case(2, ((5, 8, 6),), ((12, IDENT, 0.0),), (_conv(0, 0, 3, 2, 1, bias=0),), (), 2, (1,), (None,),
                      (None,), "adjoint with output_padding 1 on both axes (even plane, k3 s2 p1)"),
    "c4s2_odd": Case(2, ((5, 9, 7),), ((12, LEAKY, SLOPE),), (_conv(0, 0, 4, 2, 1),), (), 3, (1,), (None,), (None,),
                     "output_padding 1 from an odd plane (k4 s2 p1)"),
    "cdil": Case(2, ((4, 7, 9),), ((10, SIGMOID, 0.0),), (_conv(0, 0, 3, 1, 2, 2, bias=0),), (), 4, (0,), (None,),
                 (None,), "dilated adjoint"),
    "ct3seg": Case(3, ((20, 4, 4), (12, 4, 4), (8, 8, 8)), ((40, LEAKY, SLOPE),),
                   (_convT(0, 0, 4, 2, 1, bias=0), _convT(0, 1, 4, 2, 1), _pw(0, 2)), (), 26, (None, None, None),
                   (None, None, None), (None,),
                   "three inputs; adjoints conv s2 x2 and pw; conv_wgrad operand swap for the convT edges"),
    "dense": Case(3, ((10, 1, 1),), ((70, IDENT, 0.0),), (_convT(0, 0, 4),), (), 6, (None,), (None,), ("dense",),
                  "route 'dense' (ConvT k4 s1 p0 on a 1x1 input, no bias)"),
    "dense_bias": Case(3, ((10, 1, 1),), ((70, IDENT, 0.0),), (_convT(0, 0, 4, bias=0),), (), 7, (None,), (None,),
                       (None,), "the same job with a bias: the 16 one-tap-phase implicit GEMM"),
    "fan_share": Case(2, ((6, 8, 8),), ((12, GELU, 0.0), (9, IDENT, 0.0)),
                      (_conv(0, 0, 3, 1, 1, bias=0), _conv(1, 0, 3, 1, 1)), (), 8, (0, 0), (False,), (None, None),
                      "two adjoint segments in one job; GELU pre-activation output"),
    "fan_stride": Case(2, ((6, 8, 8),), ((10, IDENT, 0.0), (7, IDENT, 0.0)),
                       (_conv(0, 0, 3, 1, 1), _conv(1, 0, 4, 2, 1, bias=0)), (), 9, (0, 0), (True,), (None, None),
                       "adjoints convT s1 + convT s2: plan_job refuses, chained through the addend"),
    "fan_mix": Case(2, ((6, 4, 4),), ((10, IDENT, 0.0), (7, IDENT, 0.0)),
                    (_convT(0, 0, 4, 2, 1), _conv(1, 0, 4, 2, 1)), (), 10, (None, 0), (True,), (None, None),
                    "adjoints conv s2 + convT s2: refused, chained"),
    "addend_a0": Case(2, ((8, 5, 7), (8, 5, 7)), ((8, IDENT, 0.0),), (_conv(0, 0, 3, 1, 1, bias=0),), ((0, 1),), 11,
                      (0,), (None, None), (None,), "adds; the addend's gradient (identity)"),
    "addend_a1": Case(2, ((8, 5, 7), (8, 5, 7)), ((8, RELU, 0.0),), (_conv(0, 0, 3, 1, 1, bias=0),), ((0, 1),), 12,
                      (0,), (None, None), (None,), "adds; the addend's gradient through ReLU"),
    "shortcut": Case(2, ((8, 6, 5), (5, 6, 5)), ((12, IDENT, 0.0),), (_conv(0, 0, 3, 1, 1, bias=0), _pw(0, 1, bias=1)),
                     (), 13, (0, None), (None, None), (None,), "the DBlock job: conv + pw, two biases, two db"),
    "headT": Case(2, ((9, 5, 3), (8, 5, 3)), ((3, TANH, 0.0),), (_convT(0, 0, 4, 2, 1, bias=0), _convT(0, 1, 4, 2, 1)),
                  (), 14, (None, None), (None, None), ("convT",),
                  "route 'convT' (small M); its adjoints (conv s2, M 9 / 8) on the implicit GEMM"),
    "full": Case(3, ((7, 4, 4),), ((1, IDENT, 0.0),), (_conv(0, 0, 4, bias=0),), (), 15, (0,), (None,), ("full",),
                 "route 'full', one plane size"),
    "full2": Case(3, ((7, 4, 4), (5, 2, 2)), ((1, IDENT, 0.0),), (_conv(0, 0, 4, bias=0), _conv(0, 1, 2)), (), 16,
                  (0, 0), (None, None), ("full",), "route 'full', two plane sizes (training only)"),
    "headT3": Case(2, ((17, 5, 7),), ((3, TANH, 0.0),), (_convT(0, 0, 3, 1, 1, bias=0),), (), 17, (None,), (None,),
                   ("convT3",), "route 'convT3' and ffc_convt3x3_smallm_dgrad"),
}
SMALLM_CASES = ("headT", "full", "full2", "headT3", "dense")


def spec_of(case):
    """the op's spec string, as _autograd.conv_spec writes it"""
    import json
    d = {"outs": [[int(M), int(a), float(p)] for M, a, p in case.outs], "edges": [list(e) for e in case.edges]}
    if case.adds:
        d["adds"] = [list(a) for a in case.adds]
    return json.dumps(d, separators=(",", ":"))


def out_hw(e, H, W):
    _, _, kind, k, s, p, d, op, _, _ = e
    if kind == "conv":
        return tuple((n + 2 * p - d * (k - 1) - 1) // s + 1 for n in (H, W))
    if kind == "convT":
        return tuple((n - 1) * s - 2 * p + d * (k - 1) + op + 1 for n in (H, W))
    return H, W


def w_shape(case, e):
    j, i, kind, k = case.edges[e][:4]
    M, C = case.outs[j][0], case.inputs[i][0]
    return (C, M, k, k) if case.edges[e][8] == 1 else (M, C, k, k)


def n_bias(case):
    return sum(1 for e in case.edges if e[9] >= 0)


class Data(NamedTuple):
    xs: list
    ws: list
    bs: list
    gouts: list


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 inputs, weights (1 / sqrt(fan-in of the output)), biases and fresh random cotangents of a case"""
    c = CASES[name]
    gen = torch.Generator().manual_seed(7000 + c.seed)
    xs = [torch.randn((c.B,) + shp, generator=gen) for shp in c.inputs]
    ws, bs = [], [None] * n_bias(c)
    for e, ed in enumerate(c.edges):
        j, kind, k, s = ed[0], ed[2], ed[3], ed[4]
        fan = sum(c.inputs[o[1]][0] * (max(1, o[3] * o[3] // (o[4] * o[4])) if o[2] == "convT" else o[3] * o[3])
                  for o in c.edges if o[0] == j)
        ws.append(torch.randn(w_shape(c, e), generator=gen) / fan ** 0.5)
        if ed[9] >= 0:
            bs[ed[9]] = 0.5 * torch.randn((c.outs[j][0],), generator=gen)
    gouts = []
    for j, (M, _, _) in enumerate(c.outs):
        e = next(ed for ed in c.edges if ed[0] == j)
        gouts.append(torch.randn((c.B, M) + out_hw(e, *c.inputs[e[1]][1:]), generator=gen))
    return Data(xs, ws, bs, gouts)


# --------------------------------------------------------------------------- the graph, in any dtype
def _edge(x, w, e):
    _, _, kind, k, s, p, d, op, lay, _ = e
    if kind == "convT":
        return F.conv_transpose2d(x, w if lay == 1 else w.transpose(0, 1), stride=s, padding=p, output_padding=op,
                                  dilation=d)
    w = w if lay == 0 else w.transpose(0, 1)
    return F.conv2d(x, w) if kind == "pw" else F.conv2d(x, w, stride=s, padding=p, dilation=d)


def pre_acts(case, xs, ws, bs):
    adds = dict(case.adds)
    pres = []
    for j in range(len(case.outs)):
        t = 0
        for e, ed in enumerate(case.edges):
            if ed[0] != j:
                continue
            t = t + _edge(xs[ed[1]], ws[e], ed)
            if ed[9] >= 0:
                t = t + bs[ed[9]][None, :, None, None]
        if j in adds:
            t = t + xs[adds[j]]
        pres.append(t)
    return pres


def _leaves(data, dtype, absolute=False):
    def leaf(t):
        t = t.to(dtype)
        return (t.abs() if absolute else t.clone()).requires_grad_(True)
    return [leaf(t) for t in data.xs], [leaf(t) for t in data.ws], [leaf(t) for t in data.bs]


class Result(NamedTuple):
    outs: list      # per output
    pres: list      # per output (the op appends those of the GELU outputs)
    g_pre: list     # per output: act'(t) * gout
    dx: list
    dW: list
    db: list


def graph(case, data, dtype=torch.float64, gouts=None, gelu_from_output=False):
    """forward and backward of the case in ``dtype`` (float64: the reference; float32: plain torch for the TOL rule).
    gouts: cotangents per output (None entries: a dead output, cotangent zero).  gelu_from_output: the planted
    defect that hands the GELU backward the output instead of the pre-activation"""
    xs, ws, bs = _leaves(data, dtype)
    pres = pre_acts(case, xs, ws, bs)
    outs = [cr.act64(t, act, param) for t, (_, act, param) in zip(pres, case.outs)]
    gouts = data.gouts if gouts is None else gouts
    gouts = [torch.zeros_like(o) if g is None else g.to(dtype) for g, o in zip(gouts, outs)]
    g_pre = list(torch.autograd.grad(outs, pres, gouts, retain_graph=True))
    if gelu_from_output:
        for j, (_, act, param) in enumerate(case.outs):
            if act == GELU:
                y = outs[j].detach().clone().requires_grad_(True)
                g_pre[j], = torch.autograd.grad(cr.act64(y, act, param), y, gouts[j])
    grads = torch.autograd.grad(pres, xs + ws + bs, g_pre)
    n, m = len(xs), len(xs) + len(ws)
    det = [g.detach() for g in grads]
    return Result([o.detach() for o in outs], [t.detach() for t in pres], [g.detach() for g in g_pre],
                  det[:n], det[n:m], det[m:])


def bounds(case, data, ref, tol=TOL, gouts=None):
    """-> Result of per-element bounds for ``ref`` (the float64 graph); g_pre holds G (docstring)"""
    f64 = torch.float64
    xs, ws, bs = _leaves(data, f64, absolute=True)
    P = pre_acts(case, xs, ws, bs)
    gouts = data.gouts if gouts is None else gouts
    b_out, b_pre, G = [], [], []
    for j, (_, act, _) in enumerate(case.outs):
        lin = tol * P[j].detach()
        out = lin if act in (IDENT, RELU, LEAKY) else LIP[act] * lin + ACT_ABS * ref.pres[j].abs().clamp_min(1.0)
        g = torch.zeros_like(lin) if gouts[j] is None else gouts[j].to(f64).abs()
        Gj = tol * ref.g_pre[j].abs()
        if act not in (IDENT, RELU, LEAKY):
            stored = lin if act == GELU else out
            Gj = Gj + (LIP2[act] * stored + ACT_ABS) * g
        b_out.append(out)
        b_pre.append(lin)
        G.append(Gj)
    grads = [g.detach() for g in torch.autograd.grad(P, xs + ws + bs, G)]
    n, m = len(xs), len(xs) + len(ws)
    return Result(b_out, b_pre, G, grads[:n], grads[n:m], grads[m:])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 Result, bounds Result) of a case at TOL: computed once, shared, never modified"""
    c, data = CASES[name], inputs(name)
    ref = graph(c, data)
    return ref, bounds(c, data, ref)


def tensors(case, res):
    """[(family, label, tensor)] of a Result in the order the comparisons walk: outputs, the appended GELU
    pre-activations, dx, dW, db"""
    out = [("forward", f"out{j}", t) for j, t in enumerate(res.outs)]
    out += [("forward", f"pre{j}", res.pres[j]) for j, (_, act, _) in enumerate(case.outs) if act == GELU]
    out += [("dx", f"dx{i}", t) for i, t in enumerate(res.dx)]
    out += [("dW", f"dW{e}", t) for e, t in enumerate(res.dW)]
    out += [("db", f"db{b}", t) for b, t in enumerate(res.db)]
    return out


def share(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0: a dead output's exact zeros)"""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    ok = (err == 0) & (bound == 0)
    return float(torch.where(ok, torch.zeros_like(err), err / bound).max())


def shares(case, got, ref, bnd):
    """{(family, label): share} of a Result-like ``got`` against the reference"""
    return {(fam, lab): share(g, r, b) for (fam, lab, g), (_, _, r), (_, _, b)
            in zip(tensors(case, got), tensors(case, ref), tensors(case, bnd))}


def kink_margin(case, ref, bnd):
    """min over the ReLU / LeakyReLU outputs' elements of |pre| / (forward bound of pre): must exceed 1"""
    m = float("inf")
    for j, (_, act, _) in enumerate(case.outs):
        if act in (RELU, LEAKY):
            m = min(m, float((ref.pres[j].abs() / bnd.pres[j]).min()))
    return m


# --------------------------------------------------------------------------- the host's backward, mirrored in fp64
def wgrad_ref(U, V, k, s, p, d):
    """ffc_conv_wgrad: dW[m][n][kh][kw] = sum_{b, q} U[b, m, q] V[b, n, q s - p + k d], zeros outside V"""
    B, Mu, PH, PW = U.shape
    _, Nv, VH, VW = V.shape
    hi = [max(n, (k - 1) * d + (P - 1) * s + 1 - p) for n, P in ((VH, PH), (VW, PW))]
    Vp = torch.zeros(B, Nv, p + hi[0], p + hi[1], dtype=torch.float64)
    Vp[:, :, p:p + VH, p:p + VW] = V
    dW = torch.zeros(Mu, Nv, k, k, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            win = Vp[:, :, kh * d: kh * d + (PH - 1) * s + 1: s, kw * d: kw * d + (PW - 1) * s + 1: s]
            dW[:, :, kh, kw] = torch.einsum("bmhw,bnhw->mn", U.double(), win)
    return dW


def mirror_backward(case, data, g_pre, Seg, adjoint_seg, plan_job, defect=None, gouts=None):
    """_autograd.conv_layer_backward_impl restated in float64 from the pre-activation gradients: the data gradient
    as conv_refs.conv_job_ref over adjoint_seg of each edge with the weight's layout flipped, one job where
    plan_job takes the segments together and chained through the addend where it raises ValueError; the weight
    gradient as wgrad_ref with the operands in conv_wgrad's order (x first for a convT edge); db = sum g_pre.
    defect: 'op' (the adjoint's output_padding dropped: the last rows / columns stay zero), 'wgrad_swap' (a convT
    edge's operands in a conv edge's order), 'addend' (the addend's gradient omitted), 'db_post' (db from the
    post-activation gradient), 'chain' (a chained group's running sum not passed on).  -> (dx, dW, db, chained per
    input)"""
    f64 = torch.float64
    xs, ws = [x.to(f64) for x in data.xs], [w.to(f64) for w in data.ws]
    added = {i: j for j, i in case.adds}
    dx, chained = [], []
    for i, x in enumerate(xs):
        if i in added:
            dx.append(torch.zeros_like(x) if defect == "addend" else g_pre[added[i]].clone())
            chained.append(None)
            continue
        adj = []
        for e, ed in enumerate(case.edges):
            if ed[1] != i:
                continue
            g = g_pre[ed[0]]
            kind, k, s, p, d, op = ed[2:8]
            sg = Seg("pw", x.shape[1], x.shape[2], x.shape[3]) if kind == "pw" else \
                Seg(kind, x.shape[1], x.shape[2], x.shape[3], k, s, p, d, op)
            a = adjoint_seg(sg, g.shape[1], g.shape[2], g.shape[3])
            if defect == "op" and a.kind == "convT":
                a = Seg("convT", a.C, a.IH, a.IW, a.k, a.s, a.p, a.d, 0)
            adj.append((e, a, ed[8], g))
        groups = [adj]
        chain = None
        if len(adj) > 1:
            chain = False
            try:
                plan_job(case.B, x.shape[1], tuple(a[1] for a in adj))
            except ValueError:
                groups, chain = [[a] for a in adj], True
        acc = None
        for grp in groups:
            pre, _ = cr.conv_job_ref([a[1] for a in grp], [a[3] for a in grp], [ws[a[0]] for a in grp],
                                     [1 - a[2] for a in grp], addend=None if defect == "chain" else acc)
            acc = torch.zeros_like(x)
            acc[:, :, :pre.shape[2], :pre.shape[3]] = pre     # smaller than x only under defect 'op'
        dx.append(acc)
        chained.append(chain)
    dW, db = [], [None] * n_bias(case)
    for e, ed in enumerate(case.edges):
        j, i, kind, k, s, p, d = ed[:7]
        xT = (kind == "convT") != (defect == "wgrad_swap" and kind == "convT")
        U, V = (xs[i], g_pre[j]) if xT else (g_pre[j], xs[i])
        dW.append(wgrad_ref(U, V, k, s, p, d).reshape(ws[e].shape))
        if ed[9] >= 0:
            src = (data.gouts if gouts is None else gouts)[j].to(f64) if defect == "db_post" else g_pre[j]
            db[ed[9]] = src.sum(dim=(0, 2, 3))
    return dx, dW, db, chained
