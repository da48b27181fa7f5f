"""Training path: the implementations behind the autograd-registered custom ops of ops.py for the
FFC operator surface (BASELINE config 3, FFC-DCGAN generator + discriminator forward + backward),
and the module-facing helpers that compose those ops.

The reference differentiates through ATen.  Here every op the reference's forward is made of
is one ``torch.ops.ffc.*`` custom op whose forward AND backward (another ffc op, wired by
``register_autograd``) launch the HIP kernels of ``libffc_amd.so`` (no torch compute on the path,
no CPU fallback):

  reference op (file:line)                                  custom op          backward op / kernels
  FFC / FFCTranspose local convs + ST conv2, summed per     ffc::conv_layer    ffc::conv_layer_backward:
    output branch (ffc.py:89-97, ffc_transpose.py:96-106,                      act_bwd; adjoint conv/convT on
    spectral_transform.py:108), FU conv_layer (fourier_unity                  ffc_conv_forward / convp (same
    .py:45), ST conv1 (:89), nn.Linear                                        weight, other layout); wgrad
  BatchNorm2d (+ activation): bn_l/bn_g (ffc_bn_act.py:       ffc::bn_act        ffc::bn_act_backward (ffc_bn_bwd)
    73-81), ST bn1+act1 (:89), FU bn+relu (:46-49)
  SELayer (spectral_transform.py:23-28, :87)                 ffc::se_scale      ffc::se_scale_backward
  AvgPool2d(2) / Upsample(x2) downsample (:44-47, :77)       ffc::pool2/up2     each other (adjoints)
  rfftn + Re/Im interleave (fourier_unity.py:38-42)          ffc::rfft2         ffc::irfft2 (mirrored x 0.5)
  de-interleave + irfftn (+ x residual) (:51-56, ST :108)     ffc::irfft2        ffc::rfft2 (mirrored x 2)
  NoiseInjection (noise_injection.py:25-32)                  ffc::noise_inject  ffc::noise_wgrad
  local Fourier unit's split / cat and repeat + add           ffc::lfu_split     ffc::lfu_split_backward
    (spectral_transform.py:94-108; with set_lfu only)         ffc::lfu_tile_add  ffc::lfu_tile_backward
  Self_Attn after its stacked projection (attention_layer     ffc::self_attn     ffc::self_attn_bwd
    .py:30-39; the projection is an ffc::conv_layer)

FFT adjoints (verified in fp64): d/dX of irfftn(ortho) is rfftn(ortho) with the
mirrored bins doubled; d/dx of rfftn(ortho) is irfftn(ortho) with the mirrored bins halved.
The modules switch to this path when autograd is recording and an input or parameter needs a
gradient; under ``torch.no_grad()`` the fused inference kernels run.
"""
from __future__ import annotations

import functools
import json
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _plan
from . import _runtime as rt
from ._lib import FFCError, check, ptr


def wants_grad(module: nn.Module, *tensors) -> bool:
    if not torch.is_grad_enabled():
        return False
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        return True
    return any(p.requires_grad for p in module.parameters())


def _stream(t):
    return rt.stream_of(t)


def _act_out(t: torch.Tensor, act, param, stream):
    """out-of-place y = act(t) (GELU, which the backward needs the input of)"""
    C = t.shape[1]
    one = torch.ones(C, device=t.device, dtype=torch.float32)
    zero = torch.zeros(C, device=t.device, dtype=torch.float32)
    y = torch.empty_like(t)
    check(rt.lib().ffc_bn_act_apply(ptr(t), ptr(y), t.shape[0], C, t[0, 0].numel(), ptr(one), ptr(zero), act,
                                    float(param), stream), "ffc_bn_act_apply")
    return y


def act_backward(t, dy, act, param):
    """dx = dy * act'(.): t = activation output (GELU: input)"""
    if act == 0:
        return dy
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    with rt.observe("act_bwd", bytes=12.0 * dy.numel()):
        check(rt.lib().ffc_act_bwd(ptr(t), ptr(dy), ptr(dx), dy.numel(), act, float(param), _stream(dy)),
              "ffc_act_bwd")
    return dx


# --------------------------------------------------------------------------- convolutions
def adjoint_seg(sg: _plan.Seg, M: int, OH: int, OW: int) -> _plan.Seg:
    """the segment whose forward is the adjoint (data gradient) of ``sg`` (output M x OH x OW)"""
    if sg.pool or sg.gate:
        raise NotImplementedError("pooled / gated segments have no training path")
    if sg.kind == "pw":
        return _plan.Seg("pw", M, OH, OW)
    if sg.kind == "conv":
        base = _plan.convT_out(OH, sg.k, sg.s, sg.p, sg.d, 0)
        op = sg.IH - base
        if op != sg.IW - _plan.convT_out(OW, sg.k, sg.s, sg.p, sg.d, 0) or not 0 <= op < max(sg.s, sg.d):
            raise NotImplementedError(f"conv adjoint needs output_padding {op} for {sg}")
        return _plan.Seg("convT", M, OH, OW, sg.k, sg.s, sg.p, sg.d, op)
    adj = _plan.Seg("conv", M, OH, OW, sg.k, sg.s, sg.p, sg.d)
    if _plan.seg_out(adj) != (sg.IH, sg.IW):
        raise NotImplementedError(f"convT adjoint does not return to the input size for {sg}")
    return adj


def run_conv(cache, key, B, M, segs, weights, inputs, out_shape=None, act=(0, 0.0), addend=None):
    """one implicit-GEMM launch: out = act(sum_s conv_s(x_s) [+ addend]) (plans cached in ``cache``)"""
    dev = inputs[0].device
    # the job's full shape and the plan switches are part of the key (a caller's key alone may leave
    # out the output channels, and one cache serves every module of a structure)
    ex, lp = rt.cached_conv(cache, (key, B, M, tuple(segs), str(dev), rt.plan_knobs()), B, M, segs, weights, dev,
                            pw_ok=True)
    pl = ex.plan
    out = torch.empty(out_shape or (B, pl.M, pl.OH, pl.OW), device=dev, dtype=torch.float32)
    lp.launch([ex.job([(x, None) for x in inputs], out, act[0], act[1], addend, None)], _stream(out),
              flops=ex.flops)
    return out


def conv_forward(cache, key, B, M, segs, weights, inputs, out_shape=None, act=(0, 0.0), addend=None):
    """out = act(sum_s conv_s(x_s) [+ addend]) on the kernel rt.conv_route picks for the training path: a
    direct kernel (small M; ConvTranspose2d on a 1x1 input), the implicit-GEMM kernels otherwise"""
    weights = rt.conv_weights(weights)
    route = rt.conv_route(segs, weights, M, addend is not None, False, rt.TRAIN_ROUTES, training=True)
    if route is None:
        return run_conv(cache, key, B, M, segs, weights, inputs, out_shape, act, addend)
    stream = _stream(inputs[0])
    if route == "dense":
        # FFCGenerator ffc0 (models/ffc_generator.py:24): W (C, M, k, k) is the GEMM's (K, N) as it stands
        sg = segs[0]
        N = M * sg.k * sg.k
        out = torch.empty((B, M, sg.k, sg.k), device=inputs[0].device, dtype=torch.float32)
        rt.dense_forward(inputs[0], weights[0].w, None, B, sg.C, N, N, out, None, act, stream)
        return out
    # the packed convT weights in one slot per job: under spectral norm W / sigma is a new tensor every step
    return rt.smallm_forward(route, segs, weights, inputs, M, B, act, stream, rt.packs_of(cache), pack_slot=key)


def wgrad_splits(B, Mu, NT, P, bt=64):
    """split-K count for ffc_conv_wgrad (split-once kernel).  128x128 tiles: >= 512 workgroups and
    <= 1024 k per split; 64x64 tiles: >= 1024 workgroups and <= 4096 k per split; at most 1024 splits,
    >= 64 k each, partial sums capped at 32 M floats.  Fitted on MI355X to every weight gradient of
    the gan64train (B = 256) and fgan128train (B = 64) steps over 4-8 split counts each
    (tools/wgrad_probe.py, profiles/r03/wgrad/): the large tiles lose to the partial-sum traffic
    beyond ~1 k-deep splits, the small ones want the deeper grid"""
    tiles = -(-Mu // bt) * -(-NT // bt)
    K = B * P
    if bt >= 128:
        S = max(-(-512 // max(1, tiles)), K // 1024)
    else:
        S = max(-(-1024 // max(1, tiles)), K // 4096)
    S = min(S, 1024, max(1, K // 64), max(1, (32 << 20) // max(1, Mu * NT)))
    return max(1, S)


def conv_wgrad(U, V, k, s, p, d, dW_shape):
    """ffc_conv_wgrad: dW[m][n][kh][kw] = sum U[b,m,q] V[b,n,q*s-p+k*d] (see include/ffc_amd.h)"""
    B, Mu, PH, PW = U.shape
    _, Nv, VH, VW = V.shape
    NT = Nv * k * k
    S = wgrad_splits(B, Mu, NT, PH * PW, rt.lib().ffc_conv_wgrad_tile(Mu, NT))
    dW = torch.empty(dW_shape, device=U.device, dtype=torch.float32)
    if dW.numel() != Mu * NT:
        raise FFCError(f"weight gradient shape {dW_shape} != ({Mu}, {Nv}, {k}, {k})")
    ws = torch.empty(S * Mu * NT, device=U.device, dtype=torch.float32) if S > 1 else None
    with rt.observe("wgrad", flops=2.0 * B * Mu * NT * PH * PW):
        check(rt.lib().ffc_conv_wgrad(ptr(U), Mu, PH, PW, ptr(V), Nv, VH, VW, B, k, s, p, d, S, ptr(ws), ptr(dW), 0,
                                      _stream(U)), "ffc_conv_wgrad")
    return dW


def reduce_ws(x):
    """the split count (ffc_reduce_splits) of the per-channel reductions over x (B, C, ...) and their fp64 workspace"""
    B, C = x.shape[:2]
    S = rt.lib().ffc_reduce_splits(B, C, x[0, 0].numel())
    return S, torch.empty(S * C * 2, device=x.device, dtype=torch.float64)


def channel_moments(x):
    """fp64 raw moments [C][3] {n, sum x, sum x^2} of x (B, C, ...) per channel (ffc_channel_moments)"""
    B, C = x.shape[:2]
    S, ws = reduce_ws(x)
    mom = torch.empty((C, 3), device=x.device, dtype=torch.float64)
    check(rt.lib().ffc_channel_moments(ptr(x), B, C, x[0, 0].numel(), ptr(ws), S, ptr(mom), _stream(x)),
          "ffc_channel_moments")
    return mom


def channel_sum(g):
    """sum over (B, H, W) per channel (bias gradient)"""
    return channel_moments(g)[:, 1].float()


# --------------------------------------------------------------------------- conv layer (ffc::conv_layer)
# spec (JSON): {"outs": [[M, act, param], ...], "edges": [[j, i, kind, k, s, p, d, op, layout, bias], ...]}:
# output j = act_j(sum over its edges of conv(kind, k, s, p, d, op)(xs[i]) with ws[e] (+ bs[bias])).
# Shapes come from the tensors, so one spec serves every batch size.
# plans / packed weights of every conv_layer op, keyed by (spec, shapes): a pool of caches, each
# held by one caller at a time (rt.StreamPool: a plan's packed weights and split-K partials are
# written on its holder's stream)
_CL_POOL = rt.StreamPool(dict)


@functools.lru_cache(maxsize=4096)
def parse_conv_spec(spec: str):
    d = json.loads(spec)
    return [tuple(o) for o in d["outs"]], [tuple(e) for e in d["edges"]]


@functools.lru_cache(maxsize=4096)
def parse_conv_adds(spec: str):
    """{output j: input i}: xs[i] (the output's shape, no edge reads it) is added to output j before its
    activation -- a residual block's identity shortcut (the kernels' ``addend``)"""
    return {int(j): int(i) for j, i in json.loads(spec).get("adds", ())}


def conv_spec(outs, edges, adds=None) -> str:
    """outs: [(M, act, param)]; edges: [(j, i, Seg, layout, bias index or -1)]; adds: [(j, i)] (parse_conv_adds)
    -> spec string"""
    d = {"outs": [[int(M), int(a), float(p)] for M, a, p in outs],
         "edges": [[j, i, sg.kind, sg.k, sg.s, sg.p, sg.d, sg.op, lay, b] for j, i, sg, lay, b in edges]}
    if adds:
        d["adds"] = [[int(j), int(i)] for j, i in adds]
    return json.dumps(d, separators=(",", ":"))


def _edge_seg(e, x) -> _plan.Seg:
    _, _, kind, k, s, p, d, op, _, _ = e
    if kind == "pw":
        return _plan.Seg("pw", x.shape[1], x.shape[2], x.shape[3])
    return _plan.Seg(kind, x.shape[1], x.shape[2], x.shape[3], k, s, p, d, op)


def conv_layer_out_shape(e, x, M):
    """output shape of edge e (spec tuple) applied to x with M output channels (works on SymInts)"""
    _, _, kind, k, s, p, d, op, _, _ = e
    B, _, H, W = x.shape
    if kind == "conv":
        return (B, M, _plan.conv_out(H, k, s, p, d), _plan.conv_out(W, k, s, p, d))
    if kind == "convT":
        return (B, M, _plan.convT_out(H, k, s, p, d, op), _plan.convT_out(W, k, s, p, d, op))
    return (B, M, H, W)


def conv_layer_impl(xs, ws, bs, spec):
    """ffc::conv_layer: -> outputs, then the pre-activation of every GELU output (the backward's input)"""
    outs_s, edges = parse_conv_spec(spec)
    adds = parse_conv_adds(spec)
    rt.note_tensors(list(ws) + list(bs))
    xs = [rt.require(x, "conv_layer input") for x in xs]
    ws = [rt.require(w, "conv_layer weight") for w in ws]
    bs = [rt.require(b, "conv_layer bias") for b in bs]
    B = xs[0].shape[0]
    segs = [_edge_seg(e, xs[e[1]]) for e in edges]
    outs, pres = [], []
    for j, (M, act, param) in enumerate(outs_s):
        es = [e for e in range(len(edges)) if edges[e][0] == j]
        sgs = tuple(segs[e] for e in es)
        wts = [rt.ConvWeight(ws[e], edges[e][8], edges[e][3], edges[e][3],
                             bs[edges[e][9]] if edges[e][9] >= 0 else None) for e in es]
        fused = act if act != 5 else 0
        addend = None
        if j in adds:
            addend = xs[adds[j]]
            if any(ed[1] == adds[j] for ed in edges):
                raise NotImplementedError("conv_layer: an input that is an addend may feed no edge of the same op")
            if tuple(addend.shape) != tuple(conv_layer_out_shape(edges[es[0]], xs[edges[es[0]][1]], M)):
                raise RuntimeError(f"conv_layer: addend {tuple(addend.shape)} is not output {j}'s shape")
        with _CL_POOL.hold() as cache:
            y = conv_forward(cache, ("fwd", spec, j, B, sgs), B, M, sgs, wts, [xs[edges[e][1]] for e in es],
                             act=(fused, param), addend=addend)
        if act == 5:
            pres.append(y)
            y = _act_out(y, act, param, _stream(y))
        if RECORD is not None and act in (1, 2):   # ReLU / LeakyReLU kinks (fgan128 Discriminator)
            RECORD.append(y.detach())
        outs.append(y)
    return outs + pres


def _is_convt3_job(outs_s, edges, e, x, ws):
    """edge e is the only segment of its output and that job ran on conv_route's 'convT3' kernel: its data
    gradient then runs on ffc_convt3x3_smallm_dgrad (same switch, same caps as the forward)"""
    j = edges[e][0]
    if sum(1 for ed in edges if ed[0] == j) != 1:
        return False
    bias = x.new_empty(0) if edges[e][9] >= 0 else None
    w = rt.ConvWeight(ws[e], edges[e][8], edges[e][3], edges[e][3], bias)
    return rt.conv_route((_edge_seg(edges[e], x),), [w], outs_s[j][0], False, False, rt.TRAIN_ROUTES,
                         training=True) == "convT3"


def conv_layer_backward_impl(xs, ws, ts, gouts, needs, spec):
    """ffc::conv_layer_backward: ts[j] = output j (its pre-activation for GELU); needs: per x, w, b.
    -> [dx per x, dW per w, db per b] (empty tensors where not needed)"""
    outs_s, edges = parse_conv_spec(spec)
    n_in, ne = len(xs), len(ws)
    nb = sum(1 for e in edges if e[9] >= 0)
    gs = []
    for j, (M, act, param) in enumerate(outs_s):
        g = gouts[j]
        gs.append(None if g is None else act_backward(ts[j], g.contiguous(), act, param))
    B = xs[0].shape[0]
    grads = [xs[0].new_empty(0) for _ in range(n_in + ne + nb)]   # distinct: op outputs may not alias
    added = {i: j for j, i in parse_conv_adds(spec).items()}
    for i in range(n_in):
        if not needs[i]:
            continue
        if i in added:   # the addend's gradient is the pre-activation gradient itself (a copy: outputs may not alias)
            g = gs[added[i]]
            grads[i] = torch.zeros_like(xs[i]) if g is None else g.clone()
            continue
        es = [(e, edges[e]) for e in range(ne) if edges[e][1] == i and gs[edges[e][0]] is not None]
        x = xs[i]
        if not es:
            grads[i] = torch.zeros_like(x)
            continue
        C = x.shape[1]
        if len(es) == 1 and _is_convt3_job(outs_s, edges, es[0][0], x, ws):
            # the small-M 3x3 transposed head: its adjoint (a Conv2d from <= 4 to C channels) on the direct kernel
            e, ed = es[0]
            grads[i] = rt.convt3_dgrad(gs[ed[0]], ws[e].contiguous(), tuple(x.shape), _stream(x))
            continue
        adj = []
        for e, ed in es:
            g = gs[ed[0]]
            adj.append((e, adjoint_seg(_edge_seg(ed, x), g.shape[1], g.shape[2], g.shape[3]), ed[8], g))
        # one launch when the adjoint segments can share a job, else chained through the addend
        groups = [adj]
        try:
            _plan.plan_job(B, C, tuple(a[1] for a in adj))
        except ValueError:
            groups = [[a] for a in adj]
        dx = None
        for grp in groups:
            segs = tuple(a[1] for a in grp)
            wts = [rt.ConvWeight(ws[a[0]].contiguous(), 1 - a[2], a[1].k, a[1].k, None) for a in grp]
            key = ("adj", spec, i, tuple(a[0] for a in grp), B, C, segs)
            with _CL_POOL.hold() as cache:
                dx = conv_forward(cache, key, B, C, segs, wts, [a[3] for a in grp], out_shape=tuple(x.shape),
                                  addend=dx)
        grads[i] = dx
    for e, ed in enumerate(edges):
        j, i, kind, k, s, p, d = ed[:7]
        g = gs[j]
        if needs[n_in + e]:
            w, x = ws[e], xs[i].contiguous()
            if g is None:
                grads[n_in + e] = torch.zeros_like(w)
            elif kind == "convT":
                grads[n_in + e] = conv_wgrad(x, g, k, s, p, d, tuple(w.shape))
            else:
                grads[n_in + e] = conv_wgrad(g, x, k, s, p, d, tuple(w.shape))
        if ed[9] >= 0 and needs[n_in + ne + ed[9]]:
            grads[n_in + ne + ed[9]] = channel_sum(g) if g is not None else xs[0].new_zeros(outs_s[j][0])
    return grads


def conv_layer(B, outs, edges, inputs, adds=None):
    """the ffc::conv_layer op over modules: edges (out j, input i, Seg, module) whose weight / bias
    are the parameters (spectral norm refreshed first, as the module call would); adds [(out j, input i)]:
    inputs added to an output before its activation"""
    spec_edges, ws, bs = [], [], []
    for j, i, sg, m in edges:
        rt.sn_refresh_train(m)
        b = -1
        if m.bias is not None:
            b = len(bs)
            bs.append(m.bias)
        spec_edges.append((j, i, sg, 1 if isinstance(m, nn.ConvTranspose2d) else 0, b))
        ws.append(m.weight)
    ys = torch.ops.ffc.conv_layer(list(inputs), ws, bs, conv_spec(outs, spec_edges, adds))
    return ys[:len(outs)]


# --------------------------------------------------------------------------- BatchNorm2d + activation
def bn_normalize(x, gamma, beta, running_mean, running_var, use_batch, eps, sync):
    """nn.BatchNorm2d's normalisation of x (B, C, H, W) folded to (scale, shift), from the batch statistics when
    use_batch, else from the running ones; gamma / beta may be None.  -> (scale, shift, stats): stats = the fp64
    batch moments [C][3] {n, sum x, sum x^2} (with ``sync``: all-reduced when a SyncBN group is active), or the
    running (mean, var) [2][C]"""
    C = x.shape[1]
    scale = torch.empty(C, device=x.device, dtype=torch.float32)
    shift = torch.empty(C, device=x.device, dtype=torch.float32)
    if use_batch:
        with rt.observe("bn_moments", bytes=4.0 * x.numel()):
            stats = channel_moments(x)
        grp = rt._sync_group() if sync else None   # SyncBN: global-batch statistics
        if grp is not None:
            from .distributed import merge_moments
            merge_moments(stats, group=grp)
        running = (None, None)
    else:
        stats = torch.stack((running_mean.detach(), running_var.detach())).float().contiguous()
        running = (ptr(stats[0]), ptr(stats[1]))
    rt.bn_finalize(rt.BnArgs(C, ptr(gamma), ptr(beta), *running, None, 0, 0.1, float(eps), 1.0),
                   stats if use_batch else None, scale, shift, _stream(x))
    return scale, shift, stats


def bn_act_impl(x, gamma, beta, running_mean, running_var, use_batch, eps, act, param, up=False):
    """ffc::bn_act: y = act(BN(x)) with nn.BatchNorm2d's normalisation (batch statistics when
    use_batch, else the running ones).  -> [y, scale, shift, stats]: stats = the fp64 batch moments
    [C][3] {n, sum x, sum x^2} (all-reduced under SyncBN) with batch statistics, the running
    (mean, var) [2][C] otherwise -- the backward's input and ffc::bn_update_running's.
    ``up`` (ffc::bn_act_up2b): y = the bilinear x2 upsample of act(BN(x)) (ffc_act_up2b; act(BN(x)) itself is
    not written)"""
    x = rt.require(x, "x")
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    n_feat = running_mean.numel() if running_mean is not None else (gamma.numel() if gamma is not None else C)
    if n_feat != C:
        raise RuntimeError(f"running_mean should contain {C} elements not {n_feat}")
    scale, shift, stats = bn_normalize(x, gamma, beta, running_mean, running_var, use_batch, eps, sync=True)
    if up:
        return [act_up2b(x, scale, shift, False, act, param), scale, shift, stats]
    y = torch.empty_like(x)
    with rt.observe("bn_act", bytes=8.0 * x.numel()):
        check(rt.lib().ffc_bn_act_apply(ptr(x), ptr(y), B, C, HW, ptr(scale), ptr(shift), act, float(param),
                                        _stream(x)), "ffc_bn_act_apply")
    return [y, scale, shift, stats]


def bn_update_running_impl(running_mean, running_var, num_batches_tracked, stats, momentum, count_mult):
    """ffc::bn_update_running: running stats <- batch moments (unbiased variance), nn.BatchNorm2d's rule"""
    C = running_mean.numel()
    scratch = torch.empty(2 * C, device=running_mean.device, dtype=torch.float32)
    rt.bn_finalize(rt.BnArgs(C, None, None, ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), 1,
                             float(momentum), 1e-5, float(count_mult)),
                   stats, scratch, scratch[C:], _stream(running_mean))


def update_running(bn: nn.BatchNorm2d, stats):
    """nn.BatchNorm2d's running-statistics update of ``bn`` from the batch moments ``stats`` an op returned
    (ffc::bn_update_running), in training mode with tracked statistics only"""
    if rt.bn_mode(bn)[1]:
        torch.ops.ffc.bn_update_running(bn.running_mean, bn.running_var, bn.num_batches_tracked, stats,
                                        rt.bn_momentum(bn), 1.0)


def bn_act_backward_impl(x, dy, scale, shift, stats, gamma, use_batch, sync, eps, act, param, need_dx, has_gamma,
                         has_beta):
    """ffc::bn_act_backward -> [dx, dgamma, dbeta] (empty tensors where not needed / absent).
    x is the op's raw input (the saved tensor, not the forward's contiguous copy): the kernels read
    and write dense NCHW, so x is made contiguous here and dx is allocated NCHW-contiguous"""
    x = x.contiguous()
    dy = dy.contiguous()
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    L = rt.lib()
    S, ws = reduce_ws(x)
    coef = torch.empty(C * 3, device=x.device, dtype=torch.float32)
    dgamma = torch.empty(C, device=x.device, dtype=torch.float32) if has_gamma else None
    dbeta = torch.empty(C, device=x.device, dtype=torch.float32) if has_beta else None
    dx = torch.empty_like(x) if need_dx else None
    stream = _stream(x)
    grp = rt._sync_group() if sync else None
    if grp is not None:
        # torch.nn.SyncBatchNorm backward: dx from the all-reduced {sum g, sum g*x}, this rank's
        # own sums for dgamma / dbeta (the caller's data-parallel wrapper reduces parameter grads)
        import torch.distributed as dist
        sums = torch.empty((C, 2), device=x.device, dtype=torch.float64)
        with rt.observe("bn_bwd", bytes=8.0 * x.numel()):
            check(L.ffc_bn_bwd_sums(ptr(x), ptr(dy), B, C, HW, ptr(scale), ptr(shift), act, float(param),
                                    ptr(ws), S, ptr(sums), stream), "ffc_bn_bwd_sums")
        gsums = sums.clone()
        dist.all_reduce(gsums, group=grp)
        g = ptr(gamma) if has_gamma else None
        check(L.ffc_bn_bwd_coeff(ptr(sums), C, ptr(stats), float(eps), g, ptr(coef), ptr(dgamma), ptr(dbeta),
                                 stream), "ffc_bn_bwd_coeff")
        check(L.ffc_bn_bwd_coeff(ptr(gsums), C, ptr(stats), float(eps), g, ptr(coef), None, None, stream),
              "ffc_bn_bwd_coeff")
        if dx is not None:
            with rt.observe("bn_bwd", bytes=12.0 * x.numel()):
                check(L.ffc_bn_bwd_apply(ptr(x), ptr(dy), B, C, HW, ptr(scale), ptr(shift), act, float(param),
                                         ptr(coef), ptr(dx), stream), "ffc_bn_bwd_apply")
    else:
        with rt.observe("bn_bwd", bytes=12.0 * x.numel()):
            check(L.ffc_bn_bwd(ptr(x), ptr(dy), B, C, HW, ptr(scale), ptr(shift), act, float(param),
                               ptr(stats) if use_batch else None,
                               None if use_batch else ptr(stats[0]), None if use_batch else ptr(stats[1]),
                               float(eps), ptr(gamma) if has_gamma else None, ptr(ws), S, ptr(coef), ptr(dgamma),
                               ptr(dbeta), ptr(dx), stream), "ffc_bn_bwd")
    return [t if t is not None else x.new_empty(0) for t in (dx, dgamma, dbeta)]


RECORD = None   # tests: a list collecting every BN + activation output (kink patterns of the path)


def bn_act(bn: nn.BatchNorm2d, x, act=(0, 0.0)):
    """BatchNorm2d ``bn`` + activation on the ffc::bn_act op (the module's tensors as arguments), then
    the running-statistics update in training mode (ffc::bn_update_running)"""
    y, _, _, stats = torch.ops.ffc.bn_act(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, rt.bn_mode(bn)[0],
                                          float(bn.eps), int(act[0]), float(act[1]))
    update_running(bn, stats)
    if RECORD is not None:
        RECORD.append(y.detach())
    return y


# --------------------------------------------------------------------------- SELayer
def se_scale_impl(x, w1, w2):
    """ffc::se_scale: x * sigmoid(w2 . relu(w1 . mean_HW(x))) (hidden width w1.shape[0] may be 0)"""
    x = rt.require(x, "x")
    B, C, H, W = x.shape
    hid = w1.shape[0]
    L = rt.lib()
    stream = _stream(x)
    w1d = w1.contiguous() if hid else None
    w2d = w2.contiguous() if hid else None
    gate = torch.empty((B, C), device=x.device, dtype=torch.float32)
    with rt.observe("se_gate", bytes=4.0 * x.numel()):
        check(L.ffc_se_gate(ptr(x), B, C, H, W, 0, ptr(w1d), ptr(w2d), hid, ptr(gate), stream), "ffc_se_gate")
    zeros = torch.zeros(B * C, device=x.device, dtype=torch.float32)
    y = torch.empty_like(x)
    check(L.ffc_bn_act_apply(ptr(x), ptr(y), 1, B * C, H * W, ptr(gate), ptr(zeros), 0, 0.0, stream),
          "ffc_bn_act_apply")
    return y


def se_scale_backward_impl(x, dy, w1, w2):
    """ffc::se_scale_backward -> [dx, dw1, dw2] (x as saved by the op: made contiguous, as the forward's
    rt.require copy was)"""
    x = x.contiguous()
    dy = dy.contiguous()
    B, C, H, W = x.shape
    hid = w1.shape[0]
    dev = x.device
    dx = torch.empty_like(x)
    if not hid:   # Linear(C, 0) / Linear(0, C): empty weights get empty gradients; the gate is 0.5
        check(rt.lib().ffc_se_bwd(ptr(x), ptr(dy), B, C, H, W, None, None, 0, ptr(dx), None, None, None, None,
                                  ptr(torch.empty(4 * B * C, device=dev)), _stream(x)), "ffc_se_bwd")
        return [dx, torch.zeros_like(w1), torch.zeros_like(w2)]
    vec = lambda n: torch.empty((B, n, 1, 1), device=dev, dtype=torch.float32)  # noqa: E731
    dpre2, hact, dpre1, mean = vec(C), vec(hid), vec(hid), vec(C)
    ws = torch.empty(4 * B * C, device=dev, dtype=torch.float32)
    w1c, w2c = w1.contiguous(), w2.contiguous()
    with rt.observe("se_bwd", bytes=16.0 * x.numel()):
        check(rt.lib().ffc_se_bwd(ptr(x), ptr(dy), B, C, H, W, ptr(w1c), ptr(w2c), hid, ptr(dx), ptr(dpre2), ptr(hact),
                                  ptr(dpre1), ptr(mean), ptr(ws), _stream(x)), "ffc_se_bwd")
    dw1 = conv_wgrad(dpre1, mean, 1, 1, 0, 1, (hid, C))      # fc.0: (hid, C)
    dw2 = conv_wgrad(dpre2, hact, 1, 1, 0, 1, (C, hid))      # fc.2: (C, hid)
    return [dx, dw1, dw2]


def se_layer(se, x):
    if se.fc[0].bias is not None or se.fc[2].bias is not None:
        raise NotImplementedError("SELayer with bias")
    return torch.ops.ffc.se_scale(x, se.fc[0].weight, se.fc[2].weight)


# --------------------------------------------------------------------------- pool / upsample
def pool2_impl(x, scale):
    """ffc::pool2: scale * (sum of each 2x2 block) -- AvgPool2d(2, 2) at scale 0.25 (spectral_transform.py:46-47)"""
    x = rt.require(x, "x")
    B, C, H, W = x.shape
    if H % 2 or W % 2:
        raise NotImplementedError("AvgPool2d(2) downsample of an odd-sized input")
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=torch.float32)
    check(rt.lib().ffc_pool2(ptr(x), B * C, H, W, float(scale), ptr(y), _stream(x)), "ffc_pool2")
    return y


def up2_impl(x, scale):
    """ffc::up2: scale * nearest x2 -- Upsample(scale_factor=2, mode='nearest') at scale 1 (:44-45)"""
    x = rt.require(x, "x")
    B, C, h, w = x.shape
    y = torch.empty((B, C, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
    check(rt.lib().ffc_up2(ptr(x), B * C, h, w, float(scale), ptr(y), _stream(x)), "ffc_up2")
    return y


def act_impl(x, act, param):
    """ffc::act: y = act(x) out of place (ReLU .. Sigmoid: the backward reads the output).  DBlock's leading
    nn.ReLU(True) without touching the caller's tensor"""
    x = rt.require(x, "x")
    if x.dim() != 4 or not 1 <= act <= 4:
        raise NotImplementedError(f"ffc::act: a (B, C, H, W) tensor and ReLU / LeakyReLU / Tanh / Sigmoid, got "
                                  f"{tuple(x.shape)}, act {act}")
    return _act_out(x, act, param, _stream(x))


def act_up2b(x, scale, shift, per_sample, act, param):
    """up2_bilinear(act(scale * x + shift)) on ffc_act_up2b (x dense NCHW on the GPU; scale / shift (C), (B, C)
    with per_sample, or None)"""
    B, C, h, w = x.shape
    y = torch.empty((B, C, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
    with rt.observe("act_up2b", bytes=20.0 * x.numel()):
        check(rt.lib().ffc_act_up2b(ptr(x), ptr(scale), ptr(shift), 1 if per_sample else 0, B, C, h, w, int(act),
                                    float(param), ptr(y), _stream(x)), "ffc_act_up2b")
    return y


def up2_bilinear_impl(x, scale, shift, act, param):
    """ffc::up2_bilinear: F.interpolate(act(scale * x + shift), scale_factor=2, mode='bilinear',
    align_corners=False); scale / shift: (C,) per channel, (B, C) per sample and channel, or None"""
    x = rt.require(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"up2_bilinear: x must be (B, C, h, w), got {tuple(x.shape)}")
    B, C = x.shape[:2]
    if (scale is None) != (shift is None):
        raise RuntimeError("up2_bilinear: scale and shift go together")
    per_sample = False
    if scale is not None:
        scale, shift = rt.require(scale, "scale"), rt.require(shift, "shift")
        if tuple(scale.shape) != tuple(shift.shape) or tuple(scale.shape) not in ((C,), (B, C)):
            raise RuntimeError(f"up2_bilinear: scale / shift must be ({C},) or ({B}, {C}), got "
                               f"{tuple(scale.shape)} / {tuple(shift.shape)}")
        per_sample = scale.dim() == 2
    return act_up2b(x, scale, shift, per_sample, act, param)


def up2_bilinear_adjoint_impl(dy):
    """ffc::up2_bilinear_adjoint: the transpose of the plain bilinear x2 upsample, (B, C, 2h, 2w) -> (B, C, h, w)"""
    dy = rt.require(dy, "dy")
    if dy.dim() != 4 or dy.shape[2] % 2 or dy.shape[3] % 2:
        raise RuntimeError(f"up2_bilinear_adjoint: dy must be (B, C, 2h, 2w), got {tuple(dy.shape)}")
    B, C, H, W = dy.shape
    dx = torch.empty((B, C, H // 2, W // 2), device=dy.device, dtype=torch.float32)
    with rt.observe("up2b_adjoint", bytes=5.0 * dy.numel()):
        check(rt.lib().ffc_up2b_adjoint(ptr(dy), B * C, H // 2, W // 2, ptr(dx), _stream(dy)), "ffc_up2b_adjoint")
    return dx


def pool2_act_impl(x, act, param):
    """ffc::pool2_act: act(AvgPool2d(2)(x)) in one pass (a down-sampling DBlock's output, activated for the next
    block)"""
    x = rt.require(x, "x")
    B, C, H, W = x.shape
    if H % 2 or W % 2:
        raise NotImplementedError("AvgPool2d(2) downsample of an odd-sized input")
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=torch.float32)
    with rt.observe("pool2_act", bytes=5.0 * x.numel()):
        check(rt.lib().ffc_pool2_act(ptr(x), B * C, H, W, int(act), float(param), ptr(y), _stream(x)),
              "ffc_pool2_act")
    return y


def pool2_act_backward_impl(y, dy, act, param):
    """ffc::pool2_act_backward: dx = nearest x2 of 0.25 * dy * act'(y), y the op's output"""
    y, dy = y.contiguous(), rt.require(dy, "dy")
    B, C, h, w = y.shape
    dx = torch.empty((B, C, 2 * h, 2 * w), device=y.device, dtype=torch.float32)
    with rt.observe("pool2_act_bwd", bytes=24.0 * y.numel()):
        check(rt.lib().ffc_pool2_act_bwd(ptr(y), ptr(dy), B * C, h, w, int(act), float(param), ptr(dx), _stream(y)),
              "ffc_pool2_act_bwd")
    return dx


def relu_sum_pool_impl(x):
    """ffc::relu_sum_pool: torch.sum(relu(x), (2, 3)) -> (B, C) (fgan128_complete.py:432-435)"""
    x = rt.require(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"relu_sum_pool: x must be (B, C, H, W), got {tuple(x.shape)}")
    B, C, H, W = x.shape
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    with rt.observe("relu_sum_pool", bytes=4.0 * x.numel()):
        check(rt.lib().ffc_relu_sum_pool(ptr(x), B * C, H * W, ptr(out), _stream(x)), "ffc_relu_sum_pool")
    return out


def relu_sum_pool_backward_impl(x, dout):
    """ffc::relu_sum_pool_backward: dx = (x > 0) * dout[b, c]"""
    x, dout = x.contiguous(), rt.require(dout, "dout")
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    with rt.observe("relu_sum_pool_bwd", bytes=8.0 * x.numel()):
        check(rt.lib().ffc_relu_sum_pool_bwd(ptr(x), ptr(dout), B * C, H * W, ptr(dx), _stream(x)),
              "ffc_relu_sum_pool_bwd")
    return dx


def bn_act_up2b(bn: nn.BatchNorm2d, x, act=(0, 0.0)):
    """bilinear x2 upsample of BatchNorm2d ``bn`` + activation on the ffc::bn_act_up2b op (GBlock's b1 -> ReLU ->
    F.interpolate, fgan128_complete.py:148-165), then the running-statistics update in training mode"""
    y, _, _, stats = torch.ops.ffc.bn_act_up2b(x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                               rt.bn_mode(bn)[0], float(bn.eps), int(act[0]), float(act[1]))
    update_running(bn, stats)
    return y


# --------------------------------------------------------------------------- NoiseInjection, Linear
def noise_inject_impl(x, weight, noise):
    """ffc::noise_inject: x + weight[c] * noise[b] (layers/noise_injection.py:25-32)"""
    x = rt.require(x, "x")
    B, C, H, W = x.shape
    noise = rt.require(noise, "noise")
    if tuple(noise.shape) != (B, 1, H, W) or (H * W) % 4:
        raise NotImplementedError("NoiseInjection: noise must be (B, 1, H, W) with H*W % 4 == 0")
    if weight.numel() != C:
        raise RuntimeError(f"NoiseInjection has {weight.numel()} channels, tensor has {C}")
    out = torch.empty_like(x)
    with rt.observe("noise_inject", bytes=8.0 * x.numel() + 4.0 * noise.numel()):
        check(rt.lib().ffc_noise_inject(ptr(x), ptr(weight.contiguous()), ptr(noise), ptr(out), B, C, H * W,
                                        _stream(x)), "ffc_noise_inject")
    return out


def noise_wgrad_impl(g, noise):
    """ffc::noise_wgrad: dweight[c] = sum g[:, c] * noise -> (1, C, 1, 1)"""
    g = g.contiguous()
    B, C, H, W = g.shape
    noise = noise.contiguous()   # the saved op input: a strided view (e.g. n[:, :1]) reads as dense (B, 1, H, W)
    if tuple(noise.shape) != (B, 1, H, W):
        raise RuntimeError(f"noise must be {(B, 1, H, W)}, got {tuple(noise.shape)}")
    dw = torch.empty(C, device=g.device, dtype=torch.float32)
    check(rt.lib().ffc_noise_wgrad(ptr(g), ptr(noise), B, C, H * W, ptr(dw), _stream(g)), "ffc_noise_wgrad")
    return dw.view(1, C, 1, 1)


def noise_inject(mod, x, noise=None):
    """NoiseInjection ``mod`` on the ffc::noise_inject op (noise drawn with normal_() as the reference
    does when not given)"""
    B, C, H, W = x.shape
    if noise is None:
        noise = x.new_empty(B, 1, H, W).normal_()
    return torch.ops.ffc.noise_inject(x, mod.weight, rt.require(noise, "noise"))


class _LinearAs1x1:
    """nn.Linear(K, N) seen by conv_layer as a 1x1 Conv2d on a 1x1 input: weight (N, K, 1, 1) is a view
    of the Linear's weight, so its gradient flows back to the parameter"""

    def __init__(self, lin: nn.Linear):
        self.weight = lin.weight.view(lin.out_features, lin.in_features, 1, 1)
        self.bias = lin.bias
        self.out_channels = lin.out_features


def linear(lin: nn.Linear, z):
    """nn.Linear forward + backward (fgan128_complete.py:453-455 noise_to_feature, and the spectral-norm
    fc of the fgan128 Discriminator, :540) -> (B, N)"""
    B, K = z.shape
    rt.sn_refresh_train(lin)   # the 1x1 view below must see this call's W / sigma
    (y,) = conv_layer(B, [(lin.out_features, 0, 0.0)], [(0, 0, _plan.Seg("pw", K, 1, 1), _LinearAs1x1(lin))],
                      [z.reshape(B, K, 1, 1)])
    return y.reshape(B, lin.out_features)


# --------------------------------------------------------------------------- Self_Attn
def _attn_supported(B, C, H, W, what):
    """the entry-point prefix that takes the shape: "ffc_attn" at C <= 64, "ffc_attnw" (the wide kernels) at
    72 <= C <= 256; NotImplementedError when neither does; ``what`` leads the message, up to the shape"""
    if B >= 1 and rt.lib().ffc_attn_supported(C, H, W):
        return "ffc_attn"
    if B >= 1 and rt.lib().ffc_attnw_supported(C, H, W):
        return "ffc_attnw"
    raise NotImplementedError(f"{what} {(B, C, H, W)}: the HIP attention kernels take "
                              "C % 8 == 0, 8 <= C <= 256, H * W <= 65536")


def _attn_dims(x, qkv, what):
    """(B, C, H, W, d, entry-point prefix) of a Self_Attn call; NotImplementedError naming the shape when the
    kernels refuse it"""
    if x.dim() != 4:
        raise NotImplementedError(f"{what}: x must be (B, C, H, W), got {tuple(x.shape)}")
    B, C, H, W = x.shape
    abi = _attn_supported(B, C, H, W, f"{what}: unsupported shape")
    d = C // 8
    if tuple(qkv.shape) != (B, 2 * d + C, H, W):
        raise RuntimeError(f"{what}: the stacked projection must be {(B, 2 * d + C, H, W)}, got {tuple(qkv.shape)}")
    return B, C, H, W, d, abi


def _attn_L(L, like, B, N, what):
    """the log-sum-exp rows the kernels index as L[b * N + i]"""
    if tuple(L.shape) != (B, N) or L.device != like.device:
        raise RuntimeError(f"{what}: L must be {(B, N)} on {like.device}, got {tuple(L.shape)} on {L.device}")


def _attn_gamma(gamma, what):
    if gamma.numel() != 1:
        raise RuntimeError(f"{what}: gamma must have one element, got shape {tuple(gamma.shape)}")


def _attn_rows(qkv, d, N):
    """device pointers of the q, k, v rows of the stacked projection (B, 2d + C, N)"""
    base = qkv.data_ptr()
    return base, base + 4 * d * N, base + 8 * d * N


def self_attn_impl(x, qkv, gamma, save):
    """ffc::self_attn: y = gamma * softmax(q^T k) applied to v + x from the stacked projection qkv (B, 2d + C,
    H, W) (layers/attention_layer.py:30-39) -> [y, L (B, N) log-sum-exp rows, o (B, C, N) with ``save``, else
    empty]"""
    x = rt.require(x, "x")
    qkv = rt.require(qkv, "qkv")
    gamma = rt.require(gamma, "gamma")
    B, C, H, W, d, abi = _attn_dims(x, qkv, "Self_Attn")
    _attn_gamma(gamma, "Self_Attn")
    N = H * W
    y = torch.empty_like(x)
    L = torch.empty((B, N), device=x.device, dtype=torch.float32)
    o = torch.empty((B, C, N) if save else (0,), device=x.device, dtype=torch.float32)
    q, k, v = _attn_rows(qkv, d, N)
    with rt.observe("self_attn", flops=2.0 * B * N * N * (d + C)):
        check(getattr(rt.lib(), abi + "_forward")(q, k, v, (2 * d + C) * N, ptr(x), ptr(gamma), ptr(y), ptr(L),
                                                  ptr(o) if save else None, B, C, H, W, _stream(x)),
              abi + "_forward")
    return [y, L, o]


def self_attn_matrix_impl(qkv, L, C):
    """ffc::self_attn_matrix: the attention matrix (B, N, N) = exp(S - L) from the stacked projection"""
    qkv = rt.require(qkv, "qkv")
    L = rt.require(L, "L")
    what = "Self_Attn matrix"
    if qkv.dim() != 4:
        raise RuntimeError(f"{what}: qkv must be 4-D (B, 2d + C, H, W), got {tuple(qkv.shape)}")
    B, M, H, W = qkv.shape
    abi = _attn_supported(B, C, H, W, f"{what}: unsupported shape (B, C, H, W) =")
    d, N = C // 8, H * W
    if M != 2 * d + C:
        raise RuntimeError(f"{what}: the stacked projection of C = {C} must be {(B, 2 * d + C, H, W)}, got "
                           f"{tuple(qkv.shape)}")
    _attn_L(L, qkv, B, N, what)
    P = torch.empty((B, N, N), device=qkv.device, dtype=torch.float32)
    q, k, _ = _attn_rows(qkv, d, N)
    with rt.observe("self_attn_matrix", bytes=4.0 * B * N * N):
        check(getattr(rt.lib(), abi + "_matrix")(q, k, (2 * d + C) * N, ptr(L), ptr(P), B, C, H, W, _stream(qkv)),
              abi + "_matrix")
    return P


def self_attn_bwd_impl(dy, qkv, o, L, gamma):
    """ffc::self_attn_bwd -> [dqkv (B, 2d + C, H, W), dgamma (1)] (dx of the residual is dy itself)"""
    dy = rt.require(dy, "dy")
    qkv = rt.require(qkv, "qkv")
    o = rt.require(o, "o")
    L = rt.require(L, "L")
    gamma = rt.require(gamma, "gamma")
    B, C, H, W, d, abi = _attn_dims(dy, qkv, "Self_Attn backward")
    N = H * W
    if tuple(o.shape) != (B, C, N):
        raise RuntimeError("Self_Attn backward: the forward ran without save (no attention output kept): o must be "
                           f"{(B, C, N)}, got {tuple(o.shape)}")
    _attn_L(L, dy, B, N, "Self_Attn backward")
    _attn_gamma(gamma, "Self_Attn backward")
    dqkv = torch.empty_like(qkv)
    dgamma = torch.empty(1, device=dy.device, dtype=torch.float32)
    ws = torch.empty(getattr(rt.lib(), abi + "_ws_floats")(B, C, H, W), device=dy.device, dtype=torch.float32)
    q, k, v = _attn_rows(qkv, d, N)
    dq, dk, dv = _attn_rows(dqkv, d, N)
    with rt.observe("self_attn_bwd", flops=2.0 * B * N * N * (4 * d + 3 * C)):
        check(getattr(rt.lib(), abi + "_backward")(ptr(dy), q, k, v, (2 * d + C) * N, ptr(o), ptr(L), ptr(gamma), dq,
                                                   dk, dv, (2 * d + C) * N, ptr(dgamma), ptr(ws), B, C, H, W,
                                                   _stream(dy)), abi + "_backward")
    return [dqkv, dgamma]


class _StackedQKV:
    """query_conv, key_conv and value_conv of a Self_Attn seen by conv_layer as one 1x1 Conv2d with
    2d + C outputs.  With gradients recording the stack is a fresh cat, so the gradient flows back to the
    three modules' parameters; otherwise it is kept until a parameter changes (its packed form with it)."""

    def __init__(self, mod, grad):
        ps = [mod.query_conv.weight, mod.key_conv.weight, mod.value_conv.weight,
              mod.query_conv.bias, mod.key_conv.bias, mod.value_conv.bias]
        if grad:
            self.weight, self.bias = torch.cat(ps[:3]), torch.cat(ps[3:])
        else:
            key = tuple((p.data_ptr(), p._version) for p in ps)
            hit = mod.__dict__.get("_stacked")
            if hit is None or hit[0] != key:
                with torch.no_grad():
                    hit = mod.__dict__["_stacked"] = (key, torch.cat(ps[:3]), torch.cat(ps[3:]))
            _, self.weight, self.bias = hit
        self.out_channels = self.weight.shape[0]


def self_attn(mod, x, need_attention=None):
    """Self_Attn ``mod`` on x (B, C, H, W) -> (out, attention or None): one stacked projection on the
    pointwise GEMM (ffc::conv_layer), the fused attention (ffc::self_attn), and with mod.need_attention (or the
    caller's ``need_attention`` for this call) the attention matrix (ffc::self_attn_matrix, no gradient)"""
    x = rt.require(x, "x")
    B, C, H, W = x.shape
    if C != mod.chanel_in:
        raise RuntimeError(f"Self_Attn has {mod.chanel_in} channels, tensor has {C}")
    _attn_supported(B, C, H, W, "Self_Attn: unsupported shape")
    grad = wants_grad(mod, x)
    M = 2 * (C // 8) + C
    (qkv,) = conv_layer(B, [(M, 0, 0.0)], [(0, 0, _plan.Seg("pw", C, H, W), _StackedQKV(mod, grad))], [x])
    y, L, _ = torch.ops.ffc.self_attn(x, qkv, mod.gamma, grad)
    attention = None
    if mod.need_attention if need_attention is None else need_attention:
        attention = torch.ops.ffc.self_attn_matrix(qkv.detach(), L.detach(), C)
    return y, attention


# --------------------------------------------------------------------------- FFTs
def rfft2_impl(x, mirror_scale):
    """ffc::rfft2: interleave(rfftn(x, ortho)) -> (B, 2C, H, W/2+1), mirrored bins x mirror_scale
    (2: the adjoint of irfftn at scale 1, which ffc::irfft2's backward runs)"""
    x = rt.require(x, "x")
    B, C, H, W = x.shape
    Z = torch.empty((B, 2 * C, H, W // 2 + 1), device=x.device, dtype=torch.float32)
    with rt.observe("rfft2", bytes=4.0 * x.numel() + 4.0 * Z.numel()):
        check(rt.lib().ffc_rfft2_planes(ptr(x), B * C, H, W, float(mirror_scale), ptr(Z), _stream(x)),
              "ffc_rfft2_planes")
    return Z


def irfft2_impl(Z, H, W, mirror_scale, r):
    """ffc::irfft2: irfftn(deinterleave(Z), s=(H, W), ortho) [+ r], mirrored bins x mirror_scale
    (0.5: the adjoint of rfftn at scale 1, which ffc::rfft2's backward runs)"""
    Z = rt.require(Z, "Z")
    B, C2 = Z.shape[:2]
    y = torch.empty((B, C2 // 2, H, W), device=Z.device, dtype=torch.float32)
    r = rt.require(r, "residual") if r is not None else None
    with rt.observe("irfft2", bytes=4.0 * Z.numel() + 4.0 * y.numel()):
        check(rt.lib().ffc_irfft2_planes(ptr(Z), B * (C2 // 2), H, W, float(mirror_scale), ptr(r), ptr(y),
                                         _stream(Z)), "ffc_irfft2_planes")
    return y


def fourier_unit(fu, x, residual: bool):
    """FourierUnitSN.forward (fourier_unity.py:32-56) [+ x] on the training path"""
    B, C, H, W = x.shape
    fu._check(C)
    if fu.mix_precision != "fp32":
        raise NotImplementedError("the training path computes the spectral mix in fp32 only (config 5's fp16 "
                                  "mix is forward-only)")
    if (H > 64 or W > 64) and not (H == W and H in (128,)):
        raise NotImplementedError("training-path Fourier unit: planes up to 64x64, or square 128x128")
    Z = torch.ops.ffc.rfft2(x, 1.0)
    seg = _plan.Seg("pw", 2 * C, H, W // 2 + 1)
    (U,) = conv_layer(B, [(2 * C, 0, 0.0)], [(0, 0, seg, fu.conv_layer)], [Z])
    R = bn_act(fu.bn, U, (1, 0.0))
    return torch.ops.ffc.irfft2(R, H, W, 1.0, x if residual else None)


# --------------------------------------------------------------------------- local Fourier unit (LFU)
def _lfu_dims(x, what):
    B, c, H, W = x.shape
    if c % 4 or H % 2 or W % 2 or H < 2 or W < 2:
        raise NotImplementedError(f"{what}: needs channels % 4 == 0 and even H, W; got {tuple(x.shape)}")
    return B, c, H, W


def lfu_split_impl(s):
    """ffc::lfu_split: the quadrant stack xs (B, c, H/2, W/2) of the first c/4 channels of s (B, c, H, W);
    channel blocks top-left, bottom-left, top-right, bottom-right (ffc_lfu_gather, identity transform)"""
    s = rt.require(s, "s")
    B, c, H, W = _lfu_dims(s, "lfu_split")
    xs = torch.empty((B, c, H // 2, W // 2), device=s.device, dtype=torch.float32)
    with rt.observe("lfu_gather", bytes=4.0 * (s.numel() // 4 + xs.numel())):
        check(rt.lib().ffc_lfu_gather(ptr(s), B, c, H, W, 1, None, None, 0, ptr(xs), _stream(s)), "ffc_lfu_gather")
    return xs


def lfu_split_backward_impl(dxs):
    """ffc::lfu_split_backward: ds (B, c, H, W) from dxs (B, c, H/2, W/2); zeros beyond channel c/4"""
    dxs = rt.require(dxs, "dxs")
    B, c, H2, W2 = dxs.shape
    ds = torch.empty((B, c, 2 * H2, 2 * W2), device=dxs.device, dtype=torch.float32)
    with rt.observe("lfu_gather_bwd", bytes=4.0 * (dxs.numel() + ds.numel())):
        check(rt.lib().ffc_lfu_gather_bwd(ptr(dxs), B, c, 2 * H2, 2 * W2, ptr(ds), _stream(dxs)),
              "ffc_lfu_gather_bwd")
    return ds


def lfu_tile_add_impl(v, ys, out=None):
    """ffc::lfu_tile_add: v + ys.repeat(1, 1, 2, 2) (ffc_lfu_tile_add; out=v: in place)"""
    v, ys = rt.require(v, "v"), rt.require(ys, "ys")
    B, c, H, W = _lfu_dims(v, "lfu_tile_add")
    if tuple(ys.shape) != (B, c, H // 2, W // 2):
        raise RuntimeError(f"lfu_tile_add: ys must be {(B, c, H // 2, W // 2)}, got {tuple(ys.shape)}")
    if out is None:
        out = torch.empty_like(v)
    with rt.observe("lfu_tile_add", bytes=4.0 * (2 * v.numel() + ys.numel())):
        check(rt.lib().ffc_lfu_tile_add(ptr(v), ptr(ys), B, c, H, W, ptr(out), _stream(v)), "ffc_lfu_tile_add")
    return out


def lfu_tile_backward_impl(dv):
    """ffc::lfu_tile_backward: dys (B, c, H/2, W/2) = the four quadrants of dv summed (fixed order)"""
    dv = rt.require(dv, "dv")
    B, c, H, W = _lfu_dims(dv, "lfu_tile_backward")
    dys = torch.empty((B, c, H // 2, W // 2), device=dv.device, dtype=torch.float32)
    with rt.observe("lfu_tile_bwd", bytes=4.0 * (dv.numel() + dys.numel())):
        check(rt.lib().ffc_lfu_tile_bwd(ptr(dv), B, c, H, W, ptr(dys), _stream(dv)), "ffc_lfu_tile_bwd")
    return dys


def spectral_v(st, x):
    """v = s + fu(s) [+ tile(lfu(quadrants of s)) when st.run_lfu], s = relu(bn1(conv1(se(downsample(x)))))
    (spectral_transform.py:77-108, before conv2)"""
    if st.groups != 1:
        raise NotImplementedError("grouped SpectralTransform (groups != 1) is not on the hot path")
    if st.stride == 2 and st.upsample:
        x = torch.ops.ffc.up2(x, 1.0)
    elif st.stride == 2:
        x = torch.ops.ffc.pool2(x, 0.25)
    B, Cin, H, W = x.shape
    c = st.conv1.out_channels
    if st.run_lfu:
        st.lfu_check(c, H, W)
    x = se_layer(st.se_block, x)
    (t,) = conv_layer(B, [(c, 0, 0.0)], [(0, 0, _plan.Seg("pw", Cin, H, W), st.conv1)], [x])
    s = bn_act(st.bn1, t, (1, 0.0))
    v = fourier_unit(st.fu, s, residual=True)
    if not st.run_lfu:
        return v
    ys = fourier_unit(st.lfu, torch.ops.ffc.lfu_split(s), residual=False)
    return torch.ops.ffc.lfu_tile_add(v, ys)


# --------------------------------------------------------------------------- class-conditional fgan128
def _label_tensor(labels, what):
    """class labels are a tensor on the device (never read on the host)"""
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"{what}: labels must be a tensor, got {type(labels).__name__}")
    if not labels.is_cuda:
        raise FFCError(f"{what}: labels must be on a ROCm/HIP device (there is no CPU fallback)")


def _labels(labels, B, what):
    """class labels as the kernels read them: an int64 device tensor (B,)"""
    _label_tensor(labels, what)
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != B:
        raise RuntimeError(f"{what}: labels must be int64 of shape ({B},), got {labels.dtype} {tuple(labels.shape)}")
    return labels.contiguous()


STEM_CH = 256   # channels of each stem branch (ngf * 4, fgan128_cond_complete.py:74-85)


def cond_stem_impl(z, labels, embed, w_in, b_in, w_label, b_label, gamma_in, beta_in, gamma_label, beta_label,
                   rmean_in, rvar_in, rmean_label, rvar_label, use_batch, eps):
    """ffc::cond_stem: FCondGenerator's stem (fgan128_cond_complete.py:91-101),
    cat([GELU(BN(ConvT(z))), GELU(BN(ConvT(label_embed[labels])))], 1) -> [y, pre, scale, shift, stats].
    pre: the (B, 512, 4, 4) ConvTranspose2d outputs of both branches (ffc_cond_stem_forward); scale /
    shift (512): the two BatchNorms folded; stats: the fp64 batch moments [512][3] with batch
    statistics (the input of ffc::bn_update_running and of the backward), else the running (mean, var)
    [2][512]"""
    z = rt.require(z, "z")
    B, K = z.shape
    labels = _labels(labels, B, "cond_stem")
    NC = embed.shape[0]
    C = STEM_CH
    if tuple(embed.shape) != (NC, NC) or tuple(w_in.shape) != (K, C, 4, 4) or tuple(w_label.shape) != (NC, C, 4, 4):
        raise RuntimeError(f"cond_stem: label_embed {tuple(embed.shape)}, input_conv {tuple(w_in.shape)}, "
                           f"label_conv {tuple(w_label.shape)} do not form the stem of z {tuple(z.shape)}")
    if use_batch and rt._sync_group() is not None:
        raise NotImplementedError("the conditional stem's BatchNorms have no SyncBN path (sharded conditional "
                                  "training is not supported)")
    ts = [rt.require(t.detach(), "cond_stem parameter") for t in (embed, w_in, b_in, w_label, b_label, gamma_in,
                                                                   beta_in, gamma_label, beta_label)]
    embed, w_in, b_in, w_label, b_label, gamma_in, beta_in, gamma_label, beta_label = ts
    L = rt.lib()
    dev, stream = z.device, _stream(z)
    pre = torch.empty((B, 2 * C, 4, 4), device=dev, dtype=torch.float32)
    scale = torch.empty(2 * C, device=dev, dtype=torch.float32)
    shift = torch.empty(2 * C, device=dev, dtype=torch.float32)
    slab = None
    if use_batch:
        rows = L.ffc_cond_stem_slab_rows(B)
        if L.ffc_bn_reduce_ws_doubles(rows, C):
            raise NotImplementedError(f"cond_stem: batch {B} is beyond the single-launch BN merge")
        slab = torch.empty((2, rows, C, 4), device=dev, dtype=torch.float32)
    with rt.observe("cond_stem", flops=2.0 * B * (K + NC) * C * 16):
        check(L.ffc_cond_stem_forward(ptr(z), ptr(labels), ptr(embed), ptr(w_in), ptr(b_in), ptr(w_label),
                                      ptr(b_label), B, K, NC, ptr(pre), ptr(slab), stream), "ffc_cond_stem_forward")
    if use_batch:
        from ._lib import BnRfItem
        stats = torch.empty((2 * C, 3), device=dev, dtype=torch.float64)
        arr = (BnRfItem * 2)()
        for k, (g, b) in enumerate(((gamma_in, beta_in), (gamma_label, beta_label))):
            arr[k] = BnRfItem(ptr(slab[k]), rows, C, ptr(stats[k * C:]), ptr(g), ptr(b), None, None, None, 0, 0.1,
                              float(eps), 1.0, ptr(scale[k * C:]), ptr(shift[k * C:]))
        with rt.observe("bn_stats"):
            check(L.ffc_bn_reduce_finalize_batch(arr, 2, stream), "ffc_bn_reduce_finalize_batch")
    else:
        stats = torch.stack((torch.cat((rmean_in.detach(), rmean_label.detach())),
                             torch.cat((rvar_in.detach(), rvar_label.detach())))).float().contiguous()
        for k, (g, b) in enumerate(((gamma_in, beta_in), (gamma_label, beta_label))):
            rt.bn_finalize(rt.BnArgs(C, ptr(g), ptr(b), ptr(stats[0, k * C:]), ptr(stats[1, k * C:]), None, 0, 0.1,
                                     float(eps), 1.0), None, scale[k * C:], shift[k * C:], stream)
    y = torch.empty_like(pre)
    from ._lib import BnApplyItem
    item = (BnApplyItem * 1)()
    item[0] = BnApplyItem(ptr(pre), ptr(y), B, 2 * C, 16, ptr(scale), ptr(shift), 5, 0.0, None, None, None)
    with rt.observe("bn_act", bytes=8.0 * pre.numel()):
        check(L.ffc_bn_act_apply_batch(item, 1, stream), "ffc_bn_act_apply_batch")
    return [y, pre, scale, shift, stats]


def cond_stem_backward_impl(dpre, z, labels, embed, w_in, w_label, needs):
    """ffc::cond_stem_backward: needs = [dz, d label_embed, dw_in, db_in, dw_label, db_label] -> those
    gradients (empty tensors where not needed); deterministic (ffc_cond_stem_backward)"""
    dpre = rt.require(dpre, "dpre")
    z = z.contiguous()
    B, K = z.shape
    NC = embed.shape[0]
    dev = z.device
    embed, w_in, w_label = embed.contiguous(), w_in.contiguous(), w_label.contiguous()
    shapes = [(B, K), (NC, NC), tuple(w_in.shape), (STEM_CH,), tuple(w_label.shape), (STEM_CH,)]
    outs = [torch.empty(s if n else (0,), device=dev, dtype=torch.float32) for s, n in zip(shapes, needs)]
    p = [ptr(t) if n else None for t, n in zip(outs, needs)]
    ws = torch.empty(B * NC, device=dev, dtype=torch.float32) if needs[1] else None
    with rt.observe("cond_stem_bwd", flops=2.0 * B * (K + NC) * STEM_CH * 16):
        check(rt.lib().ffc_cond_stem_backward(ptr(dpre), ptr(z), ptr(labels.contiguous()), ptr(embed), ptr(w_in),
                                              ptr(w_label), B, K, NC, p[2], p[3], p[4], p[5], p[0], p[1], ptr(ws),
                                              _stream(z)), "ffc_cond_stem_backward")
    return outs


def embed_rows_impl(weight, labels):
    """ffc::embed_rows: nn.Embedding lookup weight[labels] -> (B, D) (ffc_embed_gather_rows)"""
    weight = rt.require(weight, "label_embed.weight")
    NC, D = weight.shape
    B = labels.shape[0]
    labels = _labels(labels, B, "embed_rows")
    out = torch.empty((B, D), device=weight.device, dtype=torch.float32)
    with rt.observe("embed_gather", bytes=8.0 * out.numel()):
        check(rt.lib().ffc_embed_gather_rows(ptr(weight), ptr(labels), B, NC, D, ptr(out), _stream(weight)),
              "ffc_embed_gather_rows")
    return out


def embed_rows_backward_impl(grad, labels, num_classes):
    """ffc::embed_rows_backward: the per-class sums of the rows of grad (B, D), in sample order ->
    (num_classes, D); zeros for absent classes (ffc_embed_scatter_rows)"""
    grad = rt.require(grad, "grad")
    B, D = grad.shape
    out = torch.empty((num_classes, D), device=grad.device, dtype=torch.float32)
    with rt.observe("embed_scatter", bytes=4.0 * grad.numel() + 4.0 * out.numel()):
        check(rt.lib().ffc_embed_scatter_rows(ptr(grad), ptr(labels.contiguous()), B, num_classes, D, ptr(out),
                                              _stream(grad)), "ffc_embed_scatter_rows")
    return out


# --------------------------------------------------------------------------- conditional batch norm
def cbn_act_impl(x, labels, embed, running_mean, running_var, use_batch, eps, act, param, noise_w, noise):
    """ffc::cbn_act: y = act(BN0(x) * gamma[labels] + beta[labels]) [+ noise_w * noise], BN0 the
    affine-less nn.BatchNorm2d normalisation (batch statistics when use_batch, else the running ones)
    and (gamma | beta) the halves of embed's rows (layers/cond/cond_bn.py:16-24).
    -> [y, scale0, shift0, stats]: stats as ffc::bn_act returns them"""
    x = rt.require(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"cbn_act: x must be (B, C, H, W), got {tuple(x.shape)}")
    B, C = x.shape[:2]
    HW = x.shape[2] * x.shape[3]
    labels = _labels(labels, B, "cbn_act")
    embed = rt.require(embed.detach(), "embed.weight")
    if embed.dim() != 2 or embed.shape[1] != 2 * C:
        raise RuntimeError(f"cbn_act: embed.weight must be (num_classes, {2 * C}), got {tuple(embed.shape)}")
    if running_mean is not None and running_mean.numel() != C:
        raise RuntimeError(f"running_mean should contain {C} elements not {running_mean.numel()}")
    if use_batch and rt._sync_group() is not None:
        raise NotImplementedError("ConditionalBatchNorm2d has no SyncBN path (its backward sums would need their "
                                  "own all-reduce)")
    if (noise_w is None) != (noise is None):
        raise RuntimeError("cbn_act: noise_w and noise go together")
    if noise is not None:
        noise = rt.require(noise, "noise")
        noise_w = rt.require(noise_w.detach(), "noise weight").reshape(-1)
        if tuple(noise.shape) != (B, 1) + tuple(x.shape[2:]) or noise_w.numel() != C:
            raise RuntimeError(f"cbn_act: noise must be {(B, 1) + tuple(x.shape[2:])} with {C} weights, got "
                               f"{tuple(noise.shape)} / {noise_w.numel()}")
    scale, shift, stats = bn_normalize(x, None, None, running_mean, running_var, use_batch, eps, sync=False)
    y = torch.empty_like(x)
    from ._lib import CbnApplyItem
    item = (CbnApplyItem * 1)()
    item[0] = CbnApplyItem(ptr(x), ptr(y), B, C, HW, embed.shape[0], ptr(scale), ptr(shift), ptr(embed), ptr(labels),
                           int(act), float(param), ptr(noise_w), ptr(noise))
    with rt.observe("cbn_act", bytes=8.0 * x.numel() + (4.0 * noise.numel() if noise is not None else 0.0)):
        check(rt.lib().ffc_cbn_act_apply_batch(item, 1, _stream(x)), "ffc_cbn_act_apply_batch")
    return [y, scale, shift, stats]


def cbn_act_backward_impl(x, dy, labels, embed, scale, shift, use_batch, act, param, need_dx, need_embed):
    """ffc::cbn_act_backward -> [dx, d embed] (empty tensors where not needed).  Two passes over x and
    dy (per-sample sums, then dx); d embed is the row scatter of the sums: sample order, no atomics,
    exact zeros for classes absent from the batch"""
    x = x.contiguous()
    dy = dy.contiguous()
    B, C = x.shape[:2]
    HW = x.shape[2] * x.shape[3]
    labels = labels.contiguous()
    embed = embed.detach().contiguous()
    K = embed.shape[0]
    L = rt.lib()
    dev, stream = x.device, _stream(x)
    args = (ptr(x), ptr(dy), ptr(labels), ptr(embed), B, C, HW, K, ptr(scale), ptr(shift), int(act), float(param))
    dx = dembed = coef = None
    if need_embed or (need_dx and use_batch):
        sums = torch.empty((B, 2 * C), device=dev, dtype=torch.float32)
        with rt.observe("cbn_bwd", bytes=8.0 * x.numel()):
            check(L.ffc_cbn_bwd_sums(*args, ptr(sums), stream), "ffc_cbn_bwd_sums")
        if need_embed:
            dembed = torch.empty((K, 2 * C), device=dev, dtype=torch.float32)
            check(L.ffc_embed_scatter_rows(ptr(sums), ptr(labels), B, K, 2 * C, ptr(dembed), stream),
                  "ffc_embed_scatter_rows")
        if need_dx and use_batch:
            coef = torch.empty((C, 2), device=dev, dtype=torch.float32)
            check(L.ffc_cbn_bwd_coeff(ptr(sums), ptr(labels), ptr(embed), B, C, HW, K, ptr(coef), stream),
                  "ffc_cbn_bwd_coeff")
    if need_dx:
        dx = torch.empty_like(x)
        with rt.observe("cbn_bwd", bytes=12.0 * x.numel()):
            check(L.ffc_cbn_bwd_apply(*args, ptr(coef), ptr(dx), stream), "ffc_cbn_bwd_apply")
    return [t if t is not None else x.new_empty(0) for t in (dx, dembed)]


def cbn_labels(y, what="ConditionalBatchNorm2d"):
    """the reference's double torch.squeeze of the label argument (cond_bn.py:17-18) -> (B,) int64
    device labels; a 0-d result (B == 1) fails as the reference's chunk(2, 1) does"""
    _label_tensor(y, what)
    y = torch.squeeze(torch.squeeze(y))
    if y.dim() == 0:
        raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got 1)")
    return y


def cbn_act(cbn, x, y, act=(0, 0.0), noise=None):
    """ConditionalBatchNorm2d ``cbn`` + activation (+ the NoiseInjection (module, noise) that follows) on
    the ffc::cbn_act op, then nn.BatchNorm2d's running-statistics update in training mode"""
    bn = cbn.bn
    if bn.weight is not None:
        raise NotImplementedError("ConditionalBatchNorm2d wraps an affine-less BatchNorm2d")
    labels = cbn_labels(y)
    nw = nz = None
    if noise is not None:
        mod, nz = noise
        if nz is None:
            nz = x.new_empty(x.shape[0], 1, x.shape[2], x.shape[3]).normal_()
        nw = mod.weight
    out, _, _, stats = torch.ops.ffc.cbn_act(x, labels, cbn.embed.weight, bn.running_mean, bn.running_var,
                                             rt.bn_mode(bn)[0], float(bn.eps), int(act[0]), float(act[1]), nw, nz)
    update_running(bn, stats)
    if RECORD is not None:
        RECORD.append(out.detach())
    return out


def cond_stem(mod, z, labels):
    """FCondGenerator's stem over its modules (input_conv, label_conv, label_embed) on ffc::cond_stem,
    then nn.BatchNorm2d's running-statistics updates in training mode"""
    conv_i, bn_i, act_i = mod.input_conv
    conv_l, bn_l, act_l = mod.label_conv
    for bn in (bn_i, bn_l):
        if bn.weight is None or bn.running_mean is None:
            raise NotImplementedError("cond_stem: affine BatchNorm2d with running statistics only")
    if rt.act_code(act_i) != (5, 0.0) or rt.act_code(act_l) != (5, 0.0):
        raise NotImplementedError("cond_stem: the stem's activation is GELU")
    modes = {rt.bn_mode(bn_i), rt.bn_mode(bn_l)}
    if len(modes) != 1 or bn_i.eps != bn_l.eps:
        raise NotImplementedError("cond_stem: both stem BatchNorms must be in the same mode, with the same eps")
    use_batch, _ = modes.pop()
    y, _, _, _, stats = torch.ops.ffc.cond_stem(
        z, labels, mod.label_embed.weight, conv_i.weight, conv_i.bias, conv_l.weight, conv_l.bias, bn_i.weight,
        bn_i.bias, bn_l.weight, bn_l.bias, bn_i.running_mean, bn_i.running_var, bn_l.running_mean, bn_l.running_var,
        use_batch, float(bn_i.eps))
    for k, bn in enumerate((bn_i, bn_l)):
        update_running(bn, stats[k * STEM_CH:(k + 1) * STEM_CH])
    return y


# --------------------------------------------------------------------------- spectral norm
SN_EPS_ADD = 1   # FFC_SN_EPS_ADD of include/ffc_amd.h: normalize(x) = x / (||x|| + eps)


def sn_view(shape, dim):
    """(M, K, R, stride_m, stride_i) of SpectralNorm.reshape_weight_to_matrix read in place
    (ffc_sn_job): dim 0 is the dense (M, K) matrix, dim 1 of (d0, M, rest...) has
    Wm[m, i * R + r] = W[i, m, r] with R = prod(rest)"""
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    if len(shape) < 2 or n == 0:
        raise NotImplementedError(f"spectral norm of a weight of shape {shape}")
    if dim == 0 or (dim == 1 and shape[0] == 1):
        M = shape[dim]
        return M, n // M, n // M, n // M, 0
    if dim != 1:
        raise NotImplementedError(f"spectral norm over dim {dim} (dim 0: Conv2d / Linear, dim 1: ConvTranspose2d)")
    M = shape[1]
    R = n // (shape[0] * M)
    return M, shape[0] * R, R, R, M * R


def _sn_table(w_orig, dims, device):
    """ffc_sn_job array with the views and workspace offsets filled in, and the workspace"""
    from . import _lib
    L = rt.lib()
    jobs = (_lib.SnJob * len(w_orig))()
    off = 0
    for jb, w, dim in zip(jobs, w_orig, dims):
        jb.M, jb.K, jb.R, jb.stride_m, jb.stride_i = sn_view(w.shape, dim)
        need = L.ffc_sn_ws_bytes(jb.M, jb.K)
        if not need:
            raise NotImplementedError(f"spectral norm of a weight of shape {tuple(w.shape)}")
        jb.ws_off = off
        off += need
    return jobs, torch.empty(off, device=device, dtype=torch.uint8)


def _sn_check(ts, what, shapes=None):
    for i, t in enumerate(ts):
        rt.require(t, what)
        if not t.is_contiguous():
            raise FFCError(f"spectral norm: {what} must be contiguous")
        if shapes is not None and t.numel() != shapes[i]:
            raise RuntimeError(f"spectral norm: {what} has {t.numel()} elements, expected {shapes[i]}")


def sn_weight_impl(w_orig, u, v, w, sigma, saved, dims, training, flags=None):
    """ffc::sn_weight: the spectral_norm pre-hook of len(w_orig) layers in one table (three launches in
    training mode, two in eval mode).  Writes w[i] = w_orig[i] / sigma[i], sigma (n,), in training
    mode u[i] / v[i] in place, and -- when ``saved`` is a flat tensor of sum(M + K) floats -- this
    call's (u, v) of every layer into it, for the backward.  ``flags``: ffc_sn_job.flags per layer
    (SN_EPS_ADD: the SAGAN wrapper's x / (||x|| + eps)), None: 0 everywhere"""
    n = len(w_orig)
    if not (n and len(u) == len(v) == len(w) == len(dims) == n and sigma.numel() == n):
        raise RuntimeError("sn_weight: one (w_orig, u, v, w, dim) per layer and one sigma each")
    if flags is not None and len(flags) != n:
        raise RuntimeError("sn_weight: one flags word per layer (or none)")
    dev = w_orig[0].device
    jobs, ws = _sn_table(w_orig, dims, dev)
    _sn_check(w_orig, "weight_orig")
    _sn_check(w, "weight", [t.numel() for t in w_orig])
    _sn_check(u, "weight_u", [jb.M for jb in jobs])
    _sn_check(v, "weight_v", [jb.K for jb in jobs])
    _sn_check([sigma], "sigma")
    total = sum(jb.M + jb.K for jb in jobs)
    if saved.numel() not in (0, total):
        raise RuntimeError(f"sn_weight: saved must hold {total} floats (or none)")
    pos = saved.data_ptr()
    for i, jb in enumerate(jobs):
        jb.w_orig, jb.u, jb.v, jb.w = ptr(w_orig[i]), ptr(u[i]), ptr(v[i]), ptr(w[i])
        jb.sigma = sigma.data_ptr() + 4 * i
        jb.flags = int(flags[i]) if flags is not None else 0
        if saved.numel():
            jb.u_save, jb.v_save = pos, pos + 4 * jb.M
            pos += 4 * (jb.M + jb.K)
    nbytes = sum((12.0 if training else 8.0) * t.numel() + 4.0 * t.numel() for t in w_orig)
    with rt.observe("sn_weight", bytes=nbytes):
        check(rt.lib().ffc_sn_forward(jobs, n, 1 if training else 0, ptr(ws), ws.numel(), _stream(w_orig[0])),
              "ffc_sn_forward")


def sn_weight_bwd_impl(dw, w_orig, saved, sigma, dims):
    """ffc::sn_weight_bwd -> [dw_orig]: dw / sigma - (<dw, w_orig> / sigma^2) u v^T per layer, (u, v) the
    forward call's copies in ``saved``; two launches for the table"""
    n = len(w_orig)
    dev = w_orig[0].device
    jobs, ws = _sn_table(w_orig, dims, dev)
    dw = [g.contiguous() for g in dw]
    _sn_check(w_orig, "weight_orig")
    _sn_check(dw, "grad", [t.numel() for t in w_orig])
    if saved.numel() != sum(jb.M + jb.K for jb in jobs) or sigma.numel() != n:
        raise RuntimeError("sn_weight_bwd: saved / sigma do not match the layers")
    out = [torch.empty_like(t) for t in w_orig]
    pos = saved.data_ptr()
    for i, jb in enumerate(jobs):
        jb.w_orig, jb.dw, jb.dw_orig = ptr(w_orig[i]), ptr(dw[i]), ptr(out[i])
        jb.u, jb.v = pos, pos + 4 * jb.M
        pos += 4 * (jb.M + jb.K)
        jb.sigma = sigma.data_ptr() + 4 * i
    with rt.observe("sn_weight_bwd", bytes=sum(16.0 * t.numel() for t in w_orig)):
        check(rt.lib().ffc_sn_backward(jobs, n, ptr(ws), ws.numel(), _stream(w_orig[0])), "ffc_sn_backward")
    return out


class SnLayer(NamedTuple):
    """one layer of a SpectralNormWeight table (a plain (u, v, dim) tuple is taken as SnLayer(u, v, dim))"""
    u: torch.Tensor          # buffers: constants for autograd, advanced in place
    v: torch.Tensor
    dim: int
    flags: int = 0           # ffc_sn_job.flags (SN_EPS_ADD); the backward does not depend on it
    live: bool = False       # the backward reads u and v as they stand when it runs, not this call's copies


class SpectralNormWeight(torch.autograd.Function):
    """SpectralNorm.compute_weight for a list of layers: (weight_orig...) -> (weight...).  ``layers`` is
    [SnLayer] (or [(weight_u, weight_v, dim)]) -- buffers, constants for autograd as in the hook, advanced in
    place in training mode.  Saves weight_orig, sigma and this call's (u, v) (the kernels' own copies: the
    buffers move on at the next forward, which may come before this backward, the reason the hook
    clones them).  Backward: ffc::sn_weight_bwd over the whole list.  With ``live`` (the same for every layer of
    a table) nothing is copied and the backward takes u and v as they then stand -- what the SAGAN wrapper's
    graph does, which holds the Parameters themselves while every later forward replaces their data
    (spectral.py:30-34); it costs one concatenation of the vectors per backward."""

    @staticmethod
    def forward(ctx, layers, training, *w_orig):
        src = [w.detach() for w in w_orig]
        src = [s if s.is_contiguous() else s.contiguous() for s in src]
        layers = [l if isinstance(l, SnLayer) else SnLayer(*l) for l in layers]
        live = {bool(l.live) for l in layers}
        if len(live) != 1:
            raise NotImplementedError("spectral norm: the layers of one table save u / v alike")
        live = live.pop()
        flags = [int(l.flags) for l in layers]
        dims = [int(l.dim) for l in layers]
        out = [torch.empty_like(s) for s in src]
        sigma = torch.empty(len(src), device=src[0].device, dtype=torch.float32)
        need = any(ctx.needs_input_grad[2:]) and not live
        saved = torch.empty(sum(l.u.numel() + l.v.numel() for l in layers) if need else 0, device=src[0].device,
                            dtype=torch.float32)
        torch.ops.ffc.sn_weight(src, [l.u for l in layers], [l.v for l in layers], out, sigma, saved, dims,
                                bool(training), flags if any(flags) else None)
        ctx.dims = dims
        ctx.live = [t for l in layers for t in (l.u, l.v)] if live else None
        ctx.save_for_backward(saved, sigma, *src)
        return tuple(out)

    @staticmethod
    def backward(ctx, *dws):
        saved, sigma, *src = ctx.saved_tensors
        if ctx.live is not None:
            saved = torch.cat([t.detach().reshape(-1) for t in ctx.live])
        dws = [g if g is not None else torch.zeros_like(s) for g, s in zip(dws, src)]
        grads = torch.ops.ffc.sn_weight_bwd(dws, src, saved, sigma, ctx.dims)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


def sn_hook(mod):
    """the module's SpectralNorm pre-hook when it is switched to the HIP path (set_sn_hip), else None"""
    if not mod.__dict__.get("sn_hip"):
        return None
    from torch.nn.utils.spectral_norm import SpectralNorm
    for h in mod._forward_pre_hooks.values():
        if isinstance(h, SpectralNorm):
            return h
    return None


def sn_weights(mods, hooks):
    """refresh the spectral-norm weights of ``mods`` in one table: mod.<name> <- <name>_orig / sigma as a
    differentiable function of <name>_orig (one power iteration each in training mode)"""
    layers = [(getattr(m, h.name + "_u"), getattr(m, h.name + "_v"), h.dim) for m, h in zip(mods, hooks)]
    modes = {bool(m.training) for m in mods}
    if len(modes) != 1:
        raise NotImplementedError("spectral norm: the layers of one table must share train / eval mode")
    ws = SpectralNormWeight.apply(layers, modes.pop(), *[getattr(m, h.name + "_orig") for m, h in zip(mods, hooks)])
    for m, h, w in zip(mods, hooks, ws):
        setattr(m, h.name, w)


# --------------------------------------------------------------------------- adaptive-weight loss
AW_JOBS_PER_LAUNCH = 0   # gradient pairs per launch of ffc_aw_*: 1..16; 0: the library's 16 (tests vary the split)
AW_STATS = 8             # [rr, ff, rf, rs, fs, w_r, w_f, case]


def _aw_lists(g_real, g_fake, out=None):
    """the pointer / numel arrays of ffc_aw_* for two gradient lists (and the outputs)"""
    import ctypes
    n = len(g_real)
    if not n or len(g_fake) != n or (out is not None and len(out) != n):
        raise RuntimeError("aw: g_real, g_fake (and out) must be lists of the same non-zero length")
    lists = [g_real, g_fake] + ([out] if out is not None else [])
    for i in range(n):
        for ts, what in zip(lists, ("g_real", "g_fake", "out")):
            t = ts[i]
            rt.require(t, f"aw: {what}[{i}]")
            if not t.is_contiguous():
                raise FFCError(f"aw: {what}[{i}] must be contiguous")
            if t.numel() != g_real[i].numel() or t.device != g_real[0].device:
                raise RuntimeError(f"aw: {what}[{i}] does not match g_real[{i}] (numel, device)")
    arrays = [(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in lists]
    numel = (ctypes.c_longlong * n)(*[t.numel() for t in g_real])
    return arrays, numel, n


def aw_weights_impl(g_real, g_fake, real_validity, fake_validity, alpha1, alpha2, delta, epsilon, normalized):
    """ffc::aw_weights -> stats (8,) fp64 = [rr, ff, rf, rs, fs, w_r, w_f, case]: the dots of the two
    gradient lists per 16384-element chunk, then one workgroup for the weights of aw_loss.py:49-96
    (ceil(n / 16) + 1 launches); nothing leaves the device"""
    (pr, pf), numel, n = _aw_lists(g_real, g_fake)
    rv, fv = rt.require(real_validity, "aw: real_validity"), rt.require(fake_validity, "aw: fake_validity")
    if not (alpha1 < alpha2):
        raise RuntimeError("aw_weights: alpha1 < alpha2")
    if not rv.numel() or not fv.numel():
        raise RuntimeError("aw_weights: empty logits")
    dev = g_real[0].device
    L = rt.lib()
    nws = L.ffc_aw_ws_doubles(numel, n)
    ws = torch.empty(nws, device=dev, dtype=torch.float64)
    stats = torch.empty(AW_STATS, device=dev, dtype=torch.float64)
    with rt.observe("aw_weights", bytes=sum(8.0 * t.numel() for t in g_real)):
        check(L.ffc_aw_weights(pr, pf, numel, n, ptr(rv), rv.numel(), ptr(fv), fv.numel(), float(alpha1),
                               float(alpha2), float(delta), float(epsilon), 1 if normalized else 0,
                               AW_JOBS_PER_LAUNCH, ptr(ws), nws, ptr(stats), _stream(g_real[0])), "ffc_aw_weights")
    return stats


def aw_combine_impl(g_real, g_fake, stats, out):
    """ffc::aw_combine: out[i] <- (float)w_r * g_real[i] + (float)w_f * g_fake[i], the weights read from
    ``stats`` on the device (ceil(n / 16) launches)"""
    (pr, pf, po), numel, n = _aw_lists(g_real, g_fake, out)
    if stats.dtype != torch.float64 or stats.numel() != AW_STATS or not stats.is_contiguous() or \
            stats.device != g_real[0].device:
        raise RuntimeError("aw_combine: stats must be the (8,) fp64 tensor of aw_weights")
    with rt.observe("aw_combine", bytes=sum(12.0 * t.numel() for t in g_real)):
        check(rt.lib().ffc_aw_combine(pr, pf, po, numel, n, ptr(stats), AW_JOBS_PER_LAUNCH, _stream(g_real[0])),
              "ffc_aw_combine")


# --------------------------------------------------------------------------- fused Adam / AdamW
OPTIM_JOBS_PER_LAUNCH = 0   # entries per launch of ffc_optim_step: 1..64; 0: the library's 64 (tests vary the split)
OPTIM_STATE = 4             # int64 words of a state block: [t, s, (lr_eff, step_size), (sqrt_bc2, decay)]
OPTIM_ADAMW, OPTIM_ADAM = 0, 1


def _optim_state(state, what):
    if state.dtype != torch.int64 or not state.is_cuda or not state.is_contiguous() or not state.numel() or \
            state.numel() % OPTIM_STATE:
        raise RuntimeError(f"{what}: state must be a contiguous int64 tensor of {OPTIM_STATE} words per block on the GPU")
    return state


def optim_step_impl(params, grads, exp_avgs, exp_avg_sqs, state, lr, beta1, beta2, eps, weight_decay, decay_steps,
                    mode):
    """ffc::optim_step: t <- t + 1 in ``state`` (one block), then torch's single-tensor Adam (mode 1) / AdamW
    (mode 0) update of every (param, grad, exp_avg, exp_avg_sq) in place, lr scaled on the device by
    max(0, 1 - s / decay_steps) when decay_steps > 0 (1 + ceil(n / 64) launches); nothing leaves the device"""
    import ctypes
    n = len(params)
    lists = [params, grads, exp_avgs, exp_avg_sqs]
    if any(len(ts) != n for ts in lists):
        raise RuntimeError("optim_step: params, grads, exp_avgs and exp_avg_sqs must be lists of the same length")
    _optim_state(state, "optim_step")
    if state.numel() != OPTIM_STATE:
        raise RuntimeError("optim_step: state must be one block")
    for i in range(n):
        for ts, what in zip(lists, ("params", "grads", "exp_avgs", "exp_avg_sqs")):
            t = ts[i]
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
                raise FFCError(f"optim_step: {what}[{i}]: fp32 tensors on the GPU only")
            if not t.is_contiguous():
                raise FFCError(f"optim_step: {what}[{i}] must be contiguous")
            if t.numel() != params[i].numel() or t.device != state.device:
                raise RuntimeError(f"optim_step: {what}[{i}] does not match params[{i}] (numel) or the state's device")
    arrays = [(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in lists]
    numel = (ctypes.c_longlong * n)(*[t.numel() for t in params])
    with rt.observe("optim_step", bytes=sum(28.0 * t.numel() for t in params)):
        check(rt.lib().ffc_optim_step(*arrays, numel, n, ptr(state), float(lr), float(beta1), float(beta2), float(eps),
                                      float(weight_decay), int(decay_steps), int(mode), OPTIM_JOBS_PER_LAUNCH,
                                      _stream(state)), "ffc_optim_step")


def optim_tick_impl(state):
    """ffc::optim_tick: s <- s + 1 in every block of ``state``: scheduler.step() on the device (one launch)"""
    _optim_state(state, "optim_tick")
    with rt.observe("optim_tick", bytes=16.0 * (state.numel() // OPTIM_STATE)):
        check(rt.lib().ffc_optim_tick(ptr(state), state.numel() // OPTIM_STATE, _stream(state)), "ffc_optim_tick")
