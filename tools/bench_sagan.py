#!/usr/bin/env python
"""Time the SAGAN baseline (fastfourierconvolution_amd.sagan, training.sagan_step) against an ATen restatement of
the same formulas on the same GPU: G forward, D forward and one hinge iteration, eager and replayed from a hipGraph,
with need_attention on and off.  B = 64, z = 128, 32 x 32.

    python tools/bench_sagan.py [--iters 50] [--warmup 10]

Prints one table row per (what, need_attention, mode): library ms, ATen ms, ATen / library.  The ATen side is
tests/sagan_refs.py-style code in fp32 (torch conv / conv_transpose / batch_norm / bmm / softmax, the wrapper's power
iteration in torch ops), the same weights on both sides."""
import argparse
import os
import sys

import torch
import torch.nn.functional as tF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import training  # noqa: E402

B, Z = 64, 128
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------ the ATen restatement (fp32, nn.Modules)
def _l2n(x):
    return x / (x.norm() + 1e-12)


def _sn_weight(m):
    w = m.weight_bar
    Wm = w.reshape(w.shape[0], -1)
    # in place, so that the addresses a captured graph holds stay valid; the graph of sigma gets copies, since an
    # in-place write to a tensor autograd saved is an error (the reference replaces .data instead)
    with torch.no_grad():
        m.weight_v.copy_(_l2n(Wm.t().mv(m.weight_u)))
        m.weight_u.copy_(_l2n(Wm.mv(m.weight_v)))
    return w / m.weight_u.detach().clone().dot(Wm.mv(m.weight_v.detach().clone()))


def _attn(a, x, need):
    b, c, h, w = x.shape
    q = tF.conv2d(x, a.query_conv.weight, a.query_conv.bias).view(b, -1, h * w).permute(0, 2, 1)
    k = tF.conv2d(x, a.key_conv.weight, a.key_conv.bias).view(b, -1, h * w)
    att = torch.softmax(torch.bmm(q, k), dim=-1)
    v = tF.conv2d(x, a.value_conv.weight, a.value_conv.bias).view(b, -1, h * w)
    out = torch.bmm(v, att.permute(0, 2, 1)).view(b, c, h, w)
    return a.gamma * out + x, (att if need else None)


def aten_G(G, z):
    x = z.view(z.size(0), z.size(1), 1, 1)
    for seq, (s, p) in zip((G.l1, G.l2, G.l3), ((1, 0), (2, 1), (2, 1))):
        m, bn = seq[0].module, seq[1]
        x = tF.conv_transpose2d(x, _sn_weight(m), m.bias, stride=s, padding=p)
        x = torch.relu(tF.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, bn.eps))
    x, p2 = _attn(G.attn2, x, G.need_attention)
    return torch.tanh(tF.conv_transpose2d(x, G.last[0].weight, G.last[0].bias, stride=2, padding=1)), p2


def aten_D(D, x):
    for seq in (D.l1, D.l2, D.l3):
        m = seq[0].module
        x = tF.leaky_relu(tF.conv2d(x, _sn_weight(m), m.bias, stride=2, padding=1), 0.1)
    x, p1 = _attn(D.attn1, x, D.need_attention)
    return tF.conv2d(x, D.last[0].weight, D.last[0].bias).squeeze(), p1


def aten_step(G, D, oG, oD, z_d, z_g, real):
    d_real, _ = aten_D(D, real)
    lr = torch.relu(1.0 - d_real).mean()
    with torch.no_grad():
        fake, _ = aten_G(G, z_d)
    d_fake, _ = aten_D(D, fake)
    lf = torch.relu(1.0 + d_fake).mean()
    oD.zero_grad(set_to_none=False)
    oG.zero_grad(set_to_none=False)
    (lr + lf).backward()
    oD.step()
    fake, _ = aten_G(G, z_g)
    out, _ = aten_D(D, fake)
    lg = -out.mean()
    oD.zero_grad(set_to_none=False)
    oG.zero_grad(set_to_none=False)
    lg.backward()
    oG.step()
    return lr, lf, lg


# ------------------------------------------------------------------ timing
def _time(fn, iters, warmup, graph):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    run = fn
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        run = g.replay
        for _ in range(3):
            run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _cell(fn, iters, warmup, graph):
    """_time, or NaN with the reason on stderr when the call cannot run in this mode (a capture torch refuses)"""
    try:
        return _time(fn, iters, warmup, graph)
    except RuntimeError as e:
        print(f"not measured ({'replay' if graph else 'eager'}): {str(e).splitlines()[0]}", file=sys.stderr)
        return float("nan")


def _models(need):
    torch.manual_seed(0)
    G, D = F.SAGANGenerator(B, 32, Z, 64).to(DEV).train(), F.SAGANDiscriminator(B, 32, 64).to(DEV).train()
    with torch.no_grad():
        G.attn2.gamma.fill_(0.5)
        D.attn1.gamma.fill_(0.5)
    G.need_attention = D.need_attention = need
    return G, D


def _adam(m, lr):
    return torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr, betas=(0.0, 0.9), capturable=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    z, z2 = torch.randn(B, Z, device=DEV), torch.randn(B, Z, device=DEV)
    real = torch.tanh(torch.randn(B, 3, 32, 32, device=DEV))
    print(f"SAGAN baseline, B = {B}, z = {Z}, 32 x 32 on {torch.cuda.get_device_name(0)}; ms per call")
    print(f"{'what':<12}{'attention':<11}{'mode':<8}{'library':>10}{'ATen':>10}{'ATen/lib':>10}")
    for need in (True, False):
        for graph in (False, True):
            rows = []
            G, D = _models(need)
            Ga, Da = _models(need)
            with torch.no_grad():
                rows.append(("G forward", _cell(lambda: G(z), a.iters, a.warmup, graph),
                             _cell(lambda: aten_G(Ga, z), a.iters, a.warmup, graph)))
                rows.append(("D forward", _cell(lambda: D(real), a.iters, a.warmup, graph),
                             _cell(lambda: aten_D(Da, real), a.iters, a.warmup, graph)))
            G, D = _models(need)
            Ga, Da = _models(need)
            oG, oD, oGa, oDa = _adam(G, 1e-4), _adam(D, 4e-4), _adam(Ga, 1e-4), _adam(Da, 4e-4)
            rows.append(("sagan_step", _cell(lambda: training.sagan_step(G, D, oG, oD, z, z2, real), a.iters, a.warmup, graph),
                         _cell(lambda: aten_step(Ga, Da, oGa, oDa, z, z2, real), a.iters, a.warmup, graph)))
            for what, lib, aten in rows:
                print(f"{what:<12}{('on' if need else 'off'):<11}{('replay' if graph else 'eager'):<8}"
                      f"{lib:>10.3f}{aten:>10.3f}{aten / lib:>10.2f}", flush=True)


if __name__ == "__main__":
    main()
