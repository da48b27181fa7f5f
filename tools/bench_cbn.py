"""Timing of the conditional batch norm (ffc::cbn_act and its two-pass backward) and of one conditional
G + D hinge step on one GPU.

    python tools/bench_cbn.py [--batch 64] [--iters 200] [--json out.json]

Layer timings: at the local-branch shapes of FCondGenerator32's conv2..conv4 (C, side) = (192, 2mg),
(96, 4mg), (48, 8mg) for mg = 4 and mg = 6, train mode, GELU, with the NoiseInjection add:

  fused_fwd   ffc::cbn_act (batch moments + finalize + the fused conditional apply)
  aten_fwd    the same as ATen ops on the same GPU: F.batch_norm without affine, embedding lookup,
              multiply-add, F.gelu, noise add
  fused_bwd   ffc::cbn_act_backward (per-sample sums, row scatter, coefficients, dx)
  aten_bwd    torch.autograd.grad of the ATen composition w.r.t. x and the table

Step timings: training.generator_step + discriminator_step of FCondGenerator32 / FCondDiscriminator32
(labels=), and of the unconditional FGenerator32 / FDiscriminator32 pair beside it for scale.

Every figure: warm-up, then the HIP-event time of ``--iters`` back-to-back calls divided by their
number, the median of 5 such runs (eager launches; nothing here is captured into a graph, so launch
overhead is part of both sides).  One JSON line per row on stdout."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import training as T  # noqa: E402


def timed(fn, iters, runs=5, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)


def aten_cbn(x, labels, table, nw, nz):
    C = x.shape[1]
    e = TF.embedding(labels, table)
    y = TF.batch_norm(x, None, None, None, None, True, 0.1, 1e-5)
    return TF.gelu(e[:, :C, None, None] * y + e[:, C:, None, None]) + nw * nz


def layer_rows(B, iters, K=10):
    rows = []
    for mg in (4, 6):
        for C, side in ((192, 2 * mg), (96, 4 * mg), (48, 8 * mg)):
            x = torch.randn(B, C, side, side, device="cuda")
            dy = torch.randn_like(x)
            labels = torch.randint(0, K, (B,), device="cuda")
            table = torch.randn(K, 2 * C, device="cuda")
            nw = torch.randn(1, C, 1, 1, device="cuda")
            nz = torch.randn(B, 1, side, side, device="cuda")
            op = torch.ops.ffc.cbn_act
            with torch.no_grad():
                y, sc, sh, _ = op(x, labels, table, None, None, True, 1e-5, 5, 0.0, nw, nz)
                diff = float((y - aten_cbn(x, labels, table, nw, nz)).abs().max())
                r = {"mg": mg, "batch": B, "C": C, "side": side, "fwd_max_abs_diff": diff}
                r["fused_fwd_ms"] = timed(lambda: op(x, labels, table, None, None, True, 1e-5, 5, 0.0, nw, nz), iters)
                r["aten_fwd_ms"] = timed(lambda: aten_cbn(x, labels, table, nw, nz), iters)
                r["fused_bwd_ms"] = timed(lambda: torch.ops.ffc.cbn_act_backward(x, dy, labels, table, sc, sh, True, 5,
                                                                                 0.0, True, True), iters)
            xg, tg = x.clone().requires_grad_(True), table.clone().requires_grad_(True)

            def aten_fb():
                torch.autograd.grad(aten_cbn(xg, labels, tg, nw, nz), (xg, tg), dy)
            fb = timed(aten_fb, iters)
            with torch.no_grad():
                r["aten_bwd_ms"] = fb - timed(lambda: aten_cbn(xg, labels, tg, nw, nz), iters)
            r["fwd_speedup"] = r["aten_fwd_ms"] / r["fused_fwd_ms"]
            r["bwd_speedup"] = r["aten_bwd_ms"] / r["fused_bwd_ms"]
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def step_row(B, iters, K=10):
    with contextlib.redirect_stdout(io.StringIO()):
        pairs = {"cond": (F.FCondGenerator32(128, 4, K).cuda(), F.FCondDiscriminator32(True, 4, K).cuda()),
                 "uncond": (F.FGenerator32(128, 4).cuda(), F.FDiscriminator32(True, 4).cuda())}
    z = torch.randn(B, 128, device="cuda")
    real = torch.randn(B, 3, 32, 32, device="cuda")
    labels = torch.randint(0, K, (B,), device="cuda")
    r = {"batch": B, "device": torch.cuda.get_device_name(0)}
    for name, (G, D) in pairs.items():
        G.train()
        D.train()
        oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
        oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
        lab = labels if name == "cond" else None

        def step():
            T.generator_step(G, D, oG, oD, z, labels=lab)
            T.discriminator_step(G, D, oG, oD, z, real, labels=lab)
        r[name + "_gd_step_ms"] = timed(step, max(10, iters // 10), warmup=5)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    rows = layer_rows(args.batch, args.iters) + [step_row(args.batch, args.iters)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
