"""Timing of the ResNet SNGAN-128 baseline (SNGANGenerator128 / SNGANDiscriminator128) and of its resampling
kernels on one GPU.

    python tools/bench_resnet.py [--batch 64] [--ngf 1024] [--skip-models] [--json out.json]

Two tables, one JSON line per row on stdout:
  kernel  each new op at the model's own shapes (the five GBlock planes and the DBlock planes at the given ngf /
          ndf and batch) against an ATen composition of the same formula written here (F.interpolate of a
          BatchNorm-folded ReLU, its autograd backward, relu(avg_pool2d), relu().sum((2, 3))), as replays of a
          hipGraph holding GRAPH_CALLS calls (device time per call);
  model   the generator's eval forward, its train-mode forward + backward, and generator_step +
          discriminator_step of the pair, with set_sn_hip.
After a warm-up of each side, ROUNDS rounds alternate the sides of a row in one process (tools/bench_baseline.py's
scheme); reported: the median and the minimum over the rounds."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import training  # noqa: E402
from fastfourierconvolution_amd.graphs import capture_step  # noqa: E402

from bench_baseline import compare  # noqa: E402

GRAPH_CALLS = 10
ops = torch.ops.ffc


def graph_compare(sides):
    """{name: fn} -> {name: (median ms, min ms)} per call, from hipGraph replays of GRAPH_CALLS calls"""
    graphs = {}
    with torch.no_grad():
        for name, fn in sides.items():
            fn()
            graphs[name] = capture_step(lambda fn=fn: [fn() for _ in range(GRAPH_CALLS)])
    if any(g is None for g in graphs.values()):
        raise RuntimeError("capture failed")
    res = compare({name: g.replay for name, g in graphs.items()})
    return {name: (med / GRAPH_CALLS, lo / GRAPH_CALLS) for name, (med, lo) in res.items()}


def kernel_rows(B, ngf):
    rows = []
    bw = 4
    g_planes = [(ngf >> max(0, i - 1), bw << i) for i in range(5)]          # (C_in, side) of block2..block6
    d_planes = [(ngf >> (4 - i), 64 >> i) for i in range(5)]                 # (C, pooled side) of block1..block5
    for C, s in g_planes:
        x = torch.randn(B, C, s, s, device="cuda")
        sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
        g = torch.randn(B, C, 2 * s, 2 * s, device="cuda")
        cases = {
            "act_up2b": (lambda: ops.up2_bilinear(x, sc, sh, 1, 0.0),
                         lambda: Fn.interpolate(torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)),
                                                scale_factor=2, mode="bilinear", align_corners=False)),
            "up2b_adjoint": (lambda: ops.up2_bilinear_adjoint(g),
                             lambda: torch.ops.aten.upsample_bilinear2d_backward(g, [2 * s, 2 * s], [B, C, s, s], False,
                                                                                 2.0, 2.0)),
        }
        for op, (hip, aten) in cases.items():
            with torch.no_grad():
                err = float((hip() - aten()).norm() / aten().norm())
            res = graph_compare({"hip": hip, "aten": aten})
            r = {"table": "kernel", "op": op, "B": B, "C": C, "plane": s, "normwise_vs_aten": err,
                 "hip_ms": res["hip"][0], "hip_min_ms": res["hip"][1], "aten_ms": res["aten"][0],
                 "aten_min_ms": res["aten"][1], "speedup": res["aten"][0] / res["hip"][0]}
            print(json.dumps(r), flush=True)
            rows.append(r)
        del x, g
        torch.cuda.empty_cache()
    for C, s in d_planes:
        x = torch.randn(B, C, 2 * s, 2 * s, device="cuda")
        res = graph_compare({"hip": lambda: ops.pool2_act(x, 1, 0.0), "aten": lambda: torch.relu(Fn.avg_pool2d(x, 2))})
        r = {"table": "kernel", "op": "pool2_act", "B": B, "C": C, "plane": 2 * s, "hip_ms": res["hip"][0],
             "aten_ms": res["aten"][0], "speedup": res["aten"][0] / res["hip"][0]}
        print(json.dumps(r), flush=True)
        rows.append(r)
        del x
        torch.cuda.empty_cache()
    x = torch.randn(B, ngf, 4, 4, device="cuda")
    res = graph_compare({"hip": lambda: ops.relu_sum_pool(x), "aten": lambda: torch.relu(x).sum((2, 3))})
    r = {"table": "kernel", "op": "relu_sum_pool", "B": B, "C": ngf, "plane": 4, "hip_ms": res["hip"][0],
         "aten_ms": res["aten"][0], "speedup": res["aten"][0] / res["hip"][0]}
    print(json.dumps(r), flush=True)
    rows.append(r)
    return rows


def model_rows(B, ngf):
    torch.manual_seed(0)
    G = F.set_sn_hip(F.SNGANGenerator128(ngf=ngf)).cuda()
    D = F.set_sn_hip(F.SNGANDiscriminator128(ndf=ngf)).cuda()
    z = torch.randn(B, 128, device="cuda")
    real = torch.tanh(torch.randn(B, 3, 128, 128, device="cuda"))
    oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
    oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))

    def ev():
        G.eval()
        with torch.no_grad():
            return G(z)

    def fwd_bwd():
        G.train().requires_grad_(True)
        G.zero_grad()
        G(z).square().mean().backward()

    def step():
        G.train()
        training.generator_step(G, D, oG, oD, z)
        training.discriminator_step(G, D, oG, oD, z, real)

    rows = []
    for name, fn in (("generator_eval_forward", ev), ("generator_forward_backward", fwd_bwd), ("g_plus_d_step", step)):
        (med, lo), = compare({name: fn}).values()
        r = {"table": "model", "row": name, "B": B, "ngf": ngf, "ms": med, "min_ms": lo}
        print(json.dumps(r), flush=True)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ngf", type=int, default=1024)
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    rows = kernel_rows(args.batch, args.ngf)
    if not args.skip_models:
        rows += model_rows(args.batch, args.ngf)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
