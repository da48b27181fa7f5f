"""Timing of the baseline generators (Generator32, Generator64) and of their 3x3 transposed head on one GPU.

    python tools/bench_baseline.py [--batches 8 64] [--planes 32 48 64] [--model-batch 64] [--json out.json]

Three tables, one JSON line per row on stdout:
  head    the head job ConvTranspose2d(64, 3, 3, s1, p1) + bias + Tanh as one ffc::conv_layer op, forward
          (no_grad) and forward + backward (gradients of x, weight and bias), on the direct small-M kernels
          (conv_route 'convT3') against the same job with USE_SMALLM off (the implicit-GEMM kernels: the
          route of the commit before the direct kernels);
  eval    the eval forward (uint8 image) of Generator32 at mg = 4 and 6 and of Generator64 (mg = 4);
  train   generator_step + discriminator_step of the same three against Discriminator32 of the matching
          image size, each beside the FFC generator of that size (FGenerator32 at the same mg; FFCGenerator
          for the 64 x 64 image).
After a warm-up of each side, ROUNDS rounds alternate the sides of a row in one process; a round is the
HIP-event time of ``iters`` back-to-back eager calls divided by their number, with iters sized from a first
call so that a window lasts about 0.1 s (at least 3 calls).  Reported: the median and the minimum over the
rounds.  The head rows are timed twice: as eager calls (``*_ms``: at these sizes mostly the host's cost of
one custom-op call) and as replays of a hipGraph holding 20 calls (``*_graph_ms``: device time per call)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import _autograd as ag  # noqa: E402
from fastfourierconvolution_amd import _runtime as rt  # noqa: E402
from fastfourierconvolution_amd import training  # noqa: E402

from fastfourierconvolution_amd.graphs import capture_step  # noqa: E402

ROUNDS = 5
GRAPH_CALLS = 20
Z = 128


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(sides):
    """sides: {name: fn} -> {name: (median ms, min ms)}; warm-up, then alternating rounds"""
    iters = {}
    for name, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[name] = int(min(400, max(3, 100.0 / max(window(fn, 1), 1e-3))))
    times = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            times[name].append(window(fn, iters[name]))
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def head_rows(batches, planes):
    conv = nn.ConvTranspose2d(64, 3, 3, stride=1, padding=1).cuda()
    params = list(conv.parameters())
    for B in batches:
        for side in planes:
            x = torch.randn(B, 64, side, side, device="cuda", requires_grad=True)
            dy = torch.randn(B, 3, side, side, device="cuda")

            def job(smallm):
                rt.USE_SMALLM = smallm
                try:
                    (y,) = ag.conv_layer(B, [(3, 3, 0.0)], [(0, 0, rt.conv_seg(conv, x), conv)], [x])
                finally:
                    rt.USE_SMALLM = True
                return y

            def fwd(smallm):
                with torch.no_grad():
                    return job(smallm)

            def fwd_bwd(smallm):
                rt.USE_SMALLM = smallm   # the backward reads the switch too
                try:
                    (y,) = ag.conv_layer(B, [(3, 3, 0.0)], [(0, 0, rt.conv_seg(conv, x), conv)], [x])
                    return torch.autograd.grad(y, [x] + params, dy)
                finally:
                    rt.USE_SMALLM = True

            with torch.no_grad():
                a, b = fwd(True), fwd(False)
                diff = float((a - b).norm() / b.norm())
            ga, gb = fwd_bwd(True), fwd_bwd(False)
            gdiff = float((ga[0] - gb[0]).norm() / gb[0].norm())
            r = {"table": "head", "B": B, "plane": side, "out_normwise_vs_gemm": diff, "dx_normwise_vs_gemm": gdiff}
            for row, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                res = compare({"direct": lambda: run(True), "gemm": lambda: run(False)})
                for name, (med, lo) in res.items():
                    r[f"{row}_{name}_ms"], r[f"{row}_{name}_min_ms"] = med, lo
                r[f"{row}_speedup"] = r[f"{row}_gemm_ms"] / r[f"{row}_direct_ms"]
                # the eager op is host-bound at these sizes: GRAPH_CALLS calls captured into one hipGraph,
                # replayed, give the device time per call
                graphs = {name: capture_step(lambda s=s: [run(s) for _ in range(GRAPH_CALLS)])
                          for name, s in (("direct", True), ("gemm", False))}
                if all(g is not None for g in graphs.values()):
                    res = compare({name: g.replay for name, g in graphs.items()})
                    for name, (med, lo) in res.items():
                        r[f"{row}_{name}_graph_ms"], r[f"{row}_{name}_graph_min_ms"] = med / GRAPH_CALLS, lo / GRAPH_CALLS
                    r[f"{row}_graph_speedup"] = r[f"{row}_gemm_graph_ms"] / r[f"{row}_direct_graph_ms"]
                del graphs
            print(json.dumps(r), flush=True)
            yield r
            del x, dy
            torch.cuda.empty_cache()


MODELS = (("Generator32", 4, 32), ("Generator32", 6, 48), ("Generator64", 4, 64))


def randomize(mod):
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("gamma") or "noise" in k:
                p.fill_(0.5)
    return mod


def model_rows(B):
    for kind, mg, side in MODELS:
        torch.manual_seed(0)
        G = randomize(quiet(getattr(F, kind), Z, mg)).cuda()
        if side == 64:
            Gf, zf = randomize(quiet(F.FFCGenerator, Z, 3, 64)).cuda(), torch.randn(B, Z, 1, 1, device="cuda")
            fname = "FFCGenerator"
        else:
            Gf, zf = randomize(quiet(F.FGenerator32, Z, mg)).cuda(), torch.randn(B, Z, device="cuda")
            fname = "FGenerator32"
        z = torch.randn(B, Z, device="cuda")
        G.eval()

        def ev():
            with torch.no_grad():
                return G(z)
        (med, lo), = compare({"eval": ev}).values()
        r = {"table": "eval", "model": kind, "mg": mg, "image": side, "B": B, "eval_ms": med, "eval_min_ms": lo,
             "img_per_s": B / med * 1e3}
        print(json.dumps(r), flush=True)
        yield r
        real = torch.tanh(torch.randn(B, 3, side, side, device="cuda"))
        sides = {}
        for name, gen, zz in ((kind, G, z), (fname, Gf, zf)):
            gen.train()
            D = quiet(F.Discriminator32, mg=side // 8).cuda().train()
            oG = torch.optim.Adam(gen.parameters(), lr=2e-4, betas=(0.0, 0.9))
            oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))

            def step(gen=gen, D=D, oG=oG, oD=oD, zz=zz):
                training.generator_step(gen, D, oG, oD, zz)
                training.discriminator_step(gen, D, oG, oD, zz, real)
            sides[name] = step
        res = compare(sides)
        r = {"table": "train", "model": kind, "mg": mg, "image": side, "B": B, "ffc_model": fname}
        for name, (med, lo) in res.items():
            tag = "baseline" if name == kind else "ffc"
            r[f"{tag}_step_ms"], r[f"{tag}_step_min_ms"] = med, lo
        print(json.dumps(r), flush=True)
        yield r
        del G, Gf, sides
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--planes", type=int, nargs="+", default=[32, 48, 64])
    ap.add_argument("--model-batch", type=int, default=64)
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS}), flush=True)
    rows = list(head_rows(args.batches, args.planes))
    if not args.skip_models:
        rows += list(model_rows(args.model_batch))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
