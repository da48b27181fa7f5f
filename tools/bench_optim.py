"""Timing of the fused optimizer step on one GPU: optim.FusedAdamW (csrc/optim_kernels.hip) against torch.optim.AdamW
with foreach=True, capturable=True (what bench.py --workload fgan128train captures) and with fused=True, capturable=True
where this torch build has it.

    python tools/bench_optim.py [--iters 50] [--batch 64] [--runs 2] [--json out.json]

  update   the optimizer step alone over the parameter lists of FGenerator32 + Discriminator32 (mg = 4),
           FGenerator + Discriminator (fgan128) and SNGANGenerator128 + SNGANDiscriminator128 (ngf = ndf = 1024), with
           fixed gradients: eager (launch overhead and host time included) and as replays of one captured hipGraph;
           kernels per step from torch.profiler where it reports device kernels; GB/s at 28 bytes per parameter
           (p, g, m, v read, p, m, v written) and the share of the 8 TB/s HBM spec
  step     one generator_step + discriminator_step at batch --batch with each optimizer, eager (the two smaller pairs)

Every time is the HIP-event time of --iters back-to-back calls divided by their number, the median of 5 such series
after a warm-up.  --runs N starts N fresh processes one after the other, each printing every row (a number that does
not repeat between processes is not a result).  One JSON line per row on stdout."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import training as T  # noqa: E402

HBM = 8e12
KW = dict(lr=2e-4, betas=(0.5, 0.999))


def timed(fn, iters, runs=5, warmup=5):
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


def _quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


PAIRS = {
    "fgan32": (lambda: F.FGenerator32(128, 4), lambda: F.Discriminator32(True, 4), 32),
    "fgan128": (lambda: F.FGenerator(128), lambda: F.Discriminator(True, 4), 128),
    "sngan128": (lambda: F.SNGANGenerator128(ngf=1024), lambda: F.SNGANDiscriminator128(ndf=1024), 128),
}


def shapes_of(name):
    with torch.device("meta"):
        G, D = _quiet(PAIRS[name][0]), _quiet(PAIRS[name][1])
    return [tuple(p.shape) for m in (G, D) for p in m.parameters()]


def optimizers():
    return {"foreach": lambda ps: torch.optim.AdamW(ps, foreach=True, capturable=True, **KW),
            "torch_fused": lambda ps: torch.optim.AdamW(ps, fused=True, capturable=True, **KW),
            "ffc": lambda ps: F.FusedAdamW(ps, **KW)}


def kernels_per_step(fn):
    """device kernels of one call, from torch.profiler; None where it reports none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def update_rows(iters):
    rows = []
    for name in PAIRS:
        shapes = shapes_of(name)
        floats = sum(int(torch.Size(s).numel()) for s in shapes)
        for key, make in optimizers().items():
            r = {"row": "update", "list": name, "tensors": len(shapes), "floats": floats, "optimizer": key}
            try:
                ps = [torch.nn.Parameter(0.05 * torch.randn(s, device="cuda")) for s in shapes]
                for p in ps:
                    p.grad = torch.randn_like(p)
                opt = make(ps)
                opt.step()
            except Exception as e:   # this torch build has no fused capturable AdamW on the GPU
                r["unavailable"] = f"{type(e).__name__}: {e}"[:200]
                rows.append(r)
                print(json.dumps(r), flush=True)
                continue
            n = iters if floats < 5e7 else max(5, iters // 5)
            r["eager_ms"] = timed(opt.step, n)
            r["kernels"] = kernels_per_step(opt.step)
            if key == "ffc":
                r["launches"] = 1 + -(-sum(1 for s in shapes if torch.Size(s).numel()) // 64)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                opt.step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                opt.step()
            r["graph_ms"] = timed(g.replay, n)
            r["graph_GBps"] = 28.0 * floats / (r["graph_ms"] * 1e-3) / 1e9
            r["graph_hbm_share"] = 28.0 * floats / (r["graph_ms"] * 1e-3) / HBM
            rows.append(r)
            print(json.dumps(r), flush=True)
            del g, opt, ps
            torch.cuda.empty_cache()
    for name in PAIRS:
        by = {r["optimizer"]: r for r in rows if r["list"] == name and "graph_ms" in r}
        if "ffc" in by and "foreach" in by:
            print(json.dumps({"row": "ratio", "list": name,
                              "graph_foreach_over_ffc": by["foreach"]["graph_ms"] / by["ffc"]["graph_ms"],
                              "eager_foreach_over_ffc": by["foreach"]["eager_ms"] / by["ffc"]["eager_ms"]}), flush=True)
    return rows


def step_rows(B, iters):
    rows = []
    for name in ("fgan32", "fgan128"):
        mg, md, side = PAIRS[name]
        z = torch.randn(B, 128, device="cuda")
        real = torch.randn(B, 3, side, side, device="cuda")
        r = {"row": "step", "pair": name, "batch": B}
        for key, make in optimizers().items():
            torch.manual_seed(0)
            G, D = _quiet(mg).cuda().train(), _quiet(md).cuda().train()
            try:
                oG, oD = make(list(G.parameters())), make(list(D.parameters()))
            except Exception:
                continue

            def step():
                T.generator_step(G, D, oG, oD, z)
                T.discriminator_step(G, D, oG, oD, z, real)
            try:
                r[f"{key}_ms"] = timed(step, max(5, iters // 5), warmup=3)
            except Exception as e:
                r[f"{key}_error"] = f"{type(e).__name__}: {e}"[:200]
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=1, help="fresh processes, one after the other")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.runs > 1:   # this process never touches the GPU
        for k in range(args.runs):
            print(json.dumps({"process": k + 1}), flush=True)
            cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--batch", str(args.batch)]
            if args.json:
                cmd += ["--json", f"{args.json}.{k + 1}"]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit(rc)
        return
    torch.manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
    rows = update_rows(args.iters) + step_rows(args.batch, args.iters)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
