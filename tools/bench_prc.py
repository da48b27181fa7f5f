"""Timing of ffc::prc (csrc/prc_kernels.hip: the whole call, seven launches) on one GPU against two baselines:

  (a) torch   a torch fp64 composition on the GPU of the same quantities: three Gram products (rocBLAS DGEMM), the
              squared distances from the norms, kthvalue and any on the N x N matrices (N = 50 000: 20 GB each)
  (b) ref     at N = 10 000 only, the reference's own route (torch_fidelity metric_prc.py:47-66): torch.cdist on the
              fp32 features in batches of 10 000, every block copied to the host, kthvalue / any there; one
              wall-clock run, the copies included

    python tools/bench_prc.py [--n 10000 50000] [--d 2048 4096] [--runs 5] [--no-torch] [--no-ref] [--json out.json]

Device times: two warm-up calls, then HIP events around one call, the median of --runs calls, min and max reported.
flops: three products of 2 N^2 D each (radii of F1, radii of F2, the cross product), none of them using symmetry.
One JSON line per row on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd  # noqa: E402,F401

F64 = torch.float64


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def composed(f1, f2, k):
    """-> counts (2,) fp64 by torch ops on the GPU, everything fp64"""
    a, b = f1.double(), f2.double()
    na, nb = (a * a).sum(dim=1), (b * b).sum(dim=1)

    def radii(x, n):
        d = (n[:, None] + n[None, :] - 2.0 * (x @ x.t())).clamp_(min=0.0)
        return d.kthvalue(k + 1, dim=1).values

    r1, r2 = radii(a, na), radii(b, nb)
    d21 = (nb[:, None] + na[None, :] - 2.0 * (b @ a.t())).clamp_(min=0.0)
    hit_2 = (d21 <= r1[None, :]).any(dim=1)
    hit_1 = (d21 <= r2[:, None]).any(dim=0)
    return torch.stack([hit_2.sum(), hit_1.sum()]).double()


def reference_route(f1, f2, k, batch=10000):
    """metric_prc.py:47-66 restated for timing only"""
    def full(x, y):
        return torch.cat([torch.cat([torch.cdist(p, q).cpu() for q in y.split(batch)], dim=1) for p in x.split(batch)], dim=0)

    nn1 = full(f1, f1).kthvalue(k + 1).values
    nn2 = full(f2, f2).kthvalue(k + 1).values
    d21 = full(f2, f1)
    return (d21 <= nn1).any(dim=1).float().mean().item(), (d21.T <= nn2).any(dim=1).float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--d", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    rows = []
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    for N in args.n:
        for D in args.d:
            f1 = torch.randn(N, D, device="cuda")
            f2 = 0.05 + 1.02 * torch.randn(N, D, device="cuda")
            med, lo, hi = timed(lambda: torch.ops.ffc.prc(f1, f2, args.k), args.runs)
            counts = torch.ops.ffc.prc(f1, f2, args.k)[4]
            r = {"row": "prc", "N": N, "D": D, "k": args.k, "hip_ms": med, "hip_ms_min": lo, "hip_ms_max": hi,
                 "tflops": 6.0 * N * N * D / (med * 1e9), "counts": counts.tolist()}
            if not args.no_torch:
                cmed, clo, chi = timed(lambda: composed(f1, f2, args.k), args.runs)
                r.update(torch_fp64_ms=cmed, torch_fp64_ms_min=clo, torch_fp64_ms_max=chi, vs_torch_fp64=cmed / med,
                         counts_torch=composed(f1, f2, args.k).tolist())
            rows.append(r)
            print(json.dumps(r), flush=True)
            if not args.no_ref and N <= 10000:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p, rc = reference_route(f1, f2, args.k)
                ms = 1e3 * (time.perf_counter() - t0)
                r = {"row": "prc_ref_route", "N": N, "D": D, "k": args.k, "host_ms": ms, "precision": p, "recall": rc,
                     "note": "cdist keeps the features' fp32, as the reference does"}
                rows.append(r)
                print(json.dumps(r), flush=True)
            del f1, f2
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
