"""Timing of the metric arithmetic on one GPU at the workload's own sizes: fidelity.FeatureStats.update,
ffc::kid_sums and ffc::isc_sums (csrc/metric_kernels.hip) against two baselines each:

  (a) host    the reference's route (torch_fidelity metric_fid.py / metric_kid.py / metric_isc.py): copy the fp32
              matrix off the GPU, then the numpy / CPU-torch restatement; one wall-clock run, the copy included
  (b) torch   a torch fp64 composition on the GPU of the same quantities (rocBLAS DGEMM for the products)

    python tools/bench_metrics.py [--n 50000] [--runs 5] [--no-host] [--json out.json]

  moments   N = 50 000 rows of D = 2048 in batches of 64 and of 1024 into one state (one "pass" = all batches)
  kid       100 subsets x 1000 rows, D = 2048, degree 3: the six sums of every subset
  isc       N = 50 000, C = 1008, 10 splits

Device times: two warm-up passes, then HIP events around one pass, the median of --runs passes (a pass is 0.01 -
1 s of back-to-back launches).  flops: 2 B D^2 per update as the dense product (the kernel computes the upper
triangle of tiles: (T + 1) / 2T of it); KID 2 m^2 D per Gram matrix, three per subset (XX and YY run (T + 1) / 2T
of their tiles).  bytes: the S2 read-modify-write, 16 D^2 per update.  One JSON line per row on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd  # noqa: E402,F401
from fastfourierconvolution_amd import fidelity as FD  # noqa: E402

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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def emit(rows, r):
    rows.append(r)
    print(json.dumps(r), flush=True)


def moments_rows(rows, N, D, runs, host):
    x = 5.0 + torch.randn(N, D, device="cuda")
    for bs in (64, 1024):
        parts = list(x.split(bs))
        st = FD.FeatureStats(D)

        def hip():
            st.state.zero_()
            for p in parts:
                st.update(p)

        n_t, piv, s1, S2 = (torch.zeros(1, device="cuda", dtype=F64), torch.zeros(D, device="cuda", dtype=F64),
                            torch.zeros(D, device="cuda", dtype=F64), torch.zeros(D, D, device="cuda", dtype=F64))

        def composed():
            S2.zero_()
            s1.zero_()
            piv.copy_(parts[0].double().mean(dim=0))
            for p in parts:
                d = p.double() - piv
                s1.add_(d.sum(dim=0))
                S2.addmm_(d.t(), d)

        med, lo, hi = timed(hip, runs)
        cmed, _, _ = timed(composed, runs)
        ups = len(parts)
        r = {"row": "moments", "N": N, "D": D, "batch": bs, "updates": ups, "hip_ms": med, "hip_ms_min": lo,
             "hip_ms_max": hi, "torch_fp64_ms": cmed, "hip_us_per_update": 1e3 * med / ups,
             "dense_tflops": 2.0 * N * D * D / (med * 1e9), "s2_rmw_tbps": 16.0 * D * D * ups / (med * 1e9),
             "vs_torch_fp64": cmed / med}
        emit(rows, r)
    if host:
        def host_route():
            f = x.cpu().numpy()
            np.mean(f, axis=0)
            np.cov(f, rowvar=False)
        emit(rows, {"row": "moments_host", "N": N, "D": D, "host_ms": wall(host_route)})


def kid_rows(rows, N, D, runs, host, subsets=100, m=1000):
    f1, f2 = torch.randn(N, D, device="cuda"), 0.1 + 1.1 * torch.randn(N, D, device="cuda")
    rng = np.random.RandomState(2020)
    idx = np.stack([np.stack([rng.choice(N, m, replace=False) for _ in range(subsets)]) for _ in range(2)])
    i1, i2 = torch.from_numpy(idx[0]).cuda(), torch.from_numpy(idx[1]).cuda()
    gamma = 1.0 / D

    def hip():
        return FD.mmd2_from_sums(torch.ops.ffc.kid_sums(f1, f2, i1, i2, 3, gamma, 1.0), m)

    def composed():
        out = []
        for s in range(subsets):
            a, b = f1[i1[s]].double(), f2[i2[s]].double()
            kxx, kyy, kxy = ((a @ a.t()) * gamma + 1.0) ** 3, ((b @ b.t()) * gamma + 1.0) ** 3, ((a @ b.t()) * gamma + 1.0) ** 3
            out.append((kxx.sum() - kxx.diagonal().sum() + kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1))
                       - 2 * kxy.sum() / (m * m))
        return torch.stack(out)

    med, lo, hi = timed(hip, runs)
    cmed, _, _ = timed(composed, runs)
    diff = float((hip() - composed()).abs().max())
    r = {"row": "kid", "N": N, "D": D, "subsets": subsets, "m": m, "hip_ms": med, "hip_ms_min": lo, "hip_ms_max": hi,
         "torch_fp64_ms": cmed, "dense_tflops": 6.0 * subsets * m * m * D / (med * 1e9), "vs_torch_fp64": cmed / med,
         "max_abs_diff_mmd2": diff}
    emit(rows, r)
    if host:
        def host_route():
            a, b = f1.cpu().numpy(), f2.cpu().numpy()
            for s in range(subsets):
                x, y = a[idx[0, s]], b[idx[1, s]]
                for p, q in ((x, x), (y, y), (x, y)):
                    ((np.matmul(p, q.T) * gamma + 1.0) ** 3).sum()
        emit(rows, {"row": "kid_host", "subsets": subsets, "m": m, "D": D, "host_ms": wall(host_route),
                    "note": "numpy keeps the features' fp32, as the reference does"})


def isc_rows(rows, N, C, runs, host, splits=10):
    lg = 3.0 * torch.randn(N, C, device="cuda")
    perm = torch.from_numpy(np.random.RandomState(2020).permutation(N)).cuda()

    def hip():
        return torch.ops.ffc.isc_sums(lg, perm, splits)[:, 3]

    def composed():
        f = lg[perm].double()
        p, logp = f.softmax(dim=1), f.log_softmax(dim=1)
        out = []
        for i in range(splits):
            pc, lc = p[i * N // splits:(i + 1) * N // splits], logp[i * N // splits:(i + 1) * N // splits]
            q = pc.mean(dim=0, keepdim=True)
            out.append((pc * (lc - q.log())).sum(dim=1).mean().exp())
        return torch.stack(out)

    med, lo, hi = timed(hip, runs)
    cmed, _, _ = timed(composed, runs)
    diff = float((hip() - composed()).abs().max())
    emit(rows, {"row": "isc", "N": N, "C": C, "splits": splits, "hip_ms": med, "hip_ms_min": lo, "hip_ms_max": hi,
                "torch_fp64_ms": cmed, "read_tbps": 4.0 * N * C / (med * 1e9), "vs_torch_fp64": cmed / med,
                "max_abs_diff_score": diff})
    if host:
        def host_route():
            f = lg.cpu()[perm.cpu()].double()
            p, logp = f.softmax(dim=1), f.log_softmax(dim=1)
            for i in range(splits):
                pc, lc = p[i * N // splits:(i + 1) * N // splits], logp[i * N // splits:(i + 1) * N // splits]
                (pc * (lc - pc.mean(dim=0, keepdim=True).log())).sum(dim=1).mean().exp().item()
        emit(rows, {"row": "isc_host", "N": N, "C": C, "host_ms": wall(host_route)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    rows = []
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    isc_rows(rows, args.n, 1008, args.runs, not args.no_host)
    moments_rows(rows, args.n, 2048, args.runs, not args.no_host)
    kid_rows(rows, args.n, 2048, args.runs, not args.no_host)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
