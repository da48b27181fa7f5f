"""Timing and peak memory of Self_Attn on one GPU: the layer of this package (stacked projection on the
pointwise GEMM + the fused kernels of csrc/attn_kernels.hip, need_attention off) against an ATen
composition of the same formulas (conv2d, bmm, softmax, bmm: what the reference's code costs on the same
GPU, materialising the (B, N, N) matrix).

    python tools/bench_attn.py [--batches 64 8] [--planes 32 48 64] [--json out.json]

C = 64 throughout.  Per shape: forward (no_grad) and forward + backward (gradients of x and of every
parameter), both sides on the same random inputs (x ~ N(0, 1), scores of deviation about 1).  After a
warm-up of each side, ROUNDS rounds alternate the two sides in one process; a round is the HIP-event time
of ``iters`` back-to-back eager calls divided by their number, with iters sized from a first call so that
a window lasts about 0.2 s (at least 3 calls).  Reported: the median and the minimum over the rounds, and
torch.cuda.max_memory_allocated over one call of each side, less what was allocated before it.  One JSON
line per row on stdout."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402

ROUNDS = 5
C = 64


def aten_forward(mod, x):
    """layers/attention_layer.py:29-40 restated on ATen"""
    Fn = torch.nn.functional
    B, Cc, H, W = x.shape
    N = H * W
    q = Fn.conv2d(x, mod.query_conv.weight, mod.query_conv.bias).view(B, -1, N).permute(0, 2, 1)
    k = Fn.conv2d(x, mod.key_conv.weight, mod.key_conv.bias).view(B, -1, N)
    attention = torch.softmax(torch.bmm(q, k), dim=-1)
    v = Fn.conv2d(x, mod.value_conv.weight, mod.value_conv.bias).view(B, -1, N)
    out = torch.bmm(v, attention.permute(0, 2, 1)).view(B, Cc, H, W)
    return mod.gamma * out + x


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def compare(sides):
    """sides: {name: fn} -> {name: (median ms, min ms, peak MiB)}; warm-up, then alternating rounds"""
    iters = {}
    for name, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[name] = int(min(200, max(3, 200.0 / max(window(fn, 1), 1e-3))))
    times = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            times[name].append(window(fn, iters[name]))
    return {name: (statistics.median(t), min(t), peak_of(sides[name])) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--planes", type=int, nargs="+", default=[32, 48, 64])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "C": C, "rounds": ROUNDS}), flush=True)
    mod = F.Self_Attn(C, "relu").cuda()
    mod.need_attention = False
    with torch.no_grad():
        mod.gamma.fill_(0.7)
        for m in (mod.query_conv, mod.key_conv):   # scores of deviation about 1 for x ~ N(0, 1)
            m.weight.normal_(0.0, (1.0 / (8 ** 0.5 * C)) ** 0.5)
    params = list(mod.parameters())
    rows = []
    for B in args.batches:
        for side in args.planes:
            x = torch.randn(B, C, side, side, device="cuda", requires_grad=True)
            dy = torch.randn(B, C, side, side, device="cuda")

            def fwd(f):
                with torch.no_grad():
                    return f(x)

            def fwd_bwd(f):
                return torch.autograd.grad(f(x), [x] + params, dy)

            hip = lambda t: mod(t)[0]   # noqa: E731
            aten = lambda t: aten_forward(mod, t)   # noqa: E731
            with torch.no_grad():
                diff = float((hip(x) - aten(x)).norm() / aten(x).norm())
            r = {"B": B, "plane": side, "N": side * side, "out_normwise_vs_aten": diff}
            for row, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                res = compare({"hip": lambda: run(hip), "aten": lambda: run(aten)})
                for name, (med, lo, peak) in res.items():
                    r[f"{row}_{name}_ms"], r[f"{row}_{name}_min_ms"], r[f"{row}_{name}_peak_mib"] = med, lo, peak
                r[f"{row}_speedup"] = r[f"{row}_aten_ms"] / r[f"{row}_hip_ms"]
            rows.append(r)
            print(json.dumps(r), flush=True)
            del x, dy
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
