"""Timing and peak memory of the wide Self_Attn (C = 256, the ffc_attnw_* kernels of csrc/attn_kernels.hip) on
one GPU against the ATen composition of the same formulas (conv2d, bmm, softmax, bmm), in the manner of
tools/bench_attn.py, whose timing loop this tool uses: both sides alternate in one process on the same inputs.

    python tools/bench_attn_wide.py [--channels 256] [--batches 64 8] [--planes 4 16 32] [--json out.json]

Planes: 4 x 4 (where the SAGAN critic's Self_Attn(256) sits), 16 x 16 and 32 x 32.  Per shape: forward (no_grad,
need_attention off) and forward + backward (gradients of x and of every parameter).  One JSON line per row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from bench_attn import ROUNDS, aten_forward, compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--planes", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    C = args.channels
    torch.manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "C": C, "rounds": ROUNDS}), flush=True)
    mod = F.Self_Attn(C, "relu").cuda()
    mod.need_attention = False
    with torch.no_grad():
        mod.gamma.fill_(0.7)
        for m in (mod.query_conv, mod.key_conv):   # scores of deviation about 1 for x ~ N(0, 1)
            m.weight.normal_(0.0, (1.0 / ((C // 8) ** 0.5 * C)) ** 0.5)
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
            r = {"B": B, "C": C, "plane": side, "N": side * side, "out_normwise_vs_aten": diff}
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
