"""Timing of the 8*mg family (FGenerator32) and of the fused Fourier unit on its 3 * 2^k planes, one GPU.

    python tools/bench_fgan48.py [--batches 64 256] [--replays 200] [--json out.json]

Every workload is warmed up, captured into one hipGraph and timed with events over ``--replays``
(>= 200) replays; the figure is the mean per replay, taken as the median of 5 such runs (as
tools/bench_cond.py).  Per batch size:

  gen_mg6_ms / gen_mg4_ms   FGenerator32.eval() forward (uint8 image), z_size 128, 48x48 / 32x32
  fu_16x24_ms, fu_8x48_ms   FourierUnitSN in train mode on the generator's two spectral shapes, input
                            (B, 16, 12, 12) / (B, 8, 24, 24) nearest-upsampled x2 inside the kernel
                            (FourierUnitSN._run, up = 2: fused pass 0 + BN fold + pass 1)
  aten_16x24_ms, aten_8x48_ms   for comparison only: the same unit composed as the reference composes it,
                            Upsample + torch.fft.rfftn + 1x1 Conv2d + BatchNorm2d + ReLU + irfftn, ATen ops on
                            the same GPU (fourier_unity.py:32-56)

One JSON line per batch size on stdout."""
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
from fastfourierconvolution_amd.graphs import capture_step  # noqa: E402


class AtenFU(nn.Module):
    """FourierUnitSN.forward of the reference on ATen ops, after a x2 nearest Upsample"""

    def __init__(self, fu):
        super().__init__()
        self.conv_layer, self.bn = fu.conv_layer, fu.bn

    def forward(self, t):
        x = nn.functional.interpolate(t, scale_factor=2, mode="nearest")
        B, C, H, W = x.shape
        f = torch.fft.rfftn(x, dim=(-2, -1), norm="ortho")
        f = torch.stack((f.real, f.imag), dim=-1).permute(0, 1, 4, 2, 3).reshape(B, -1, H, W // 2 + 1)
        f = torch.relu(self.bn(self.conv_layer(f)))
        f = f.view(B, -1, 2, H, W // 2 + 1).permute(0, 1, 3, 4, 2).contiguous()
        return torch.fft.irfftn(torch.complex(f[..., 0], f[..., 1]), s=(H, W), dim=(-2, -1), norm="ortho")


def time_graph(step, replays, runs=5):
    """ms per replay of ``step`` captured into a hipGraph: median over ``runs`` of the event-timed mean"""
    g = capture_step(step, warmup=3)
    if g is None:
        raise RuntimeError("graph capture failed")
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / replays)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.replays < 200:
        ap.error("--replays must be >= 200")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        G6 = F.FGenerator32(128, mg=6).cuda().eval()
        G4 = F.FGenerator32(128, mg=4).cuda().eval()
    fus = {(16, 12): F.FourierUnitSN(16, 16).cuda().train(), (8, 24): F.FourierUnitSN(8, 8).cuda().train()}
    rows = []
    for B in args.batches:
        z = torch.randn(B, 128, device="cuda")
        res = {"batch": B, "replays": args.replays, "device": torch.cuda.get_device_name(0)}
        with torch.no_grad():
            res["gen_mg6_ms"] = time_graph(lambda: G6(z), args.replays)
            res["gen_mg4_ms"] = time_graph(lambda: G4(z), args.replays)
            for (C, h), fu in fus.items():
                t = torch.randn(B, C, h, h, device="cuda")
                aten = AtenFU(fu)
                tag = f"{C}x{2 * h}"
                res[f"fu_{tag}_ms"] = time_graph(lambda: fu._run(t, up=2), args.replays)
                try:
                    res[f"aten_{tag}_ms"] = time_graph(lambda: aten(t), args.replays)
                except Exception as e:   # the comparison only: ATen's FFT may refuse capture
                    res[f"aten_{tag}_ms"] = None
                    res[f"aten_{tag}_error"] = str(e)[:200]
                res[f"fu_{tag}_max_abs_diff"] = float((fu._run(t, up=2) - aten(t)).abs().max())
        print(json.dumps(res), flush=True)
        rows.append(res)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
