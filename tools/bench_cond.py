"""Timing of the class-conditional fgan128 generator (FCondGenerator) on one GPU.

    python tools/bench_cond.py [--batches 64 512] [--replays 200] [--json out.json]

For each batch size, every workload is warmed up, captured into one hipGraph and timed with events
over ``--replays`` (>= 200) replays; the figure is the mean per replay, taken as the median of 5 such
runs.  Reported:

  cond_forward    FCondGenerator.eval() forward (uint8 image), z_size 128, 10 classes
  uncond_forward  FGenerator.eval() forward from the same run, for scale (a wider network: ngf 128)
  stem_fused      the fused stem alone (ffc::cond_stem, train mode: batch statistics + running update)
  stem_aten       the same stem as ATen ops on the same GPU: nn.Embedding + two nn.ConvTranspose2d +
                  BatchNorm2d + GELU + cat -- the yardstick the fused stem must not be slower than

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
from fastfourierconvolution_amd import _autograd as ag  # noqa: E402
from fastfourierconvolution_amd.graphs import capture_step  # noqa: E402


class AtenStem(nn.Module):
    def __init__(self, G):
        super().__init__()
        self.label_conv, self.input_conv, self.label_embed = G.label_conv, G.input_conv, G.label_embed

    def forward(self, z, labels):
        e = self.label_embed(labels).view(labels.shape[0], -1, 1, 1)
        return torch.cat([self.input_conv(z.reshape(z.size(0), -1, 1, 1)), self.label_conv(e)], dim=1)


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
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.replays < 200:
        ap.error("--replays must be >= 200")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        Gc = F.FCondGenerator(128, num_classes=10).cuda()
        Gu = F.FGenerator(128).cuda()
    aten = AtenStem(Gc)
    rows = []
    for B in args.batches:
        z = torch.randn(B, 128, device="cuda")
        labels = torch.randint(0, 10, (B,), device="cuda")
        res = {"batch": B, "replays": args.replays, "device": torch.cuda.get_device_name(0)}
        with torch.no_grad():
            Gc.eval()
            Gu.eval()
            res["cond_forward_ms"] = time_graph(lambda: Gc(z, labels), args.replays)
            res["uncond_forward_ms"] = time_graph(lambda: Gu(z), args.replays)
            Gc.train()
            res["stem_fused_ms"] = time_graph(lambda: ag.cond_stem(Gc, z, labels), args.replays)
            res["stem_aten_ms"] = time_graph(lambda: aten(z, labels), args.replays)
            err = float((ag.cond_stem(Gc, z, labels) - aten(z, labels)).abs().max())
        res["stem_max_abs_diff"] = err
        res["stem_speedup"] = res["stem_aten_ms"] / res["stem_fused_ms"]
        print(json.dumps(res), flush=True)
        rows.append(res)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
