"""Cost of the local Fourier unit (LFU, set_lfu) and of its two data-movement kernels on one GPU.

    python tools/bench_lfu.py [--replays 200] [--json out.json]

Every workload is warmed up, captured into one hipGraph and timed with events over ``--replays``
(>= 200) replays; the figure is the mean per replay, taken as the median of 5 such runs.  One JSON line
per figure on stdout:

  forward   gen64 (FFCGenerator(100, 3, 64), B = 256) and fgan128 (FGenerator(128), B = 64), train-mode
            BatchNorm forward under no_grad, LFU off and on, ms per step, and the LFU planes of the run
  kernel    ffc_lfu_gather and ffc_lfu_tile_add on the largest LFU layer of each model: achieved GB/s
            over the bytes they must move, 4 (N/4 + N) for the gather and 4 (2N + N/4) for the tile-add,
            N = B c H W; beside them the same data movement composed of ATen ops on the same tensors
            (split / cat / contiguous; repeat + add) over the same byte counts
  planes    the LFU plane of every SpectralTransform of the shipped models, or the refusal they raise
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import _runtime as rt  # noqa: E402
from fastfourierconvolution_amd.graphs import capture_step  # noqa: E402


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


@contextlib.contextmanager
def record_planes(into):
    """every (c, H, W) main plane an LFU is asked to run on (lfu_check is the first thing a forward
    with run_lfu does, on the modules and on the layer ops' templates alike)"""
    orig = F.SpectralTransform.lfu_check

    def check(self, c, H, W):
        if (c, H, W) not in into:
            into.append((c, H, W))
        return orig(self, c, H, W)
    F.SpectralTransform.lfu_check = check
    try:
        yield
    finally:
        F.SpectralTransform.lfu_check = orig


def build(name):
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "gen64":
            return F.FFCGenerator(100, 3, 64), lambda B: (torch.randn(B, 100, 1, 1, device="cuda"),)
        if name == "disc64":
            return F.FFCDiscriminator(3, 64), lambda B: (torch.randn(B, 3, 64, 64, device="cuda"),)
        if name == "fgan128":
            return F.FGenerator(128), lambda B: (torch.randn(B, 128, device="cuda"),)
        if name.startswith("fgan32_mg"):
            return F.FGenerator32(128, mg=int(name[-1])), lambda B: (torch.randn(B, 128, device="cuda"),)
        if name == "fcond128":
            return F.FCondGenerator(128, num_classes=10), lambda B: (
                torch.randn(B, 128, device="cuda"), torch.randint(0, 10, (B,), device="cuda"))
    raise ValueError(name)


def forward_of(G):
    return G.forward_float if hasattr(G, "forward_float") else G


def plane_map(name, B=4):
    """LFU planes of one eager train-mode forward of model ``name`` with set_lfu, or its refusal"""
    G, inputs = build(name)
    G = F.set_lfu(G.cuda().train())
    planes, err = [], None
    with record_planes(planes), torch.no_grad():
        try:
            forward_of(G)(*inputs(B))
            torch.cuda.synchronize()
        except NotImplementedError as e:
            err = str(e)
    return {"figure": "planes", "model": name,
            "lfu_planes": [f"c={c} {H}x{W} -> {H // 2}x{W // 2}" for c, H, W in planes], "raises": err}


def bench_forward(name, B, replays):
    torch.manual_seed(0)
    G, inputs = build(name)
    G = G.cuda().train()
    x = inputs(B)
    fwd = forward_of(G)
    res = {"figure": "forward", "model": name, "batch": B, "replays": replays,
           "device": torch.cuda.get_device_name(0)}
    planes = []
    with torch.no_grad():
        res["lfu_off_ms"] = time_graph(lambda: fwd(*x), replays)
        F.set_lfu(G)
        with record_planes(planes):
            res["lfu_on_ms"] = time_graph(lambda: fwd(*x), replays)
        F.set_lfu(G, False)
        res["lfu_off_again_ms"] = time_graph(lambda: fwd(*x), replays)
    res["lfu_cost_ms"] = res["lfu_on_ms"] - 0.5 * (res["lfu_off_ms"] + res["lfu_off_again_ms"])
    res["planes"] = planes
    return res


def bench_kernels(name, B, c, H, W, replays):
    """the two kernels and their ATen compositions on one (B, c, H, W) plane"""
    L = rt.lib()
    N = B * c * H * W
    t = torch.randn(B, c, H, W, device="cuda")
    sc, sh = 1 + 0.1 * torch.randn(c, device="cuda"), 0.1 * torch.randn(c, device="cuda")
    xs = torch.empty(B, c, H // 2, W // 2, device="cuda")
    v, ys = torch.randn(B, c, H, W, device="cuda"), torch.randn(B, c, H // 2, W // 2, device="cuda")
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def gather():
        rt.check(L.ffc_lfu_gather(t.data_ptr(), B, c, H, W, 1, sc.data_ptr(), sh.data_ptr(), 1, xs.data_ptr(), st()),
                 "ffc_lfu_gather")

    def gather_plain():
        rt.check(L.ffc_lfu_gather(t.data_ptr(), B, c, H, W, 1, None, None, 0, xs.data_ptr(), st()), "ffc_lfu_gather")

    def tile_add():
        rt.check(L.ffc_lfu_tile_add(v.data_ptr(), ys.data_ptr(), B, c, H, W, v.data_ptr(), st()), "ffc_lfu_tile_add")

    def aten_split():   # the reference's sketch (:96-101) on an already activated s
        a = torch.cat(torch.split(t[:, :c // 4], H // 2, dim=-2), dim=1)
        return torch.cat(torch.split(a, W // 2, dim=-1), dim=1).contiguous()

    def aten_tile_add():
        return v.add_(ys.repeat(1, 1, 2, 2))

    gb_g, gb_t = 4.0 * (N / 4 + N) / 1e9, 4.0 * (2 * N + N / 4) / 1e9
    res = {"figure": "kernel", "model": name, "plane": [B, c, H, W], "N": N, "gather_bytes_GB": gb_g,
           "tile_add_bytes_GB": gb_t}
    with torch.no_grad():
        for key, fn, gb in (("gather", gather, gb_g), ("gather_identity", gather_plain, gb_g),
                            ("aten_split_cat", aten_split, gb_g), ("tile_add", tile_add, gb_t),
                            ("aten_repeat_add", aten_tile_add, gb_t)):
            ms = time_graph(fn, replays)
            res[key + "_ms"] = ms
            res[key + "_GBps"] = gb / (ms * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-planes", action="store_true", help="leave out the plane map of the other models")
    args = ap.parse_args()
    if args.replays < 200:
        ap.error("--replays must be >= 200")
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
    for name, B in (("gen64", 256), ("fgan128", 64)):
        r = bench_forward(name, B, args.replays)
        emit(r)
        c, H, W = max(r["planes"], key=lambda p: p[0] * p[1] * p[2])
        emit(bench_kernels(name, B, c, H, W, args.replays))
    if not args.skip_planes:
        for name in ("gen64", "disc64", "fgan128", "fcond128", "fgan32_mg4", "fgan32_mg6"):
            emit(plane_map(name))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
