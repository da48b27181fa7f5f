"""Timing of the spectral-norm refresh with set_sn_hip off (torch's hook: host-driven ATen) and on
(ffc::sn_weight, csrc/sn_kernels.hip) on one GPU.

    python tools/bench_sn.py [--batch 64] [--iters 200] [--json out.json]

  refresh   the refresh alone, eager, for the wrapped layers of Discriminator32(mg=4) and
            Discriminator(mg=4): forward (one power iteration + W = W_orig / sigma per layer) and
            forward + backward (a gradient for every weight_orig).  Off: the hook per layer; on: one table.
  largest   the 512 x 8192 layer alone against its byte count at 8 TB/s (three passes over W_orig and
            one write forward; two reads, one read and one write backward)
  step      training.discriminator_step and generator_step of the fgan48 pair (FGenerator32 /
            Discriminator32, mg = 6) and the fgan128 pair (FGenerator / Discriminator), batch --batch
  launches  one train-mode D forward: library launches seen by the launch observer (as
            tools/trace_launches.py counts them; one ffc::sn_weight call is three kernels) and the ATen
            operators dispatched beside them (views and metadata excluded)

Every time: warm-up, then the HIP-event time of ``--iters`` back-to-back calls divided by their number,
the median of 5 such runs (eager launches, so launch overhead is part of both sides).  One JSON line
per row on stdout."""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import _runtime as rt  # noqa: E402
from fastfourierconvolution_amd import training as T  # noqa: E402

HBM_BYTES_PER_S = 8e12
NO_KERNEL = ("view", "reshape", "permute", "transpose", "t.", "detach", "alias", "expand", "squeeze", "unsqueeze",
             "slice", "select", "as_strided", "empty", "_unsafe_view", "size", "stride", "is_", "sym_", "lift",
             "_has_", "unbind", "split", "_local_scalar")


def timed(fn, iters, runs=5, warmup=10):
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


def _quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def _layers(model):
    return [m for m in model.modules() if hasattr(m, "weight_u")]


def refresh_rows(iters):
    rows = []
    sets = [("Discriminator32(mg=4)", lambda: F.Discriminator32(True, 4)),
            ("Discriminator(mg=4)", lambda: F.Discriminator(True, 4)),
            ("512x8192 alone", lambda: torch.nn.Sequential(torch.nn.utils.spectral_norm(torch.nn.Conv2d(512, 512, 4))))]
    for name, make in sets:
        off = _quiet(make).cuda().train()
        on = F.set_sn_hip(copy.deepcopy(off))
        r = {"row": "refresh", "layers": name, "n": len(_layers(off)),
             "floats": sum(m.weight_orig.numel() for m in _layers(off))}
        for key, model in (("off", off), ("on", on)):
            mods = _layers(model)
            params = [m.weight_orig for m in mods]

            def fwd():
                with rt.sn_batch(mods):
                    for m in mods:
                        rt.sn_refresh_train(m)

            def fwd_bwd():
                fwd()
                torch.autograd.grad([m.weight for m in mods], params, [m.weight.detach() for m in mods])
            with torch.no_grad():
                r[f"fwd_{key}_ms"] = timed(fwd, iters)
            r[f"fwd_bwd_{key}_ms"] = timed(fwd_bwd, iters)
        r["fwd_speedup"] = r["fwd_off_ms"] / r["fwd_on_ms"]
        r["fwd_bwd_speedup"] = r["fwd_bwd_off_ms"] / r["fwd_bwd_on_ms"]
        if r["n"] == 1:   # the largest layer against its five passes at the HBM rate
            nbytes = 4.0 * r["floats"]
            r["fwd_bytes_floor_ms"] = 1e3 * 4 * nbytes / HBM_BYTES_PER_S
            r["fwd_bwd_bytes_floor_ms"] = 1e3 * (4 + 4) * nbytes / HBM_BYTES_PER_S
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def _pairs():
    return {"fgan48": (lambda: F.FGenerator32(128, 6), lambda: F.Discriminator32(True, 6), 48),
            "fgan128": (lambda: F.FGenerator(128), lambda: F.Discriminator(True, 4), 128)}


def step_rows(B, iters):
    rows = []
    for name, (mg, md, side) in _pairs().items():
        r = {"row": "step", "pair": name, "batch": B}
        G0, D0 = _quiet(mg).cuda().train(), _quiet(md).cuda().train()
        z = torch.randn(B, 128, device="cuda")
        real = torch.randn(B, 3, side, side, device="cuda")
        for key in ("off", "on"):
            G, D = copy.deepcopy(G0), copy.deepcopy(D0)
            F.set_sn_hip(D, key == "on")
            F.set_sn_hip(G, key == "on")
            oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
            oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
            n = max(10, iters // 10)
            r[f"d_step_{key}_ms"] = timed(lambda: T.discriminator_step(G, D, oG, oD, z, real), n, warmup=5)
            r[f"g_step_{key}_ms"] = timed(lambda: T.generator_step(G, D, oG, oD, z), n, warmup=5)
        r["d_step_speedup"] = r["d_step_off_ms"] / r["d_step_on_ms"]
        r["g_step_speedup"] = r["g_step_off_ms"] / r["g_step_on_ms"]
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


class _CountAten(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if name.startswith("aten.") and not any(name[5:].startswith(p) for p in NO_KERNEL):
            self.n += 1
        return func(*args, **(kwargs or {}))


def launch_rows(B):
    rows = []
    for name, (_, md, side) in _pairs().items():
        r = {"row": "launches", "critic": name, "batch": B}
        D0 = _quiet(md).cuda().train()
        x = torch.randn(B, 3, side, side, device="cuda")
        for key in ("off", "on"):
            D = F.set_sn_hip(copy.deepcopy(D0), key == "on")
            with torch.no_grad():
                for _ in range(3):
                    D(x)
                torch.cuda.synchronize()
                obs = rt.LaunchObserver()
                rt.set_observer(obs)
                with _CountAten() as cnt:
                    D(x)
                rt.set_observer(None)
            torch.cuda.synchronize()
            sn = sum(1 for rec in obs.records if rec[0] == "sn_weight")
            r[f"library_launches_{key}"] = len(obs.records) + 2 * sn   # one sn_weight record: three kernels
            r[f"aten_ops_{key}"] = cnt.n
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    rows = refresh_rows(args.iters) + launch_rows(args.batch) + step_rows(args.batch, args.iters)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
