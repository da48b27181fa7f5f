"""Timing of the adaptive-weight critic loss on one GPU: ffc::aw_weights + ffc::aw_combine
(csrc/aw_kernels.hip, aw_loss.aw_method) against an ATen restatement of the reference's sequence
(layers/aw_loss.py:13-107: two backward passes into .grad, clone, cat, three .item() dots, the branch in
Python on two device scores, a per-parameter combine).

    python tools/bench_aw.py [--batch 64] [--iters 200] [--json out.json]

  ops       the op pair alone on gradient lists with the parameter shapes of Discriminator32(mg=4) and
            Discriminator(mg=4) (fgan128), against the ATen sequence from the same two lists on: clone,
            cat, dots, branch, combine (its two backward passes are not part of this row)
  step      a whole critic update at batch --batch: training.aw_discriminator_step against the same two
            critic calls followed by the reference's sequence and optim_D.step()
  launches  kernels of the op pair (the launch observer's records, as tools/trace_launches.py counts
            them: one aw_weights record is ceil(n / 16) + 1 kernels, one aw_combine record ceil(n / 16))
            and the ATen operators the reference's sequence dispatches from the two lists on (views and
            metadata excluded), with its host synchronisations (.item() and bool() of a device tensor)

Every time: warm-up, then the HIP-event time of ``--iters`` back-to-back calls divided by their number,
the median of 5 such runs (eager launches, so launch overhead and host round trips are part of both
sides).  One JSON line per row on stdout."""
import argparse
import contextlib
import copy
import io
import json
import math
import os
import statistics
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fastfourierconvolution_amd as F  # noqa: E402
from fastfourierconvolution_amd import _runtime as rt  # noqa: E402
from fastfourierconvolution_amd import training as T  # noqa: E402

NO_KERNEL = ("view", "reshape", "permute", "transpose", "t.", "detach", "alias", "expand", "squeeze", "unsqueeze",
             "slice", "select", "as_strided", "empty", "_unsafe_view", "size", "stride", "is_", "sym_", "lift",
             "_has_", "unbind", "split")
HP = dict(alpha1=0.5, alpha2=0.75, delta=0.05, epsilon=0.05)


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


def aten_weights(g_real, g_fake, real_validity, fake_validity):
    """the reference's sequence from the two cloned gradient lists to (w_r, w_f), Algorithm 1: three host
    round trips for the dots, two or more where Python compares the scores"""
    real_list = torch.cat([g.reshape(-1) for g in g_real], dim=0)
    rdotr = torch.dot(real_list, real_list).item() + 1e-4
    fake_list = torch.cat([g.reshape(-1) for g in g_fake], dim=0)
    fdotf = torch.dot(fake_list, fake_list).item() + 1e-4
    rdotf = torch.dot(real_list, fake_list).item()
    r_norm, f_norm = math.sqrt(rdotr), math.sqrt(fdotf)
    rs = torch.mean(torch.sigmoid(real_validity))
    fs = torch.mean(torch.sigmoid(fake_validity))
    eps = HP["epsilon"]
    if rs < HP["alpha1"] or rs < (fs - HP["delta"]):
        w_r, w_f = 1 / r_norm + eps, (-rdotf / (fdotf * r_norm) if rdotf <= 0 else 0.0) + eps
    elif rs > HP["alpha2"] and rs > (fs - HP["delta"]):
        w_r, w_f = (-rdotf / (rdotr * f_norm) if rdotf <= 0 else 0.0) + eps, 1 / f_norm + eps
    else:
        w_r, w_f = 1 / r_norm + eps, 1 / f_norm + eps
    return w_r, w_f


def aten_sequence(g_real, g_fake, real_validity, fake_validity):
    grad_real, grad_fake = [g.clone() for g in g_real], [g.clone() for g in g_fake]
    w_r, w_f = aten_weights(grad_real, grad_fake, real_validity, fake_validity)
    return [w_r * a + w_f * b for a, b in zip(grad_real, grad_fake)]


def aten_discriminator_step(G, D, optim_G, optim_D, z, real):
    """the critic update of the reference's drivers with its aw_loss, on the HIP layers"""
    G.requires_grad_(False)
    D.requires_grad_(True)
    fake = G(z)
    out_fake, out_real = D(fake), D(real)
    loss_real, loss_fake = T.hinge_loss_real(out_real), T.hinge_loss_fake(out_fake)
    params = [p for _, p in D.named_parameters()]
    optim_D.zero_grad()
    loss_real.backward(retain_graph=True)
    grad_real = [p.grad.clone() for p in params]
    optim_D.zero_grad()
    loss_fake.backward(retain_graph=True)
    grad_fake = [p.grad.clone() for p in params]
    optim_D.zero_grad()
    w_r, w_f = aten_weights(grad_real, grad_fake, out_real, out_fake)
    for p, a, b in zip(params, grad_real, grad_fake):
        p.grad = w_r * a + w_f * b
    optim_D.step()
    return w_r * loss_real + w_f * loss_fake


class _CountAten(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0
        self.syncs = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if name.startswith("aten._local_scalar") or name.startswith("aten.is_nonzero"):
            self.syncs += 1
        elif name.startswith("aten.") and not any(name[5:].startswith(p) for p in NO_KERNEL):
            self.n += 1
        return func(*args, **(kwargs or {}))


def _critics():
    return {"Discriminator32(mg=4)": lambda: F.Discriminator32(True, 4),
            "Discriminator(mg=4)": lambda: F.Discriminator(True, 4)}


def ops_rows(B, iters):
    rows = []
    for name, make in _critics().items():
        shapes = [tuple(p.shape) for _, p in _quiet(make).named_parameters()]
        g_real = [0.01 * torch.randn(s, device="cuda") for s in shapes]
        g_fake = [0.02 * torch.randn(s, device="cuda") for s in shapes]
        rv, fv = torch.randn(B, 1, device="cuda"), torch.randn(B, 1, device="cuda")
        out = [torch.empty_like(g) for g in g_real]
        floats = sum(g.numel() for g in g_real)

        def hip():
            stats = torch.ops.ffc.aw_weights(g_real, g_fake, rv, fv, HP["alpha1"], HP["alpha2"], HP["delta"],
                                             HP["epsilon"], True)
            torch.ops.ffc.aw_combine(g_real, g_fake, stats, out)

        r = {"row": "ops", "critic": name, "tensors": len(shapes), "floats": floats,
             "hip_ms": timed(hip, iters), "aten_ms": timed(lambda: aten_sequence(g_real, g_fake, rv, fv), iters)}
        r["speedup"] = r["aten_ms"] / r["hip_ms"]
        obs = rt.LaunchObserver()
        rt.set_observer(obs)
        hip()
        rt.set_observer(None)
        torch.cuda.synchronize()
        groups = -(-sum(1 for g in g_real if g.numel()) // 16)
        r["hip_records"] = [rec[0] for rec in obs.records]
        r["hip_kernels"] = sum(groups + 1 if rec[0] == "aw_weights" else groups for rec in obs.records)
        with _CountAten() as cnt:
            aten_sequence(g_real, g_fake, rv, fv)
        r["aten_ops"], r["aten_host_syncs"] = cnt.n, cnt.syncs
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def step_rows(B, iters):
    rows = []
    pairs = {"fgan32": (lambda: F.FGenerator32(128, 4), lambda: F.Discriminator32(True, 4), 32),
             "fgan128": (lambda: F.FGenerator(128), lambda: F.Discriminator(True, 4), 128)}
    for name, (mg, md, side) in pairs.items():
        r = {"row": "step", "pair": name, "batch": B}
        G0, D0 = _quiet(mg).cuda().train(), F.set_sn_hip(_quiet(md).cuda().train())
        z = torch.randn(B, 128, device="cuda")
        real = torch.randn(B, 3, side, side, device="cuda")
        n = max(10, iters // 10)
        for key in ("aten", "hip"):
            G, D = copy.deepcopy(G0), copy.deepcopy(D0)
            oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.9))
            oD = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.0, 0.9))
            aw = F.aw_method(**HP)
            step = (lambda: T.aw_discriminator_step(G, D, oG, oD, z, real, aw)) if key == "hip" else \
                (lambda: aten_discriminator_step(G, D, oG, oD, z, real))
            r[f"d_step_{key}_ms"] = timed(step, n, warmup=5)
        r["d_step_speedup"] = r["d_step_aten_ms"] / r["d_step_hip_ms"]
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
    rows = ops_rows(args.batch, args.iters) + step_rows(args.batch, args.iters)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
