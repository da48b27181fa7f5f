#!/usr/bin/env python
"""Record tests/golden/sagan/b{2,3}.npz from the reference's own SAGAN classes in float64 on the CPU.

    python tools/make_sagan_golden.py /path/to/reference

Run by hand, never by a test: it needs the reference checkout (benchmark_models/sagan goes on sys.path here).
The weights are tests/sagan_refs.fill(state_dict, 0) on both models; the fixtures hold inputs' results only:
  g/...  from the fill state, both models in train mode: img, p2 = G(z_g); out, p1 = D(img); (-out.mean()).backward()
         img, d_out, p1 in full, p2 at every 8th row and as column sums (in full it would be 1.5 MB at B = 3), every
         u / v and BatchNorm statistic after the forward, G's gradients
  d/...  from the fill state again: D(real), then D(G(z_d)) with G's graph cut; (d_loss_real + d_loss_fake).backward()
         both critic outputs, the two losses, D's u / v after its two forwards, D's gradients
Gradients of biases, gamma and BatchNorm affines in full; of each weight its sum, L2 norm and every 97th element."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sagan_refs as R  # noqa: E402


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def changed(model, prefix):
    keep = ("weight_u", "weight_v", "running_mean", "running_var", "num_batches_tracked")
    return {prefix + k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(keep)}


def models(B, ref):
    G = ref.Generator(B, 32, R.Z_DIM, 64).double().train()
    D = ref.Discriminator(B, 32, 64).double().train()
    R.fill(G.state_dict(), 0)
    R.fill(D.state_dict(), 0)
    return G, D


def record(B, ref):
    z_g, z_d, real = R.inputs(B)
    out = {}
    G, D = models(B, ref)
    img, p2 = G(z_g)
    d_out, p1 = D(img)
    loss = -d_out.mean()
    loss.backward()
    res = dict(img=img.detach(), p2=p2.detach(), d_out=d_out.detach(), p1=p1.detach(), g_loss=loss.detach())
    res.update(changed(G, "G."))
    res.update({k: v for k, v in changed(D, "D.").items() if "running" not in k and "tracked" not in k})
    out.update({"g/" + k: v for k, v in R.compact(res).items()})
    for k, g in grads_of(G).items():
        out.update(R.digest("g/grad/" + k, g))

    G, D = models(B, ref)
    d_real, _ = D(real)
    with torch.no_grad():
        fake, _ = G(z_d)
    d_fake, _ = D(fake)
    lr = torch.nn.ReLU()(1.0 - d_real).mean()
    lf = torch.nn.ReLU()(1.0 + d_fake).mean()
    (lr + lf).backward()
    res = dict(d_real=d_real.detach(), d_fake=d_fake.detach(), d_loss_real=lr.detach(), d_loss_fake=lf.detach())
    res.update(changed(D, "D."))
    out.update({"d/" + k: v for k, v in res.items()})
    for k, g in grads_of(D).items():
        out.update(R.digest("d/grad/" + k, g))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(sys.argv[1], "benchmark_models", "sagan"))
    import sagan_models as ref
    os.makedirs(R.GOLDEN, exist_ok=True)
    for B in (2, 3):
        out = record(B, ref)
        path = os.path.join(R.GOLDEN, f"b{B}.npz")
        np.savez(path, **{k: v.numpy() for k, v in out.items()})
        print(path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
