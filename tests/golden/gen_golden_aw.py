"""Generate the adaptive-weight loss fixture by running the REFERENCE's own aw_method in float64.

Run where the reference tree exists (not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_aw.py

layers/aw_loss.py is loaded by path; nothing of the class is restated here.

The critic is a toy: a ParameterList of zeros with Dloss_real = sum <p_i, a_i> + c_r and
Dloss_fake = sum <p_i, b_i> + c_f, so the two gradient lists the reference builds are exactly the
fp32-representable a_i and b_i.  b is built from a with cosine +0.5 (``bpos``) or -0.5 (``bneg``) and
1.5 times its norm; constant logits set rs and fs.  Tensor shapes: (1,), (3,), (5, 7), (64, 3, 3, 3), one
tensor one element longer than the kernels' 16384-element chunk (non-zero at 512 places, among them
the first and last element of the first chunk and the lone element of the second, so the fixture
stays small) and fourteen (2, 3): 19 tensors, more than one launch's table, with a ragged tail.

aw_cases.npz holds inputs and recorded results only: a.<i>, bpos.<i>, bneg.<i> (float32), and per
(algorithm, case) combination k = 0..9 the logits case<k>.real / case<k>.fake (float32), case<k>.hyper
(the values of ``hyper_names``), the reference's returned loss case<k>.loss and its param.grads
case<k>.grad.<i> (float64).

The branch is discontinuous, so every case sits away from its thresholds: |rs - alpha1|, |rs - alpha2|,
|rs - (fs - delta)| >= 1e-3 and |rdotf| >= 1e-3 ||a|| ||b||, asserted below on the reference's own
quantities in fp64.
"""
from __future__ import annotations

import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402
from fixture_weights import key_rng  # noqa: E402

REF = G.REF
SEED = 2718
CHUNK = 16384   # ffc_aw_chunk(): elements of one workgroup's chunk in csrc/aw_kernels.hip
SHAPES = [(1,), (3,), (5, 7), (64, 3, 3, 3), (CHUNK + 1,)] + [(2, 3)] * 14
SPARSE = 4      # index of the long tensor
HYPER = ("alpha1", "alpha2", "delta", "epsilon", "normalized", "cosine", "real_logit", "fake_logit", "c_r", "c_f",
         "case")
# (normalized, intended case, real logit, cosine); the fake logits are 0: fs = 0.5
COMBOS = [(n, c, r, s) for n in (1, 0)
          for c, r, s in ((1, -1.0, -0.5), (2, -1.0, 0.5), (3, 2.0, -0.5), (4, 2.0, 0.5), (5, 0.5, 0.5 if n else -0.5))]


def reference_class():
    spec = importlib.util.spec_from_file_location("ref_aw_loss", os.path.join(REF, "layers", "aw_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.aw_method


def make_lists():
    """a, and b at cosine +0.5 / -0.5 with ||b|| = 1.5 ||a|| (before rounding to float32)"""
    rng = key_rng(SEED, "aw")
    sizes = [int(np.prod(s)) for s in SHAPES]
    mask = np.ones(sum(sizes), dtype=bool)
    o = sum(sizes[:SPARSE])
    mask[o:o + sizes[SPARSE]] = False
    keep = np.concatenate([[0, CHUNK - 1, CHUNK], rng.choice(np.arange(1, CHUNK - 1), 509, replace=False)])
    mask[o + keep] = True
    a = (rng.normal(0.0, 0.05, size=mask.size) * mask).astype(np.float32).astype(np.float64)
    q = rng.normal(0.0, 1.0, size=mask.size) * mask
    q -= (q @ a) / (a @ a) * a
    q *= np.sqrt(a @ a) / np.sqrt(q @ q)
    out = {"a": a.astype(np.float32)}
    for name, c in (("bpos", 0.5), ("bneg", -0.5)):
        out[name] = (1.5 * (c * a + np.sqrt(1.0 - c * c) * q)).astype(np.float32)
    split = np.cumsum(sizes)[:-1]
    return {k: [p.reshape(s) for p, s in zip(np.split(v, split), SHAPES)] for k, v in out.items()}


def run_case(cls, lists, normalized, case, real_logit, cosine):
    hyper = dict(alpha1=0.5, alpha2=0.75, delta=0.05, epsilon=0.05, normalized=float(normalized), cosine=cosine,
                 real_logit=real_logit, fake_logit=0.0, c_r=0.75, c_f=1.25, case=float(case))
    a = [torch.from_numpy(x).double() for x in lists["a"]]
    b = [torch.from_numpy(x).double() for x in lists["bpos" if cosine > 0 else "bneg"]]
    net = torch.nn.Module()
    net.p = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros_like(x)) for x in a])
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    real = torch.full((4, 1), real_logit, dtype=torch.float32)
    fake = torch.full((2, 3), 0.0, dtype=torch.float32)
    loss_r = sum((p * x).sum() for p, x in zip(net.p, a)) + hyper["c_r"]
    loss_f = sum((p * x).sum() for p, x in zip(net.p, b)) + hyper["c_f"]
    aw = cls(hyper["alpha1"], hyper["alpha2"], hyper["delta"], hyper["epsilon"], bool(normalized))
    loss = aw.aw_loss(loss_r, loss_f, opt, net, real.double(), fake.double())
    # the condition, on the reference's own quantities
    fa, fb = torch.cat([x.reshape(-1) for x in a]), torch.cat([x.reshape(-1) for x in b])
    rs, fs = float(torch.mean(torch.sigmoid(real.double()))), float(torch.mean(torch.sigmoid(fake.double())))
    rdotf = float(torch.dot(fa, fb))
    assert min(abs(rs - hyper["alpha1"]), abs(rs - hyper["alpha2"]), abs(rs - (fs - hyper["delta"]))) >= 1e-3
    assert abs(rdotf) >= 1e-3 * float(fa.norm() * fb.norm())
    arrays = {"hyper": np.array([hyper[k] for k in HYPER]), "real": real.numpy(), "fake": fake.numpy(),
              "loss": np.float64(loss.item())}
    for i, p in enumerate(net.p):
        assert p.grad.dtype == torch.float64
        arrays[f"grad.{i}"] = p.grad.numpy().copy()
    return arrays


def main():
    cls = reference_class()
    lists = make_lists()
    arrays = {"ncases": np.int64(len(COMBOS)), "ntensors": np.int64(len(SHAPES)), "hyper_names": np.array(HYPER)}
    for k, v in lists.items():
        for i, x in enumerate(v):
            arrays[f"{k}.{i}"] = x
    for k, combo in enumerate(COMBOS):
        for name, v in run_case(cls, lists, *combo).items():
            arrays[f"case{k}.{name}"] = v
    path = os.path.join(HERE, "aw_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"aw_cases {os.path.getsize(path) / 1024:8.1f} KiB  {len(COMBOS)} cases, {len(SHAPES)} tensors")
    assert os.path.getsize(path) < 512 * 1024, "keep the fixture well under the committed-file limit"


if __name__ == "__main__":
    main()
