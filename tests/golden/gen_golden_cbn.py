"""Generate the conditional-batch-norm fixtures by running the REFERENCE's own classes in fp64.

Run where the reference tree exists (not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cbn.py

Cases (fp64 on the CPU, arrays stored as float32) -- only what the reference can run, i.e. layers
where no label reaches a SpectralTransform (in_cg == 0 or ratio_gout == 0):
  cbn_train / cbn_eval         ConditionalBatchNorm2d(6, 3) on (5, 6, 3, 3), labels shaped (B, 1, 1), class 1
                               absent from the batch, classes 0 and 2 present more than once
  cbn_up_train / cbn_up_eval   FFC_BN_ACT(32, 16, 4, 0.0, 0.25, stride=2, padding=1, GELU,
                               ConditionalBatchNorm2d, upsampling=True, num_classes=4), B = 4, 4x4
  cbn_conv3                    FFC_BN_ACT(4, 16, 3, 0.0, 0.25, 1, 1, bias=True, LeakyReLU, ..., num_classes=4), 8x8
  cbn_conv4                    FFC_BN_ACT(16, 32, 4, 0.25, 0.0, 2, 1, bias=True, LeakyReLU, ..., num_classes=4), 8x8
                               tuple input
Every case stores the forward outputs (ref.*), the updated running buffers (after.*) and, for
loss = sum <out, cot> with cot = input_array(seed + 11, "cot:" + name), the input gradients (gin.*) and
all parameter gradients (gpar.*).  Inputs and weights are not stored: tests regenerate them from
manifest_cbn.json with fixture_weights (labels are listed there).  Eval cases draw their running
statistics from the specs (mean ~ N(0, 0.3), var ~ U(0.5, 1.5)).

manifest_cbn.json also lists the state_dict keys of the four model classes of fgan_cond_complete.py
(taken out of the script with ``ast``, as gen_golden_cond.py does: the script cannot be imported).
"""
from __future__ import annotations

import ast
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import gen_golden as G  # noqa: E402
from fixture_weights import input_array, make_state  # noqa: E402

SCRIPT = os.path.join(G.REF, "fgan_cond_complete.py")
FBA = dict(norm_layer="ConditionalBatchNorm2d", num_classes=4)
UP = dict(in_channels=32, out_channels=16, kernel_size=4, ratio_gin=0.0, ratio_gout=0.25, stride=2, padding=1,
          activation_layer="GELU", upsampling=True, **FBA)
CASES = [
    dict(name="cbn_train", kind="ConditionalBatchNorm2d", ctor=dict(num_features=6, num_classes=3), mode="train",
         seed=1234, inputs={"x": [5, 6, 3, 3]}, labels=[2, 0, 2, 0, 0], label_shape=[5, 1, 1]),
    dict(name="cbn_eval", kind="ConditionalBatchNorm2d", ctor=dict(num_features=6, num_classes=3), mode="eval",
         seed=4321, inputs={"x": [5, 6, 3, 3]}, labels=[2, 0, 2, 0, 0], label_shape=[5, 1, 1]),
    dict(name="cbn_up_train", kind="FFC_BN_ACT", ctor=UP, mode="train", seed=1234, inputs={"x": [4, 32, 4, 4]},
         labels=[3, 1, 1, 0], label_shape=[4, 1, 1]),
    dict(name="cbn_up_eval", kind="FFC_BN_ACT", ctor=UP, mode="eval", seed=4321, inputs={"x": [4, 32, 4, 4]},
         labels=[3, 1, 1, 0], label_shape=[4, 1, 1]),
    dict(name="cbn_conv3", kind="FFC_BN_ACT",
         ctor=dict(in_channels=4, out_channels=16, kernel_size=3, ratio_gin=0.0, ratio_gout=0.25, stride=1,
                   padding=1, bias=True, activation_layer="LeakyReLU", **FBA),
         mode="train", seed=1234, inputs={"x": [4, 4, 8, 8]}, labels=[0, 2, 2, 3], label_shape=[4, 1, 1]),
    dict(name="cbn_conv4", kind="FFC_BN_ACT",
         ctor=dict(in_channels=16, out_channels=32, kernel_size=4, ratio_gin=0.25, ratio_gout=0.0, stride=2,
                   padding=1, bias=True, activation_layer="LeakyReLU", **FBA),
         mode="train", seed=1234, inputs={"x_l": [4, 12, 8, 8], "x_g": [4, 4, 8, 8]}, labels=[1, 1, 0, 3],
         label_shape=[4, 1, 1]),
]
MODELS = {"FCondGenerator32": ("FCondGenerator", dict(z_size=16, mg=4, num_classes=3)),
          "FCondGeneratorSTL": ("FCondGeneratorSTL", dict(z_size=16, mg=6, num_classes=3)),
          "CondDiscriminator32": ("Discriminator", dict(sn=True, mg=4, num_classes=3)),
          "FCondDiscriminator32": ("FDiscriminator", dict(sn=True, mg=4, num_classes=3))}


def load_cond(ref):
    """the reference's ConditionalBatchNorm2d and GaussianNoise, next to what gen_golden loads"""
    import layers.cond.cond_bn as cb
    import layers.gaussian_noise as gn
    return cb.ConditionalBatchNorm2d, gn.GaussianNoise


def cbn_specs(module, mode):
    """gen_golden.weight_specs restricted to the module's own state_dict keys (the wrapped BatchNorm2d
    is affine-less), plus the embedding tables: scale and shift columns both ~ N(0.6, 0.4)"""
    specs = {}
    for name, m in module.named_modules():
        pre = name + "." if name else ""
        if isinstance(m, nn.Embedding):
            specs[pre + "weight"] = [list(m.weight.shape), "normal", 0.6, 0.4, "float32"]
        elif not list(m.children()) and m.state_dict():
            specs.update({pre + k: v for k, v in G.weight_specs(m).items() if k in m.state_dict()})
    if mode == "eval":
        for k in list(specs):
            if k.endswith("running_mean"):
                specs[k] = [specs[k][0], "normal", 0.0, 0.3, "float32"]
            elif k.endswith("running_var"):
                specs[k] = [specs[k][0], "uniform", 0.5, 1.5, "float32"]
    assert set(specs) == set(module.state_dict()), set(specs) ^ set(module.state_dict())
    return specs


def f32(t):
    return t.detach().numpy().astype(np.float32)


def run_case(ref, CBN, c):
    torch.manual_seed(0)
    kw = dict(c["ctor"])
    for k in ("norm_layer", "activation_layer"):
        if k in kw:
            kw[k] = CBN if kw[k] == "ConditionalBatchNorm2d" else getattr(nn, kw[k])
    with G.contextlib.redirect_stdout(G.io.StringIO()):
        mod = (CBN if c["kind"] == "ConditionalBatchNorm2d" else ref.FFC_BN_ACT)(**kw)
    specs = cbn_specs(mod, c["mode"])
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make_state(c["seed"], specs).items()})
    mod = mod.double().train(c["mode"] == "train")
    seed = c["seed"]
    labels = torch.tensor(c["labels"], dtype=torch.int64).view(c["label_shape"])
    tin = {k: torch.from_numpy(input_array(seed, k, shp)).double().requires_grad_(True)
           for k, shp in c["inputs"].items()}
    x = tin["x"] if "x" in tin else (tin["x_l"], tin["x_g"])
    out = mod(x, labels)
    outs = {"out": out} if isinstance(out, torch.Tensor) else \
        {n: o for n, o in zip(("out_l", "out_g"), out) if isinstance(o, torch.Tensor)}
    loss = 0.0
    for n, o in outs.items():
        cot = torch.from_numpy(input_array(seed + 11, "cot:" + n, list(o.shape))).double()
        loss = loss + (o * cot).sum()
    loss.backward()
    arrays = {"ref." + n: f32(o) for n, o in outs.items()}
    for k, t in tin.items():
        arrays["gin." + k] = f32(t.grad)
    for k, p in mod.named_parameters():
        arrays["gpar." + k] = f32(p.grad)
    for k, v in G.bn_buffers(mod).items():
        arrays["after." + k] = v.astype(np.float32) if v.dtype == np.float64 else v
    return specs, arrays


def model_keys(ref, CBN, GaussianNoise):
    tree = ast.parse(open(SCRIPT).read(), SCRIPT)
    want = {v[0] for v in MODELS.values()}
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in want]
    assert len(nodes) == len(want), [n.name for n in nodes]
    ns = {"torch": torch, "nn": nn, "FFCModel": ref.FFCModel, "FFC_BN_ACT": ref.FFC_BN_ACT,
          "NoiseInjection": ref.NoiseInjection, "ConditionalBatchNorm2d": CBN, "GaussianNoise": GaussianNoise}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), SCRIPT, "exec"), ns)
    keys = {}
    for name, (cls, kw) in MODELS.items():
        with G.contextlib.redirect_stdout(G.io.StringIO()):
            m = ns[cls](**kw)
        keys[name] = {"ctor": kw, "keys": {k: list(v.shape) for k, v in m.state_dict().items()}}
    return keys


def main():
    ref = G.load_reference()
    CBN, GaussianNoise = load_cond(ref)
    manifest = {"generator": "tests/golden/gen_golden_cbn.py", "torch": torch.__version__,
                "numpy": np.__version__, "cases": [], "models": model_keys(ref, CBN, GaussianNoise)}
    total = 0
    for c in CASES:
        specs, arrays = run_case(ref, CBN, c)
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **arrays)
        entry = dict(c)
        entry["specs"] = specs
        entry["outputs"] = sorted(k for k in arrays if k.startswith("ref."))
        entry["grads"] = sorted(k for k in arrays if k.startswith(("gin.", "gpar.")))
        manifest["cases"].append(entry)
        total += os.path.getsize(path)
        print(f"{c['name']:14s} {os.path.getsize(path) / 1024:8.1f} KiB  {entry['outputs']} grads={len(entry['grads'])}")
    assert total < 512 * 1024, "the conditional-norm fixtures are meant to stay small"
    with open(os.path.join(HERE, "manifest_cbn.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
