"""Generate the class-conditional fgan128 fixtures by running the REFERENCE's own classes in fp64.

Run where the reference tree exists (not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cond.py

fgan128_cond_complete.py imports torchvision / tensorboard / torch_fidelity at module top and runs
main() at import, so it cannot be imported.  Its two model classes are taken out of the file
instead: the source is parsed with ``ast`` and only the ``FCondGenerator`` and ``Discriminator``
ClassDef nodes are compiled and executed, in a namespace that holds the reference's own layers
(imported the way gen_golden.py imports them).  Nothing of the classes is restated here.

The reference draws the train-mode NoiseInjection noise inside the layer; to feed explicit noise each
NoiseInjection instance's ``forward`` is bound to its fixture noise (layers/noise_injection.py:25
takes it as an argument).  The float image behind the eval-mode uint8 output is read with a forward
hook on the model's Resizer.

Cases (all fp64 on the CPU; arrays stored as float32): cond_gen_train, cond_gen_eval, cond_disc,
grad_cond_gen, grad_cond_disc.  Inputs are not stored: tests regenerate them with
fixture_weights.input_array(seed, name, shape) from manifest_cond.json (labels are listed there);
weights come from fixture_weights.make_state(seed, specs).  Gradient cases store the gradients of
the parameters the conditional models add (label_embed, label_conv.*, input_conv.*, the critic's
conv1) and the input gradient, for loss = <out, cot> with cot = input_array(seed + 11, "cot:out").
"""
from __future__ import annotations

import ast
import functools
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

SCRIPT = os.path.join(G.REF, "fgan128_cond_complete.py")
NOISE = {f"noise{n}_{br}": [2, 1, 2 ** (n + 1), 2 ** (n + 1)] for n in (2, 3, 4, 5, 6) for br in "lg"}
GEN = dict(kind="FCondGenerator", ctor=dict(z_size=16, num_classes=3), labels=[2, 0])
DISC = dict(kind="FCondDiscriminator", ctor=dict(sn=True, num_classes=3), labels=[1, 1])
CASES = [
    dict(name="cond_gen_train", mode="train", seed=1234, inputs={"z": [2, 16], **NOISE}, **GEN),
    dict(name="cond_gen_eval", mode="eval", seed=777,   # seed: see the rounding-edge check in run_case
         inputs={"z": [2, 16]}, **GEN),
    dict(name="cond_disc", mode="train", seed=1234, inputs={"x": [2, 3, 128, 128]}, **DISC),
    dict(name="grad_cond_gen", mode="train", seed=4321, inputs={"z": [2, 16], **NOISE}, grad=True, **GEN),
    dict(name="grad_cond_disc", mode="train", seed=4321, inputs={"x": [2, 3, 128, 128]}, grad=True, **DISC),
]
NEW_PARAMS = ("label_embed.", "label_conv.", "input_conv.", "conv1.")


def reference_classes(ref):
    """{name: class} for the script's FCondGenerator and Discriminator ClassDef nodes"""
    tree = ast.parse(open(SCRIPT).read(), SCRIPT)
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("FCondGenerator", "Discriminator")]
    assert len(nodes) == 2, [n.name for n in nodes]
    ns = {"torch": torch, "nn": nn, "FFCModel": ref.FFCModel, "FFC_BN_ACT": ref.FFC_BN_ACT,
          "NoiseInjection": ref.NoiseInjection}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), SCRIPT, "exec"), ns)
    return {"FCondGenerator": ns["FCondGenerator"], "FCondDiscriminator": ns["Discriminator"]}


def cond_specs(module):
    """weight specs per state_dict key: gen_golden.weight_specs for the FFC layers and plain convs,
    plus nn.Embedding and spectral-norm wrapped Conv2d / Linear (weight_orig, weight_u, weight_v)"""
    specs = {}
    for name, child in module.named_children():
        pre = name + "."
        if isinstance(child, nn.Embedding):
            specs[pre + "weight"] = [list(child.weight.shape), "normal", 0.0, 1.0, "float32"]
        elif hasattr(child, "weight_orig"):
            w = child.weight_orig
            specs[pre + "weight_orig"] = [list(w.shape), "normal", 0.0, w[0].numel() ** -0.5, "float32"]
            specs[pre + "weight_u"] = [list(child.weight_u.shape), "normal", 0.0, 1.0, "float32"]
            specs[pre + "weight_v"] = [list(child.weight_v.shape), "normal", 0.0, 1.0, "float32"]
            if child.bias is not None:
                specs[pre + "bias"] = [list(child.bias.shape), "normal", 0.0, 0.1, "float32"]
        else:
            specs.update({pre + k: v for k, v in G.weight_specs(child).items()})
    missing = set(module.state_dict()) ^ set(specs)
    assert not missing, missing
    return specs


def bind_noise(mod, t):
    for n in (2, 3, 4, 5, 6):
        for br, attr in (("l", "lcl"), ("g", "glb")):
            m = getattr(mod, f"{attr}_noise{n}")
            m.forward = functools.partial(type(m).forward, m, noise=t[f"noise{n}_{br}"])


def f32(t):
    return t.detach().numpy().astype(np.float32)


def run_case(classes, c):
    torch.manual_seed(0)
    with G.contextlib.redirect_stdout(G.io.StringIO()):
        mod = classes[c["kind"]](**c["ctor"])
    specs = cond_specs(mod)
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in make_state(c["seed"], specs).items()})
    mod = mod.double()
    seed, gen = c["seed"], c["kind"] == "FCondGenerator"
    labels = torch.tensor(c["labels"], dtype=torch.int64)
    tin = {k: torch.from_numpy(input_array(seed, k, shp)).double() for k, shp in c["inputs"].items()}
    arrays = {}
    floats = []
    if gen:
        mod.resizer.register_forward_hook(lambda m, i, o: floats.append(o))
    if c["mode"] == "eval":   # running stats of realistic scale: one train pass at momentum 1 on other inputs
        warm = {k: torch.from_numpy(input_array(seed + 7, k, shp)).double()
                for k, shp in {**c["inputs"], **NOISE}.items()}
        G.set_momentum(mod, 1.0)
        mod.train()
        bind_noise(mod, warm)
        with torch.no_grad():
            mod(warm["z"], labels)
        G.set_momentum(mod, 0.1)
        for k, v in G.bn_buffers(mod).items():
            arrays["before." + k] = v
        mod.eval()
    else:
        mod.train()
        if gen:
            bind_noise(mod, tin)
    first = tin["z" if gen else "x"].requires_grad_(bool(c.get("grad")))
    with torch.set_grad_enabled(bool(c.get("grad"))):
        out = mod(first, labels)
    if c.get("grad"):
        cot = torch.from_numpy(input_array(seed + 11, "cot:out", list(out.shape))).double()
        (out * cot).sum().backward()
        arrays["gin." + ("z" if gen else "x")] = f32(first.grad)
        for k, p in mod.named_parameters():
            if k.startswith(NEW_PARAMS) and p.grad is not None:
                arrays["gpar." + k] = f32(p.grad)
        arrays["ref.out"] = f32(out)
    elif c["mode"] == "eval":
        assert out.dtype == torch.uint8
        arrays["ref.out_u8"] = out.numpy()
        arrays["ref.out"] = f32(floats[-1])
        # the uint8 comparison allows one level on < 1e-3 of the pixels: the fixture must not sit on
        # rounding edges itself (distance of 255 * (x / 2 + 1 / 2) to the next integer below fp32 noise)
        q = 255.0 * (floats[-1] * 0.5 + 0.5)
        frac = q - q.floor()
        edge = float(((frac < 1e-4) | (frac > 1 - 1e-4)).double().mean())
        print(f"  share of pixels within 1e-4 of a quantization edge: {edge:.2e}")
        assert edge < 5e-4, "pick another seed: the float image sits on rounding edges"
    else:
        arrays["ref.out"] = f32(out)
    for k, v in G.bn_buffers(mod).items():
        arrays["after." + k] = v.astype(np.float32) if v.dtype == np.float64 else v
    arrays = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in arrays.items()}
    return specs, arrays


def main():
    ref = G.load_reference()
    classes = reference_classes(ref)
    manifest = {"generator": "tests/golden/gen_golden_cond.py", "torch": torch.__version__,
                "numpy": np.__version__, "cases": []}
    for c in CASES:
        specs, arrays = run_case(classes, c)
        path = os.path.join(HERE, c["name"] + ".npz")
        np.savez_compressed(path, **arrays)
        entry = dict(c)
        entry["specs"] = specs
        entry["outputs"] = sorted(k for k in arrays if k.startswith("ref."))
        entry["grads"] = sorted(k for k in arrays if k.startswith(("gin.", "gpar.")))
        manifest["cases"].append(entry)
        print(f"{c['name']:16s} {os.path.getsize(path) / 1024:8.1f} KiB  {entry['outputs']} grads={len(entry['grads'])}")
        assert os.path.getsize(path) < 760 * 1024, "fixture larger than the largest existing one"
    with open(os.path.join(HERE, "manifest_cond.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
