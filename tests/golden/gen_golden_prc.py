"""Generate tests/golden/metrics_prc.npz by running the REFERENCE's own ``prc_features_to_metric``
(torch_fidelity/metric_prc.py).

Run where the reference tree exists (not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_prc.py

``metric_prc`` imports ``torch_fidelity.utils`` at module top like the other metric modules; it is loaded from its
file under the same stand-in package as gen_golden_metrics.py builds (a ``utils`` that answers every name with a
placeholder; ``helpers``, ``defaults`` and ``deprecations`` are the reference's own).  Nothing of the reference is
restated or stored: the fixture holds inputs and recorded results only.

The reference is fed float64 tensors whose values are fp32-representable, so its ``cdist`` runs in fp64 (in fp32 it
counts a different number of samples on case A: precision 24/90 instead of 23/90).

  metrics_prc.npz   a_f1 (101, 130), a_f2 (90, 130) float32 with a common offset of +100; b_f1 (65, 33),
                    b_f2 (130, 33) float32; for case a with k in {3, 1} and case b with k = 3, and save_cpu_ram
                    off / on: <case>_k<k>_<ram> = [precision, recall, f_score] as float64
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402

PKG = os.path.join(G.REF, "torch_fidelity")


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def load_metric_prc():
    pkg = types.ModuleType("torch_fidelity")
    pkg.__path__ = [PKG]
    sys.modules["torch_fidelity"] = pkg
    sys.modules["torch_fidelity.utils"] = _Anything("torch_fidelity.utils")
    mod = None
    for name in ("defaults", "deprecations", "helpers", "metric_prc"):
        spec = importlib.util.spec_from_file_location(f"torch_fidelity.{name}", os.path.join(PKG, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
    return mod


def features(seed, n, d, offset, scale, shift):
    """gen_golden_metrics.features with its constant 0.3 as ``shift``"""
    rng = np.random.RandomState(seed)
    mix = rng.randn(d, d) / np.sqrt(d)
    return (offset + scale * rng.randn(n, d) @ mix + shift * rng.randn(d)).astype(np.float32)


CASES = {
    "a": (features(41, 101, 130, 100.0, 1.0, 0.3), features(42, 90, 130, 100.0, 1.0, 0.1), (3, 1)),
    "b": (features(41, 65, 33, 0.0, 1.0, 0.3), features(42, 130, 33, 0.0, 0.9, 0.0), (3,)),
}


def main():
    prc = load_metric_prc()
    t64 = lambda a: torch.from_numpy(a.astype(np.float64))   # noqa: E731
    rec = {}
    for case, (f1, f2, ks) in CASES.items():
        rec[f"{case}_f1"], rec[f"{case}_f2"] = f1, f2
        for k in ks:
            for ram in (False, True):
                # prc_batch_size 37: both routes split the rows, and must still agree
                r = prc.prc_features_to_metric(t64(f1), t64(f2), prc_neighborhood=k, prc_batch_size=37,
                                               save_cpu_ram=ram, verbose=False)
                rec[f"{case}_k{k}_{int(ram)}"] = np.array([r[prc.KEY_METRIC_PRECISION], r[prc.KEY_METRIC_RECALL],
                                                           r[prc.KEY_METRIC_F_SCORE]], dtype=np.float64)
            assert np.array_equal(rec[f"{case}_k{k}_0"], rec[f"{case}_k{k}_1"])
    np.savez(os.path.join(HERE, "metrics_prc.npz"), **rec)
    for key, v in rec.items():
        if "_k" in key:
            n1, n2 = len(rec[key[0] + "_f1"]), len(rec[key[0] + "_f2"])
            print(key, v.tolist(), "precision * N2 =", v[0] * n2, "recall * N1 =", v[1] * n1)


if __name__ == "__main__":
    main()
