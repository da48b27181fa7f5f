"""Generate tests/golden/metrics_*.npz by running the REFERENCE's own metric functions
(torch_fidelity/metric_fid.py, metric_kid.py, metric_isc.py).

Run where the reference tree exists (not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_metrics.py

The three metric modules import ``torch_fidelity.utils`` at module top, which pulls in torchvision and the
feature extractors.  They are loaded from their files under a stand-in ``torch_fidelity`` package whose ``utils``
module answers every name with a placeholder (none of them is called by the functions used here); ``helpers``,
``defaults`` and ``deprecations`` are the reference's own.  Nothing of the reference is restated or stored: the
fixtures hold inputs and recorded results only.

The reference is fed float64 tensors whose values are fp32-representable, so its numpy path runs in fp64
(``kid_features_to_metric`` keeps the tensor's dtype; FID and ISC promote anyway).

  metrics_fid.npz   f1 (101, 130), f2 (77, 130) float32, features with a common offset of +100;
                    mu1, sigma1, mu2, sigma2 (fid_features_to_statistics) and fid (fid_statistics_to_metric)
  metrics_kid.npz   f1 (101, 130), f2 (90, 130) float32; kid_subsets = 3, kid_subset_size = 17, the defaults
                    otherwise (degree 3, gamma 1 / D, coef0 1, seed 2020): mean, std; and degree 1 / gamma 0.25 /
                    coef0 0.5: mean_d1, std_d1
  metrics_isc.npz   logits (101, 130) float32 spanning +-40; for splits in {1, 10} and shuffle on / off:
                    mean_s<splits>_<shuffle>, std_s<splits>_<shuffle>
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


def load_metric_modules():
    pkg = types.ModuleType("torch_fidelity")
    pkg.__path__ = [PKG]
    sys.modules["torch_fidelity"] = pkg
    sys.modules["torch_fidelity.utils"] = _Anything("torch_fidelity.utils")
    out = {}
    for name in ("defaults", "deprecations", "helpers", "metric_fid", "metric_kid", "metric_isc"):
        spec = importlib.util.spec_from_file_location(f"torch_fidelity.{name}", os.path.join(PKG, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        out[name] = mod
    return out


def features(seed, n, d, offset=0.0, scale=1.0):
    rng = np.random.RandomState(seed)
    mix = rng.randn(d, d) / np.sqrt(d)
    return (offset + scale * rng.randn(n, d) @ mix + 0.3 * rng.randn(d)).astype(np.float32)


def logits(seed, n, c):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-40.0, 40.0, size=(n, c))
    x[::7] *= 0.05   # some flat rows among the peaked ones
    return x.astype(np.float32)


def main():
    ref = load_metric_modules()
    fid, kid, isc = ref["metric_fid"], ref["metric_kid"], ref["metric_isc"]
    t64 = lambda a: torch.from_numpy(a.astype(np.float64))   # noqa: E731

    f1, f2 = features(11, 101, 130, offset=100.0), features(12, 77, 130, offset=100.0, scale=1.2)
    s1, s2 = fid.fid_features_to_statistics(t64(f1)), fid.fid_features_to_statistics(t64(f2))
    assert s1["sigma"].dtype == np.float64
    value = fid.fid_statistics_to_metric(s1, s2, False)[fid.KEY_METRIC_FID]
    np.savez(os.path.join(HERE, "metrics_fid.npz"), f1=f1, f2=f2, mu1=s1["mu"], sigma1=s1["sigma"], mu2=s2["mu"],
             sigma2=s2["sigma"], fid=np.float64(value))

    k1, k2 = features(21, 101, 130), features(22, 90, 130, scale=1.1)
    kw = dict(kid_subsets=3, kid_subset_size=17)
    a = kid.kid_features_to_metric(t64(k1), t64(k2), **kw)
    b = kid.kid_features_to_metric(t64(k1), t64(k2), kid_kernel_poly_degree=1, kid_kernel_poly_gamma=0.25,
                                   kid_kernel_poly_coef0=0.5, **kw)
    np.savez(os.path.join(HERE, "metrics_kid.npz"), f1=k1, f2=k2, mean=np.float64(a[kid.KEY_METRIC_KID_MEAN]),
             std=np.float64(a[kid.KEY_METRIC_KID_STD]), mean_d1=np.float64(b[kid.KEY_METRIC_KID_MEAN]),
             std_d1=np.float64(b[kid.KEY_METRIC_KID_STD]))

    lg = logits(31, 101, 130)
    rec = dict(logits=lg)
    for splits in (1, 10):
        for shuffle in (True, False):
            r = isc.isc_features_to_metric(t64(lg), splits, shuffle, 2020)
            rec[f"mean_s{splits}_{int(shuffle)}"] = np.float64(r[isc.KEY_METRIC_ISC_MEAN])
            rec[f"std_s{splits}_{int(shuffle)}"] = np.float64(r[isc.KEY_METRIC_ISC_STD])
    np.savez(os.path.join(HERE, "metrics_isc.npz"), **rec)
    print("fid", value, "kid", a, b, "isc", {k: float(v) for k, v in rec.items() if k != "logits"})


if __name__ == "__main__":
    main()
