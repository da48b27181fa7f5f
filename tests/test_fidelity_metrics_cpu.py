"""The host side of fidelity.py's metrics without a GPU: the new names import, fid_statistics_to_metric, the
MMD^2-from-six-sums and ISC-from-chunk-sums formulas reproduce the golden values (tests/golden/metrics_*.npz), merge's
re-pivot identity holds, and the argument checks raise what the reference's do."""
import os

import numpy as np
import pytest
import torch

import metric_refs as R
from conftest import ROOT
from fastfourierconvolution_amd import fidelity as FD

GOLD = os.path.join(ROOT, "tests", "golden")


def _gold(name):
    return np.load(os.path.join(GOLD, f"metrics_{name}.npz"))


def test_new_names_import_and_old_ones_stay():
    for name in ("random_normal", "GenerativeModelModuleWrapper", "generate_batches", "FeatureStats",
                 "fid_statistics_to_metric", "kid_features_to_metric", "isc_features_to_metric", "calculate_metrics"):
        assert name in FD.__all__ and callable(getattr(FD, name))
    for op in ("feat_moments_update", "kid_sums", "isc_sums"):
        assert hasattr(torch.ops.ffc, op)
    assert FD.KEY_METRIC_FID == "frechet_inception_distance"
    assert (FD.KEY_METRIC_ISC_MEAN, FD.KEY_METRIC_ISC_STD) == ("inception_score_mean", "inception_score_std")
    assert (FD.KEY_METRIC_KID_MEAN, FD.KEY_METRIC_KID_STD) == ("kernel_inception_distance_mean",
                                                               "kernel_inception_distance_std")


def test_fid_statistics_to_metric_matches_the_fixture():
    g = _gold("fid")
    out = FD.fid_statistics_to_metric(dict(mu=g["mu1"], sigma=g["sigma1"]), dict(mu=g["mu2"], sigma=g["sigma2"]))
    assert list(out) == [FD.KEY_METRIC_FID] and out[FD.KEY_METRIC_FID] == float(g["fid"])
    with pytest.raises(ValueError):
        FD.fid_statistics_to_metric(dict(mu=g["mu1"][:5], sigma=g["sigma1"]), dict(mu=g["mu2"], sigma=g["sigma2"]))
    with pytest.raises(ValueError):
        FD.fid_statistics_to_metric(dict(mu=g["mu1"], sigma=g["sigma1"].astype(np.float32)),
                                    dict(mu=g["mu2"], sigma=g["sigma2"]))


def test_mmd2_from_six_sums_matches_the_fixture():
    g = _gold("kid")
    f1, f2 = g["f1"], g["f2"]
    i1, i2 = R.kid_tables(len(f1), len(f2), 3, 17)
    sums, bounds = R.kid_sums(f1, f2, i1, i2, 3, 1.0 / 130, 1.0)
    mm = FD.mmd2_from_sums(torch.from_numpy(R.lower(sums)), 17)
    tol = float(np.max(R.mmd2_bound(bounds, 17))) + 8 * R.U * float(mm.abs().max())
    assert abs(float(mm.mean()) - float(g["mean"])) <= tol
    assert abs(float(mm.std(unbiased=False)) - float(g["std"])) <= tol


def test_isc_from_chunk_sums_matches_the_fixture():
    g = _gold("isc")
    ch = R.isc_chunks(g["logits"], R.isc_perm(101, True), 10)
    scores = torch.stack([FD.isc_from_chunk_sums(torch.tensor(float(c["n"]), dtype=torch.float64),
                                                 torch.tensor(c["A"], dtype=torch.float64),
                                                 torch.from_numpy(c["colsum"])) for c in ch])
    assert abs(float(scores.mean()) - float(g["mean_s10_1"])) <= 1e-12 * float(g["mean_s10_1"])
    assert abs(float(scores.std(unbiased=False)) - float(g["std_s10_1"])) <= 1e-12 * float(g["mean_s10_1"])


def test_repivot_of_merge_is_the_identity_of_the_refs():
    rng = np.random.default_rng(1)
    x = (30.0 + rng.standard_normal((25, 4))).astype(np.float32)
    p, q = x[:2].astype(np.float64).mean(axis=0), x[2:6].astype(np.float64).mean(axis=0)
    a, b = R.moments([x], p), R.moments([x], q)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))   # noqa: E731
    s1, S2 = FD._repivot(t([25.0]), t(p), t(R.lower(a["s1"])), t(R.lower(a["S2"])), t(q))
    assert np.max(np.abs(s1.numpy() - R.lower(b["s1"]))) <= 1e-12
    assert np.max(np.abs(S2.numpy() - R.lower(b["S2"]))) <= 1e-11
    assert torch.equal(S2, S2.t())
    r1, r2 = R.repivot(25.0, p, R.lower(a["s1"]), R.lower(a["S2"]), q)
    assert np.max(np.abs(s1.numpy() - r1)) <= 1e-12 and np.max(np.abs(S2.numpy() - r2)) <= 1e-11


def test_argument_checks():
    f = torch.zeros(20, 4)
    with pytest.raises(NotImplementedError):
        FD.kid_features_to_metric(f, f, kid_subset_size=5, kid_kernel="rbf")
    with pytest.raises(ValueError, match="cannot be smaller"):
        FD.kid_features_to_metric(f, f[:4], kid_subset_size=5)
    with pytest.raises(ValueError, match="cannot be smaller"):
        FD.kid_features_to_metric(f[:4], f, kid_subset_size=5)
    with pytest.raises(ValueError):
        FD.kid_features_to_metric(f, torch.zeros(20, 5), kid_subset_size=5)
    with pytest.raises(ValueError):
        FD.kid_features_to_metric(f, f, kid_subset_size=5, kid_kernel_poly_degree=2.5)
    with pytest.raises(ValueError, match="splits"):
        FD.isc_features_to_metric(torch.zeros(9, 3), splits=10)
    with pytest.raises(ValueError):
        FD.isc_features_to_metric(torch.zeros(9), splits=1)
    with pytest.raises(ValueError):
        FD.FeatureStats(0, device="cpu")
    with pytest.raises(ValueError):
        FD.FeatureStats(2049, device="cpu")
    st = FD.FeatureStats(3, device="cpu")
    assert st.state.dtype == torch.float64 and st.state.numel() == 1 + 6 + 9 and st.S2.shape == (3, 3)
    with pytest.raises(ValueError):
        st.update(torch.zeros(2, 4))
    with pytest.raises(ValueError):
        st.merge(FD.FeatureStats(4, device="cpu"))
    with pytest.raises(ValueError):
        st.statistics()
    gen = FD.GenerativeModelModuleWrapper(torch.nn.Linear(4, 4), 4, noise_4d=False)
    ext = lambda im: (im, im)   # noqa: E731
    for kw in (dict(ppl=True), dict(prc=True)):
        with pytest.raises(ValueError, match="not supported"):
            FD.calculate_metrics(gen, ext, 8, None, **kw)
    with pytest.raises(TypeError):
        FD.calculate_metrics(gen, ext, 8, None, verbose=True)
    with pytest.raises(ValueError):
        FD.calculate_metrics(gen, ext, 8, None, isc=False, fid=False, kid=False)
    with pytest.raises(ValueError, match="input2"):
        FD.calculate_metrics(gen, ext, 8, None, isc=False, fid=True)
    with pytest.raises(ValueError, match="feature tensor"):
        FD.calculate_metrics(gen, ext, 8, dict(mu=0, sigma=0), isc=False, fid=False, kid=True)


def test_merge_on_the_host_equals_one_stream():
    """merge is torch fp64 ops: on CPU states filled from the refs it reproduces the single-stream state"""
    g = _gold("fid")
    f = g["f1"][:, :6]
    pa, pb = f[:4].astype(np.float64).mean(axis=0), f[50:53].astype(np.float64).mean(axis=0)
    a, b = R.moments([f[:50]], pa), R.moments([f[50:]], pb)
    whole = R.moments([f], pa)

    def fill(m, p):
        st = FD.FeatureStats(6, device="cpu")
        st.n.fill_(m["n"])
        st.pivot.copy_(torch.from_numpy(p))
        st.s1.copy_(torch.from_numpy(R.lower(m["s1"])))
        st.S2.copy_(torch.from_numpy(R.lower(m["S2"])))
        return st

    st = fill(a, pa).merge(fill(b, pb))
    assert float(st.n) == 101 and np.array_equal(st.pivot.numpy(), pa)
    assert np.max(np.abs(st.S2.numpy() - R.lower(whole["S2"]))) <= 1e-10
    empty = FD.FeatureStats(6, device="cpu").merge(fill(b, pb))
    assert np.array_equal(empty.pivot.numpy(), pb) and np.array_equal(empty.S2.numpy(), R.lower(b["S2"]))
    mu, sigma = st.statistics()["mu"], st.statistics()["sigma"]
    wm, ws = R.statistics(f)
    assert np.max(np.abs(mu - R.lower(wm))) <= 1e-12 and np.max(np.abs(sigma - R.lower(ws))) <= 1e-12
    assert np.array_equal(sigma, sigma.T)
