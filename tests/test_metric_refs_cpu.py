"""tests/metric_refs.py against plain numpy fp64 and the golden fixtures (tests/golden/metrics_*.npz, recorded from
the reference's own metric functions by tests/golden/gen_golden_metrics.py), without a GPU: the restatements the GPU
tests compare against are themselves the reference's quantities."""
import os

import numpy as np

import metric_refs as R
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


def _gold(name):
    return np.load(os.path.join(GOLD, f"metrics_{name}.npz"))


def test_wide_type():
    assert R.WIDE == (np.finfo(np.longdouble).nmant >= 63)
    a = R.lift(np.array([1.5, -2.25], dtype=np.float32))
    assert np.array_equal(R.lower(a), [1.5, -2.25])


def test_statistics_match_numpy_and_the_fixture():
    g = _gold("fid")
    for f, mu, sigma in ((g["f1"], g["mu1"], g["sigma1"]), (g["f2"], g["mu2"], g["sigma2"])):
        m, s = R.statistics(f)
        x = f.astype(np.float64)
        scale = np.abs(x - mu).T @ np.abs(x - mu) / (len(x) - 1)
        assert np.max(np.abs(R.lower(m) - x.mean(axis=0))) <= 1e-13 * 100
        assert np.all(np.abs(R.lower(s) - np.cov(x, rowvar=False)) <= (len(x) + 4) * R.U * scale + 1e-13)
        assert np.all(np.abs(R.lower(s) - sigma) <= 1e-12 * (1 + scale))   # the fixture's one-pass fp64 at offset 100
        assert np.allclose(R.lower(m), mu, rtol=1e-14, atol=0)


def test_moments_around_a_pivot_give_the_same_statistics():
    g = _gold("fid")
    f = g["f1"]
    pivot = f[:7].astype(np.float64).mean(axis=0)
    m = R.moments([f[:7], f[7:50], f[50:]], pivot)
    mu, sigma = R.statistics_from_state(m["n"], pivot, R.lower(m["s1"]), R.lower(m["S2"]))
    wm, ws = R.statistics(f)
    assert m["n"] == 101
    assert np.max(np.abs(mu - R.lower(wm))) <= 1e-13
    assert np.max(np.abs(sigma - R.lower(ws))) <= 1e-13
    b1, b2 = R.moments_bounds(m)
    assert b1.shape == (130,) and b2.shape == (130, 130) and (b2 > 0).all()


def test_repivot_identity():
    rng = np.random.default_rng(0)
    x = (50.0 + rng.standard_normal((40, 6))).astype(np.float32)
    p, q = x[:3].astype(np.float64).mean(axis=0), x[3:9].astype(np.float64).mean(axis=0)
    a, b = R.moments([x], p), R.moments([x], q)
    s1, S2 = R.repivot(40, p, R.lower(a["s1"]), R.lower(a["S2"]), q)
    assert np.max(np.abs(s1 - R.lower(b["s1"]))) <= 1e-12
    assert np.max(np.abs(S2 - R.lower(b["S2"]))) <= 1e-11


def test_fid_formula_matches_the_fixture():
    g = _gold("fid")
    assert R.fid_from_statistics(g["mu1"], g["sigma1"], g["mu2"], g["sigma2"]) == float(g["fid"])


def test_kid_matches_numpy_and_the_fixture():
    g = _gold("kid")
    f1, f2 = g["f1"], g["f2"]
    i1, i2 = R.kid_tables(len(f1), len(f2), 3, 17)
    sums, bounds = R.kid_sums(f1, f2, i1, i2, 3, 1.0 / 130, 1.0)
    x, y = f1[i1[0]].astype(np.float64), f2[i2[0]].astype(np.float64)
    kxy = (x @ y.T / 130 + 1.0) ** 3
    assert abs(float(sums[0, 4]) - kxy.sum()) <= 2 * bounds[0, 4] and abs(float(sums[0, 5]) - np.trace(kxy)) <= 2 * bounds[0, 5]
    for kw, tag in ((dict(), ""), (dict(degree=1, gamma=0.25, coef0=0.5), "_d1")):
        mean, std, tol = R.kid_metric(f1, f2, 3, 17, **kw)
        assert abs(mean - float(g["mean" + tag])) <= tol and abs(std - float(g["std" + tag])) <= tol
        assert tol < 1e-9


def test_isc_matches_numpy_and_the_fixture():
    g = _gold("isc")
    lg = g["logits"]
    for splits in (1, 10):
        for shuffle in (True, False):
            mean, std, tol = R.isc_metric(lg, splits, shuffle)
            assert abs(mean - float(g[f"mean_s{splits}_{int(shuffle)}"])) <= tol
            assert abs(std - float(g[f"std_s{splits}_{int(shuffle)}"])) <= tol
            assert tol < 1e-8
    ch = R.isc_chunks(lg, R.isc_perm(101, False), 10)
    assert [c["n"] for c in ch] == [10, 10, 10, 10, 10, 10, 10, 10, 10, 11]
    x = lg[:10].astype(np.float64)
    p = np.exp(x - x.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    assert np.max(np.abs(ch[0]["colsum"] - p.sum(axis=0))) <= 1e-14


def test_isc_chunk_boundaries_at_23():
    ch = R.isc_chunks(np.zeros((23, 3), dtype=np.float32), np.arange(23), 10)
    assert [c["n"] for c in ch] == [2, 2, 2, 3, 2, 2, 3, 2, 2, 3]   # i * 23 // 10: 0 2 4 6 9 11 13 16 18 20 23
    assert all(abs(c["E"]) <= 1e-18 for c in ch)
