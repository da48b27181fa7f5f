"""The Python surface of the metrics (fidelity.FeatureStats, kid_features_to_metric, isc_features_to_metric,
calculate_metrics) on the GPU, against the golden fixtures recorded from the reference's own metric functions
(tests/golden/metrics_*.npz) and the wide references of tests/metric_refs.py.  U = 2^-53.

Tolerances, propagated from the sums' bounds of metric_refs.py:
  FID statistics  sigma = (S2 - n d d^T) / (n - 1): the moments bound (n + 4) U sum |x - mu||x - mu|^T divided by
                  n - 1, around the state's own pivot p; mu = p + s1 / n: (n + 2) U sum |x - p| / n + U |mu|
  FID scalar      1e-9 (tr sigma1 + tr sigma2 + |mu1 - mu2|^2): the host eigen-solve is the reference's own code, so
                  only the statistics differ
  KID             per subset |d mmd2| <= (b_xx + b_dxx + b_yy + b_dyy) / (m (m - 1)) + 2 b_xy / m^2 with b the six
                  sums' bounds; the mean over subsets moves by at most the largest of these and the population std,
                  which is 1-Lipschitz in the rms of the per-subset errors, too; plus (subsets + 4) U max |mmd2| for
                  the mean / std arithmetic itself
  ISC             per chunk |d exp(E)| <= exp(E) expm1(b_E) with b_E the exponent's bound; mean and std over the
                  chunks as for KID
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import abi_bufs as B
import metric_refs as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = B.DEV


@pytest.fixture(autouse=True)
def _stop_on_a_device_fault():
    yield
    B.end_of_test()


def _gold(name):
    return np.load(os.path.join(GOLD, f"metrics_{name}.npz"))


def _fd():
    from fastfourierconvolution_amd import fidelity
    return fidelity


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stats_bounds(f, pivot):
    x = f.astype(np.float64)
    n = len(x)
    mu = x.mean(axis=0)
    a = np.abs(x - pivot)
    return (n + 2) * R.U * a.sum(axis=0) / n + R.U * np.abs(mu), (n + 4) * R.U * (a.T @ a) / (n - 1)


def _check_stats(st, f, mu, sigma, what):
    got = st.statistics()
    bm, bs = _stats_bounds(f, st.pivot.cpu().numpy())
    em, es = np.abs(got["mu"] - mu) / bm, np.abs(got["sigma"] - sigma) / bs
    print(f"OBS {what}: mu {em.max():.3f} sigma {es.max():.3f} of the bound")
    assert got["mu"].dtype == np.float64 and got["sigma"].dtype == np.float64
    assert em.max() <= 1.0 and es.max() <= 1.0
    assert np.array_equal(got["sigma"], got["sigma"].T)


def _stream_in(f, sizes):
    st = _fd().FeatureStats(f.shape[1])
    at = 0
    for b in sizes:
        st.update(_dev(f[at:at + b]))
        at += b
    assert at == len(f)
    return st


def test_feature_stats_match_the_fixture_and_fid():
    g = _gold("fid")
    FD = _fd()
    st1, st2 = _stream_in(g["f1"], (64, 36, 1)), _stream_in(g["f2"], (77,))
    _check_stats(st1, g["f1"], g["mu1"], g["sigma1"], "f1 against the fixture")
    _check_stats(st2, g["f2"], g["mu2"], g["sigma2"], "f2 against the fixture")
    wm, ws = R.statistics(g["f1"])
    _check_stats(st1, g["f1"], R.lower(wm), R.lower(ws), "f1 against the wide reference")
    s1, s2 = st1.statistics(), st2.statistics()
    fid = FD.fid_statistics_to_metric(s1, s2)[FD.KEY_METRIC_FID]
    tol = 1e-9 * (np.trace(g["sigma1"]) + np.trace(g["sigma2"]) + float(np.sum((g["mu1"] - g["mu2"]) ** 2)))
    print(f"OBS fid {fid!r} fixture {float(g['fid'])!r} tol {tol:.3e}")
    assert abs(fid - float(g["fid"])) <= tol


def test_merge_all_reduce_and_update_after_statistics():
    g = _gold("fid")
    f = g["f1"]
    FD = _fd()
    one = _stream_in(f, (50, 51))
    a, b = _stream_in(f[:50], (50,)), _stream_in(f[50:], (30, 21))
    assert not torch.equal(a.pivot, b.pivot)
    a.merge(b)
    wm, ws = R.statistics(f)
    _check_stats(a, f, R.lower(wm), R.lower(ws), "merge of two halves")
    _check_stats(one, f, R.lower(wm), R.lower(ws), "one stream")
    assert float(a.n.item()) == 101 and torch.equal(a.pivot, one.pivot)
    empty = FD.FeatureStats(130).merge(b)
    assert torch.equal(empty.state, b.state)
    # update after statistics() continues the same state
    st = _stream_in(f[:64], (64,))
    st.statistics()
    st.update(_dev(f[64:]))
    _check_stats(st, f, R.lower(wm), R.lower(ws), "update after statistics()")
    ref = _stream_in(f, (64, 37))
    assert torch.equal(st.state, ref.state)


def test_all_reduce_in_a_one_rank_group_leaves_the_state():
    import socket
    import torch.distributed as dist
    g = _gold("fid")
    st = _stream_in(g["f2"], (40, 37))
    before = st.state.clone()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        st.all_reduce()
        st.all_reduce(group=dist.group.WORLD)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert torch.equal(st.state, before)


def test_kid_matches_the_fixture():
    g = _gold("kid")
    FD = _fd()
    f1, f2 = _dev(g["f1"]), _dev(g["f2"])
    for kw, rkw, tag in ((dict(), dict(), ""),
                         (dict(kid_kernel_poly_degree=1, kid_kernel_poly_gamma=0.25, kid_kernel_poly_coef0=0.5),
                          dict(degree=1, gamma=0.25, coef0=0.5), "_d1")):
        out = FD.kid_features_to_metric(f1, f2, kid_subsets=3, kid_subset_size=17, **kw)
        assert list(out) == [FD.KEY_METRIC_KID_MEAN, FD.KEY_METRIC_KID_STD]
        mean, std, tol = R.kid_metric(g["f1"], g["f2"], 3, 17, **rkw)
        em = max(abs(out[FD.KEY_METRIC_KID_MEAN] - float(g["mean" + tag])), abs(out[FD.KEY_METRIC_KID_MEAN] - mean))
        es = max(abs(out[FD.KEY_METRIC_KID_STD] - float(g["std" + tag])), abs(out[FD.KEY_METRIC_KID_STD] - std))
        print(f"OBS kid{tag}: mean err {em:.3e} std err {es:.3e} tol {tol:.3e}")
        assert em <= tol and es <= tol
    with pytest.raises(ValueError, match="cannot be smaller"):
        FD.kid_features_to_metric(f1, f2, kid_subset_size=91)


def test_isc_matches_the_fixture():
    g = _gold("isc")
    FD = _fd()
    lg = _dev(g["logits"])
    for splits in (1, 10):
        for shuffle in (True, False):
            out = FD.isc_features_to_metric(lg, splits=splits, shuffle=shuffle)
            assert list(out) == [FD.KEY_METRIC_ISC_MEAN, FD.KEY_METRIC_ISC_STD]
            mean, std, tol = R.isc_metric(g["logits"], splits, shuffle)
            key = f"s{splits}_{int(shuffle)}"
            em = max(abs(out[FD.KEY_METRIC_ISC_MEAN] - float(g["mean_" + key])), abs(out[FD.KEY_METRIC_ISC_MEAN] - mean))
            es = max(abs(out[FD.KEY_METRIC_ISC_STD] - float(g["std_" + key])), abs(out[FD.KEY_METRIC_ISC_STD] - std))
            print(f"OBS isc {key}: mean err {em:.3e} std err {es:.3e} tol {tol:.3e}")
            assert em <= tol and es <= tol
    with pytest.raises(ValueError, match="splits"):
        FD.isc_features_to_metric(lg[:9], splits=10)


def test_graph_capture_of_two_updates_replays_to_the_eager_state():
    g = _gold("fid")
    FD = _fd()
    a, b = _dev(g["f1"][:64]), _dev(g["f1"][64:])
    eager = FD.FeatureStats(130).update(a).update(b)
    st = FD.FeatureStats(130)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.update(a).update(b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    st.state.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.update(a).update(b)
    torch.cuda.synchronize()
    assert float(st.n.item()) == 0.0   # capture records without running
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.state, eager.state)


def test_calculate_metrics_end_to_end():
    import fastfourierconvolution_amd as F
    FD = _fd()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        G = F.FGenerator32(128, 4).to(DEV).eval()
    gen = torch.Generator().manual_seed(5)
    l1, l2 = torch.nn.Linear(3 * 32 * 32, 40), torch.nn.Linear(40, 10)
    with torch.no_grad():
        for p in list(l1.parameters()) + list(l2.parameters()):
            p.copy_(torch.randn(p.shape, generator=gen) * (0.02 if p.dim() == 2 and p.shape[1] > 40 else 0.3))
    l1, l2 = l1.to(DEV), l2.to(DEV)
    seen = []

    def extractor(images):
        assert images.dtype == torch.uint8 and images.shape[1:] == (3, 32, 32)
        with torch.no_grad():
            f = l1(images.float().flatten(1) / 255.0)
            lg = l2(f)
        seen.append((f.cpu().numpy(), lg.cpu().numpy()))
        return f, lg

    real = (0.2 + 1.1 * np.random.default_rng(8).standard_normal((70, 40))).astype(np.float32)
    wrapper = FD.GenerativeModelModuleWrapper(G, 128)
    out = FD.calculate_metrics(wrapper, extractor, 96, _dev(real), isc=True, fid=True, kid=True, batch_size=64,
                               kid_subsets=3, kid_subset_size=17)
    assert [s[0].shape[0] for s in seen] == [64, 32]
    assert set(out) == {FD.KEY_METRIC_FID, FD.KEY_METRIC_ISC_MEAN, FD.KEY_METRIC_ISC_STD, FD.KEY_METRIC_KID_MEAN,
                        FD.KEY_METRIC_KID_STD}
    feats, logits = np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])
    (m1, s1), (m2, s2) = R.statistics(feats), R.statistics(real)
    fid = R.fid_from_statistics(R.lower(m1), R.lower(s1), R.lower(m2), R.lower(s2))
    tol = 1e-9 * (float(np.trace(R.lower(s1)) + np.trace(R.lower(s2))) + float(np.sum(R.lower(m1 - m2) ** 2)))
    fid_tol = tol
    assert abs(out[FD.KEY_METRIC_FID] - fid) <= tol, (out[FD.KEY_METRIC_FID], fid, tol)
    mean, std, tol = R.isc_metric(logits, 10, True)
    assert abs(out[FD.KEY_METRIC_ISC_MEAN] - mean) <= tol and abs(out[FD.KEY_METRIC_ISC_STD] - std) <= tol
    mean, std, tol = R.kid_metric(feats, real, 3, 17)
    assert abs(out[FD.KEY_METRIC_KID_MEAN] - mean) <= tol and abs(out[FD.KEY_METRIC_KID_STD] - std) <= tol
    # the three requested keys only, from cached statistics
    seen.clear()
    out2 = FD.calculate_metrics(wrapper, extractor, 96, dict(mu=R.lower(m2), sigma=R.lower(s2)), isc=True, fid=True)
    assert set(out2) == {FD.KEY_METRIC_FID, FD.KEY_METRIC_ISC_MEAN, FD.KEY_METRIC_ISC_STD}
    assert abs(out2[FD.KEY_METRIC_FID] - fid) <= fid_tol and out2[FD.KEY_METRIC_ISC_MEAN] == out[FD.KEY_METRIC_ISC_MEAN]
