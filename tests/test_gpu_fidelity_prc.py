"""The Python surface of precision and recall (fidelity.prc_features_to_metric, calculate_prc, the op ffc::prc) on the
GPU against the fixture recorded from the reference's own prc_features_to_metric in fp64
(tests/golden/metrics_prc.npz).  Every row of the fixture's cases is decided beyond 1000 x its rounding bound
(test_prc_refs_cpu.py), so the counts must be the reference's; the reference's means are fp32, hence 2^-24."""
import os

import numpy as np
import pytest
import torch

import abi_bufs as B
from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "metrics_prc.npz"))
DEV = B.DEV


@pytest.fixture(autouse=True)
def _stop_on_a_device_fault():
    yield
    B.end_of_test()


def _fd():
    from fastfourierconvolution_amd import fidelity
    return fidelity


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case,k", [("a", 3), ("a", 1), ("b", 3)])
def test_prc_matches_the_fixture(case, k):
    FD = _fd()
    f1, f2 = _dev(GOLD[f"{case}_f1"]), _dev(GOLD[f"{case}_f2"])
    precision, recall, f_score = (float(v) for v in GOLD[f"{case}_k{k}_0"])
    out = FD.prc_features_to_metric(f1, f2, prc_neighborhood=k)
    assert list(out) == [FD.KEY_METRIC_PRECISION, FD.KEY_METRIC_RECALL, FD.KEY_METRIC_F_SCORE]
    assert all(type(v) is float for v in out.values())
    print(f"OBS prc {case} k={k}: {out} fixture {(precision, recall, f_score)}")
    for got, want, n in ((out[FD.KEY_METRIC_PRECISION], precision, len(f2)), (out[FD.KEY_METRIC_RECALL], recall, len(f1))):
        count = round(want * n)
        assert round(got * n) == count and abs(got - count / n) <= 2.0 ** -24 and abs(got - want) <= 2.0 ** -24
    assert abs(out[FD.KEY_METRIC_F_SCORE] - f_score) <= 1e-6
    assert FD.prc_features_to_metric(f1, f2, prc_neighborhood=k, prc_batch_size=37, save_cpu_ram=True) == out
    if k == 3:
        assert FD.prc_features_to_metric(f1, f2) == out   # the default neighborhood
    with pytest.raises(ValueError, match="samples"):
        FD.prc_features_to_metric(f1[:k], f2, prc_neighborhood=k)


def test_op_outputs_and_graph_replay_with_new_features():
    a1, a2 = GOLD["a_f1"], GOLD["a_f2"]
    rng = np.random.default_rng(3)
    b1 = (a1 + 0.5 * rng.standard_normal(a1.shape)).astype(np.float32)
    b2 = (a2 + 0.5 * rng.standard_normal(a2.shape)).astype(np.float32)
    eager_a = torch.ops.ffc.prc(_dev(a1), _dev(a2), 3)
    eager_b = torch.ops.ffc.prc(_dev(b1), _dev(b2), 3)
    assert [tuple(t.shape) for t in eager_a] == [(101,), (90,), (90,), (101,), (2,)]
    assert [t.dtype for t in eager_a] == [torch.float64, torch.float64, torch.int32, torch.int32, torch.float64]
    assert eager_a[4].tolist() == [23.0, 14.0] and eager_a[4].tolist() == [float(eager_a[2].sum()), float(eager_a[3].sum())]
    assert eager_b[4].tolist() != eager_a[4].tolist()
    s1, s2 = _dev(a1), _dev(a2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.ffc.prc(s1, s2, 3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.ffc.prc(s1, s2, 3)
    for src, eager in (((a1, a2), eager_a), ((b1, b2), eager_b), ((a1, a2), eager_a)):
        s1.copy_(_dev(src[0]))
        s2.copy_(_dev(src[1]))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, e) for o, e in zip(out, eager))


def test_calculate_prc_with_a_stub_generator_and_extractor():
    FD = _fd()
    torch.manual_seed(0)
    net = torch.nn.Linear(6, 3 * 4 * 4).to(DEV)

    class Gen(torch.nn.Module):
        def forward(self, z):
            return (255 * torch.sigmoid(net(z))).to(torch.uint8).reshape(-1, 3, 4, 4)

    proj = torch.randn(48, 9, generator=torch.Generator().manual_seed(1)).to(DEV)
    seen = []

    def extractor(images):
        assert images.dtype == torch.uint8 and images.shape[1:] == (3, 4, 4)
        f = (images.float().flatten(1) / 255.0) @ proj
        seen.append(f)
        return f

    real = _dev((0.5 * np.random.default_rng(2).standard_normal((40, 9)) + 1.5).astype(np.float32))
    wrapper = FD.GenerativeModelModuleWrapper(Gen(), 6, noise_4d=False)
    out = FD.calculate_prc(wrapper, extractor, 50, real, batch_size=32, prc_neighborhood=2)
    assert [len(f) for f in seen] == [32, 18]
    want = FD.prc_features_to_metric(real, torch.cat(seen), prc_neighborhood=2)
    assert out == want and set(out) == {"precision", "recall", "f_score"}
    # an extractor that returns (features, logits), as calculate_metrics takes one
    assert FD.calculate_prc(wrapper, lambda im: (extractor(im), None), 50, real, batch_size=32, prc_neighborhood=2) == want
