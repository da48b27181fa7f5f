"""The host side of fidelity.prc_features_to_metric / calculate_prc without a GPU: the names and the op exist, the
C entry points are bound, and the argument checks raise ValueError before anything reaches the device."""
import pytest
import torch

from fastfourierconvolution_amd import _lib
from fastfourierconvolution_amd import fidelity as FD


def test_names_op_and_signatures():
    for name in ("prc_features_to_metric", "calculate_prc"):
        assert name in FD.__all__ and callable(getattr(FD, name))
    assert (FD.KEY_METRIC_PRECISION, FD.KEY_METRIC_RECALL, FD.KEY_METRIC_F_SCORE) == ("precision", "recall", "f_score")
    assert hasattr(torch.ops.ffc, "prc")
    names = [s[0] for s in _lib.SIGNATURES]
    assert "ffc_prc_ws_bytes" in names and "ffc_prc" in names
    lib = _lib.load()
    assert 0 < lib.ffc_prc_ws_bytes(50000, 50000, 3) < 128 * 2 ** 20
    for bad in ((3, 50, 3), (50, 3, 3), (50, 50, 0), (50, 50, 8), (64 * 65535 + 1, 50, 3)):
        assert lib.ffc_prc_ws_bytes(*bad) == 0, bad
    assert lib.ffc_prc_ws_bytes(4, 4, 3) == 8 * (4 + 4 + 4 * 4)


def test_fake_kernel_gives_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.ffc.prc(torch.empty(11, 6), torch.empty(9, 6), 3)
    assert [tuple(t.shape) for t in out] == [(11,), (9,), (9,), (11,), (2,)]
    assert [t.dtype for t in out] == [torch.float64, torch.float64, torch.int32, torch.int32, torch.float64]


def test_argument_checks():
    f = torch.zeros(20, 4)
    with pytest.raises(ValueError, match="2-D"):
        FD.prc_features_to_metric(f[0], f)
    with pytest.raises(ValueError, match="2-D"):
        FD.prc_features_to_metric(f, f.numpy())
    with pytest.raises(ValueError, match="one width"):
        FD.prc_features_to_metric(f, torch.zeros(20, 5))
    for k in (0, 8, -1, 2.0, None):
        with pytest.raises(ValueError, match="prc_neighborhood"):
            FD.prc_features_to_metric(f, f, prc_neighborhood=k)
    with pytest.raises(ValueError, match="at least 4 samples"):
        FD.prc_features_to_metric(f[:3], f)
    with pytest.raises(ValueError, match="at least 8 samples"):
        FD.prc_features_to_metric(f, f[:7], prc_neighborhood=7, prc_batch_size=5, save_cpu_ram=True)
    gen = FD.GenerativeModelModuleWrapper(torch.nn.Linear(4, 4), 4, noise_4d=False)
    with pytest.raises(ValueError, match="real_features"):
        FD.calculate_prc(gen, lambda im: im, 8, None)
    with pytest.raises(ValueError, match="GenerativeModel"):
        FD.calculate_prc(torch.nn.Linear(4, 4), lambda im: im, 8, f)
