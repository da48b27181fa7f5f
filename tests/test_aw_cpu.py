"""CPU checks of the adaptive-weight loss surface: tests/aw_refs.py against the fixture recorded from
the reference's aw_method in float64 (tests/golden/gen_golden_aw.py), the exported names and
signatures, and the library's bindings.  No GPU needed."""
import inspect

import numpy as np
import pytest

import aw_refs


@pytest.fixture(scope="module")
def cases():
    return aw_refs.load_cases()


def test_fixture_covers_every_case_of_both_algorithms(cases):
    assert sorted((c["kw"]["normalized"], c["case"]) for c in cases) == \
        [(n, k) for n in (False, True) for k in (1, 2, 3, 4, 5)]
    from fastfourierconvolution_amd import _lib
    chunk = _lib.load().ffc_aw_chunk()
    sizes = [a.size for a in cases[0]["a"]]
    assert chunk + 1 in sizes and len(sizes) > 16 and 1 in sizes and 0 not in sizes


def test_refs_reproduce_the_reference(cases):
    """The reference's dots (torch.dot in fp64) and aw_refs' (correctly rounded) each carry at most
    n u sum |x y| (u = 2^-53); at |cosine| = 0.5 that is 2 n u of rdotf and n u of rdotr / fdotf, so a
    weight ((rdotf / fdotf) / sqrt(rdotr) at worst) is within 4 n u, and so are the loss and, per
    element, the gradient against |w_r a| + |w_f b|."""
    for c in cases:
        ref = aw_refs.aw_reference(c["a"], c["b"], c["real"], c["fake"], **c["kw"])
        assert ref["case"] == c["case"], c["hyper"]
        rel = 4 * ref["n"] * aw_refs.U
        h = c["hyper"]
        loss = ref["w_r"] * h["c_r"] + ref["w_f"] * h["c_f"]
        assert abs(loss - c["loss"]) <= rel * (abs(ref["w_r"] * h["c_r"]) + abs(ref["w_f"] * h["c_f"]))
        for g, a, b, want in zip(ref["grads"], c["a"], c["b"], c["grads"]):
            assert want.dtype == np.float64 and want.shape == a.shape
            bound = rel * (np.abs(ref["w_r"] * a.astype(np.float64)) + np.abs(ref["w_f"] * b.astype(np.float64)))
            assert np.all(np.abs(g - want) <= bound), (c["hyper"], float(np.abs(g - want).max()))
    # the weights are told apart by the fixture: two cases' gradients differ by far more than the bound
    g0, g1 = cases[0]["grads"][3], cases[1]["grads"][3]
    assert np.abs(g0 - g1).max() > 1e-6


def test_exported_with_the_reference_signature():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import training
    assert "aw_method" in F.__all__ and isinstance(F.aw_method, type)
    ns = {}
    exec("from fastfourierconvolution_amd import *", ns)
    assert ns["aw_method"] is F.aw_method
    ctor = inspect.signature(F.aw_method.__init__)
    assert [(p.name, p.default) for p in list(ctor.parameters.values())[1:]] == \
        [("alpha1", 0.5), ("alpha2", 0.75), ("delta", 0.05), ("epsilon", 0.05), ("normalized_aw", True)]
    assert list(inspect.signature(F.aw_method.aw_loss).parameters) == \
        ["self", "Dloss_real", "Dloss_fake", "Dis_opt", "Dis_Net", "real_validity", "fake_validity"]
    assert list(inspect.signature(training.aw_discriminator_step).parameters) == \
        ["G", "D", "optim_G", "optim_D", "z", "real", "aw", "noises", "labels"]
    assert callable(training.hinge_loss_real) and callable(training.hinge_loss_fake)


def test_alpha_order_asserts():
    import fastfourierconvolution_amd as F
    F.aw_method(0.4, 0.6)
    for a1, a2 in ((0.75, 0.75), (0.8, 0.5)):
        with pytest.raises(AssertionError):
            F.aw_method(alpha1=a1, alpha2=a2)


def test_hinge_halves_sum_to_hinge_loss_dis():
    import torch
    from fastfourierconvolution_amd import training as T
    g = torch.Generator().manual_seed(0)
    real, fake = 2 * torch.randn(8, 1, generator=g), 2 * torch.randn(8, 1, generator=g)
    assert torch.equal(T.hinge_loss_real(real) + T.hinge_loss_fake(fake), T.hinge_loss_dis(fake, real))


def test_entry_points_bound_and_validated_without_gpu():
    import ctypes
    from fastfourierconvolution_amd import _lib
    lib = _lib.load()
    assert lib.ffc_abi_version() == 4
    bound = {s[0] for s in _lib.SIGNATURES}
    assert {"ffc_aw_chunk", "ffc_aw_ws_doubles", "ffc_aw_weights", "ffc_aw_combine"} <= bound
    chunk = lib.ffc_aw_chunk()
    numel = (ctypes.c_longlong * 4)(1, 0, chunk, chunk + 1)
    assert lib.ffc_aw_ws_doubles(numel, 4) == 3 * (1 + 0 + 1 + 2) + 1
    # rejected before any launch, with a readable error (the pointers are never dereferenced)
    p = (ctypes.c_void_p * 1)(64)
    one = (ctypes.c_longlong * 1)(8)
    rc = lib.ffc_aw_weights(p, p, one, 1, 64, 4, 64, 4, 0.75, 0.5, 0.05, 0.05, 1, 0, 64, 4, 64, None)
    assert rc == -1 and b"alpha1 < alpha2" in lib.ffc_last_error()
    rc = lib.ffc_aw_weights(p, p, one, 1, 64, 4, 64, 4, 0.5, 0.75, 0.05, 0.05, 1, 0, 64, 2, 64, None)
    assert rc == -1 and b"workspace too small" in lib.ffc_last_error()
    rc = lib.ffc_aw_combine(p, p, p, one, 1, 64, 0, None)
    assert rc == -1 and b"alias" in lib.ffc_last_error()


def test_module_refuses_cpu_parameters():
    import torch
    import fastfourierconvolution_amd as F
    net = torch.nn.Linear(3, 1)
    out = net(torch.randn(2, 3))
    with pytest.raises(NotImplementedError, match="fp32 parameters on the GPU"):
        F.aw_method().aw_loss(out.mean(), -out.mean(), None, net, out, out)
