"""CPU checks of the spectral-norm HIP path's parts that need no GPU: the float64 restatement
(tests/sn_refs.py) against torch's own hook, set_sn_hip, the matrix view handed to the kernels, and
the argument validation of the ffc_sn_* entry points.

Bounds: the restatement against the hook on a .double() module 1e-10 normwise (same formula, same
precision), against the fp32 hook 1e-5 normwise (the project's fp32-vs-fp64 kernel bound)."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm

import sn_refs as R
from fastfourierconvolution_amd import _lib

MODULES = {
    "conv": lambda: nn.Conv2d(5, 7, 3),
    "convT": lambda: nn.ConvTranspose2d(6, 10, 4),   # dim = 1
    "linear": lambda: nn.Linear(33, 9),
}


def _module(kind, dtype):
    torch.manual_seed(7)
    return spectral_norm(MODULES[kind]()).to(dtype)


def _state(m):
    return m.weight_orig.detach().clone(), m.weight_u.clone(), m.weight_v.clone()


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("kind", sorted(MODULES))
def test_restatement_matches_the_hook_in_float64(kind, training):
    m = _module(kind, torch.float64).train(training)
    w0, u0, v0 = _state(m)
    dim = R.sn_hook(m).dim
    assert dim == (1 if kind == "convT" else 0)
    w, u, v = R.run_hook(m)
    rw, ru, rv, _ = R.sn_ref(w0, u0, v0, dim, training)
    for name, a, b in (("w", w, rw), ("u", u, ru), ("v", v, rv)):
        e = R.normwise(a, b)
        print(f"  {kind} train={training} {name}: {e:.2e}")
        assert e <= 1e-10
    if not training:
        assert torch.equal(m.weight_u, u0) and torch.equal(m.weight_v, v0)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("kind", sorted(MODULES))
def test_backward_matches_autograd_through_the_hook(kind, training):
    m = _module(kind, torch.float64).train(training)
    w0, u0, v0 = _state(m)
    dim = R.sn_hook(m).dim
    w, _, _ = R.run_hook(m)
    g = torch.randn(w.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    (grad,) = torch.autograd.grad((w * g).sum(), m.weight_orig)
    _, ru, rv, sigma = R.sn_ref(w0, u0, v0, dim, training)
    e = R.normwise(grad, R.sn_ref_backward(g, w0, ru, rv, sigma, dim))
    print(f"  {kind} train={training} dW_orig: {e:.2e}")
    assert e <= 1e-10


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("kind", sorted(MODULES))
def test_restatement_against_the_fp32_hook(kind, training):
    m = _module(kind, torch.float32).train(training)
    w0, u0, v0 = _state(m)
    w, u, v = R.run_hook(m)
    rw, ru, rv, _ = R.sn_ref(w0, u0, v0, R.sn_hook(m).dim, training)
    for name, a, b in (("w", w, rw), ("u", u, ru), ("v", v, rv)):
        e = R.normwise(a, b)
        print(f"  {kind} train={training} {name}: {e:.2e}")
        assert e <= 1e-5


def test_from_matrix_inverts_to_matrix():
    w = torch.randn(3, 4, 2, 2, dtype=torch.float64)
    for dim in (0, 1):
        assert torch.equal(R.from_matrix(R.to_matrix(w, dim), w.shape, dim), w)


def test_matrix_view_reads_the_weight_in_place():
    """Wm[m][k] = w.flat[(k // R) * stride_i + m * stride_m + k % R], the view of ffc_sn_job"""
    from fastfourierconvolution_amd._autograd import sn_view
    for shape, dim in (((7, 5, 3, 3), 0), ((6, 10, 4, 4), 1), ((9, 33), 0), ((1, 8, 2, 2), 1), ((5, 3), 1)):
        w = torch.arange(float(torch.Size(shape).numel())).reshape(shape)
        M, K, Rr, sm, si = sn_view(shape, dim)
        wm = R.to_matrix(w, dim)
        assert tuple(wm.shape) == (M, K)
        m = torch.arange(M).view(-1, 1)
        k = torch.arange(K).view(1, -1)
        idx = (k // Rr) * si + m * sm + k % Rr
        assert torch.equal(w.reshape(-1)[idx], wm), (shape, dim)
    with pytest.raises(NotImplementedError):
        sn_view((4, 5, 6), 2)


# --------------------------------------------------------------------------- set_sn_hip
def _critic():
    return nn.Sequential(spectral_norm(nn.Conv2d(3, 8, 3)), nn.ReLU(), nn.Conv2d(8, 8, 1),
                         spectral_norm(nn.ConvTranspose2d(8, 4, 4)), spectral_norm(nn.Linear(4, 2)))


def test_set_sn_hip_marks_and_unmarks():
    import fastfourierconvolution_amd as F
    model = _critic()
    keys = list(model.state_dict().keys())
    wrapped = [model[0], model[3], model[4]]
    assert not any(m.__dict__.get("sn_hip") for m in model.modules())   # off by default
    assert F.set_sn_hip(model) is model
    assert all(m.__dict__.get("sn_hip") is True for m in wrapped)
    assert not model[2].__dict__.get("sn_hip") and not model[1].__dict__.get("sn_hip")
    assert list(model.state_dict().keys()) == keys
    assert all(R.sn_hook(m) is not None for m in wrapped)               # the hook stays registered
    assert all(m.__dict__.get("sn_hip") for m in copy.deepcopy(model).modules() if hasattr(m, "weight_orig"))
    assert F.set_sn_hip(model, False) is model
    assert not any(m.__dict__.get("sn_hip") for m in model.modules())
    assert list(model.state_dict().keys()) == keys
    plain = nn.Sequential(nn.Conv2d(3, 4, 3), nn.ReLU())
    assert F.set_sn_hip(plain) is plain
    assert not any("sn_hip" in m.__dict__ for m in plain.modules())


def test_set_sn_hip_off_leaves_the_hook_path_untouched_on_cpu():
    """a module that was switched on and off again runs torch's hook: same results as a fresh copy"""
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _runtime as rt
    m = _module("conv", torch.float32).train()
    ref = copy.deepcopy(m)
    F.set_sn_hip(F.set_sn_hip(m), False)
    rt.sn_refresh_train(m)
    w, u, v = R.run_hook(ref)
    assert torch.equal(m.weight, w) and torch.equal(m.weight_u, u) and torch.equal(m.weight_v, v)


def test_set_sn_hip_refuses_what_the_kernels_do_not_do():
    import fastfourierconvolution_amd as F
    two = nn.Sequential(spectral_norm(nn.Conv2d(3, 4, 3)), spectral_norm(nn.Linear(4, 4), n_power_iterations=2))
    with pytest.raises(NotImplementedError, match="1.*n_power_iterations"):
        F.set_sn_hip(two)
    assert not any(m.__dict__.get("sn_hip") for m in two.modules())     # nothing half switched
    par = nn.Sequential(torch.nn.utils.parametrizations.spectral_norm(nn.Linear(4, 4)))
    with pytest.raises(NotImplementedError, match="parametrizations"):
        F.set_sn_hip(par)
    half = nn.Sequential(spectral_norm(nn.Linear(4, 4)).double())
    with pytest.raises(NotImplementedError, match="fp32"):
        F.set_sn_hip(half)
    F.set_sn_hip(two, False)   # switching off never raises


def test_hip_path_has_no_cpu_fallback():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _runtime as rt
    m = F.set_sn_hip(_module("linear", torch.float32))
    with pytest.raises(_lib.FFCError):
        rt.sn_refresh_train(m)
    with pytest.raises(_lib.FFCError):
        rt.sn_refresh(m)


# --------------------------------------------------------------------------- C ABI
def _job(M=8, K=16, ws_off=0):
    fake = 1 << 20   # never dereferenced: every case below is refused before a launch
    return _lib.SnJob(w_orig=fake, u=fake, v=fake, w=fake + 4096, sigma=fake, dw=fake, dw_orig=fake + 8192, M=M, K=K,
                      R=K, stride_m=K, stride_i=0, ws_off=ws_off)


def test_sn_abi_argument_validation():
    lib = _lib.load()
    out = (ctypes.c_int * 12)()
    assert lib.ffc_struct_sizes(out, 12) == 0 and out[11] == ctypes.sizeof(_lib.SnJob)
    assert lib.ffc_abi_version() == 4   # additions only
    need = lib.ffc_sn_ws_bytes(8, 16)
    assert need > 0 and need % 16 == 0
    assert lib.ffc_sn_ws_bytes(0, 16) == 0 and lib.ffc_sn_ws_bytes(8, -1) == 0
    assert lib.ffc_sn_ws_bytes(1 << 16, 1 << 15) == 0   # M * K = 2^31
    # partial columns (ceil(M / 64) x K) + partial rows (ceil(K / 2048) x M) floats at least
    assert lib.ffc_sn_ws_bytes(512, 8192) >= 4 * (8 * 8192 + 4 * 512)
    ws = 1 << 24
    jobs = (_lib.SnJob * 1)(_job())
    for fwd in (True, False):
        def call(jobs, n, ws, nbytes):
            if fwd:
                return lib.ffc_sn_forward(jobs, n, 1, ws, nbytes, None)
            return lib.ffc_sn_backward(jobs, n, ws, nbytes, None)
        name = b"ffc_sn_forward" if fwd else b"ffc_sn_backward"
        assert call(jobs, 0, ws, need) == -1 and name in lib.ffc_last_error()
        assert call(jobs, -3, ws, need) == -1
        assert call(None, 1, ws, need) == -1 and b"table" in lib.ffc_last_error()
        assert call(jobs, 1, None, need) == -1 and b"workspace" in lib.ffc_last_error()
        assert call(jobs, 1, ws, need - 16) == -1 and b"workspace too small" in lib.ffc_last_error()
        assert call((_lib.SnJob * 1)(_job(ws_off=16)), 1, ws, need) == -1
        assert call((_lib.SnJob * 1)(_job(ws_off=8)), 1, ws, need + 64) == -1
        assert call((_lib.SnJob * 1)(_job(M=0)), 1, ws, need) == -1 and b"positive" in lib.ffc_last_error()
        assert call((_lib.SnJob * 1)(_job(K=-4)), 1, ws, need) == -1
        bad = _job()
        bad.u = None
        assert call((_lib.SnJob * 1)(bad), 1, ws, need) == -1 and b"null" in lib.ffc_last_error()
        bad = _job()
        bad.stride_m = 12   # neither of the two dense views
        assert call((_lib.SnJob * 1)(bad), 1, ws, need) == -1 and b"view" in lib.ffc_last_error()
        # the second job of a table is checked before the first is launched
        assert call((_lib.SnJob * 2)(_job(), _job(M=0, ws_off=need)), 2, ws, 2 * need) == -1
    bad = _job()
    bad.w = bad.w_orig
    assert lib.ffc_sn_forward((_lib.SnJob * 1)(bad), 1, 1, ws, need, None) == -1
