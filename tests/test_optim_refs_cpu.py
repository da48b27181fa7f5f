"""tests/optim_refs.py is what the GPU tests of the fused optimizer compare against: here it is checked against
torch.optim.AdamW / Adam and LambdaLR in float64, TOL is shown to be the smallest power of ten that leaves plain fp32
torch ROOM, and every planted defect is shown to break a bound.  The argument checks of ffc_optim_step /
ffc_optim_tick that return before any launch run here too: they need no device."""
import ctypes

import numpy as np
import pytest
import torch

import optim_refs as R

_REF = {}


def _ref(case):
    """the case's inputs and its float64 run, computed once"""
    if case["name"] not in _REF:
        inp = R.inputs(case)
        _REF[case["name"]] = (inp, R.run(case, *inp))
    return _REF[case["name"]]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["name"])
def test_restatement_matches_torch_float64(case):
    inp, ref = _ref(case)
    got = R.torch_run(case, *inp, torch.float64)
    for k, a, b in zip("pmv", got, ref[:3]):
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b), (case["name"], k)


def test_case_table_covers_the_settings_of_the_issue():
    assert any(c["betas"] == (0.0, 0.9) for c in R.CASES)
    for mode in (R.ADAMW, R.ADAM):
        assert {c["wd"] for c in R.CASES if c["mode"] == mode} >= {0.0, 0.01}
    assert sum(c["steps"] == 5 for c in R.CASES) >= 5 and any(c["t0"] == 99999 for c in R.CASES)


@pytest.mark.parametrize("T", [4, 1000])
def test_schedule_matches_lambda_lr(T):
    lr0 = 2e-4
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([w], lr=lr0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1 - s / T)
    want = {0, 1, T - 1, T}
    for s in range(T + 1):
        if s in want:
            assert sched.get_last_lr()[0] == R.lr_eff(lr0, s, T), s
        opt.step()
        sched.step()
    assert R.lr_eff(lr0, T, T) == 0.0 and R.lr_eff(lr0, T + 3, T) == 0.0 and R.lr_eff(lr0, 7, 0) == lr0


def test_fp32_torch_leaves_room_and_tol_is_the_smallest_power_of_ten():
    worst, where = 0.0, None
    for case in R.CASES:
        inp, ref = _ref(case)
        sh = R.shares(R.torch_run(case, *inp, torch.float32), ref)
        print(f"OBS fp32 torch, {case['name']}: " + " ".join(f"{k} {v:.3f}" for k, v in sh.items()))
        for k, v in sh.items():
            if v > worst:
                worst, where = v, (case["name"], k)
    print(f"OBS worst share {worst:.3f} at {where}")
    assert worst <= R.ROOM, (worst, where)
    assert worst * 10 > R.ROOM, f"TOL / 10 would leave room as well: {worst * 10:.3f}"


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_exceeds_a_bound(defect):
    worst = 0.0
    for case in R.CASES:
        inp, ref = _ref(case)
        worst = max(worst, max(R.shares(R.run(case, *inp, defect=defect)[:3], ref).values()))
    print(f"OBS {defect}: {worst:.3g} of the bound")
    assert worst > 1.0, (defect, worst)


# ---------------------------------------------------------------------------- rejections that need no device
def _lib():
    from fastfourierconvolution_amd import _lib
    return _lib.load()


def _step(L, **over):
    n = 2
    host = [(ctypes.c_float * 8)() for _ in range(4 * n)]   # never dereferenced: every call below is refused
    arr = [(ctypes.c_void_p * n)(*[ctypes.addressof(host[4 * i + k]) for i in range(n)]) for k in range(4)]
    state = (ctypes.c_longlong * 4)()
    a = dict(p=arr[0], g=arr[1], m=arr[2], v=arr[3], numel=(ctypes.c_longlong * n)(8, 8), n=n,
             state=ctypes.addressof(state), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, T=0, mode=0, per=0)
    a.update(over)
    status = L.ffc_optim_step(a["p"], a["g"], a["m"], a["v"], a["numel"], a["n"], a["state"], a["lr"], a["beta1"],
                              a["beta2"], a["eps"], a["wd"], a["T"], a["mode"], a["per"], None)
    return status, L.ffc_last_error().decode(), host


def test_argument_rejections_without_a_device():
    L = _lib()
    assert L.ffc_optim_state_bytes() == 32 and L.ffc_optim_max_jobs() == 64 and L.ffc_optim_chunk() == 8192
    nan = float("nan")
    p1 = _step(L, n=-1)[2]
    same = (ctypes.c_void_p * 2)(ctypes.addressof(p1[0]), ctypes.addressof(p1[0]))
    bad = [("n >= 0", dict(n=-1)), ("null list", dict(p=None)), ("null list", dict(g=None)), ("null list", dict(m=None)),
           ("null list", dict(v=None)), ("null list", dict(numel=None)), ("state", dict(state=None)),
           ("state", dict(state=ctypes.addressof(p1[0]) + 4)),
           ("beta1 and beta2", dict(beta1=1.0)), ("beta1 and beta2", dict(beta1=-0.1)), ("beta1 and beta2", dict(beta2=1.0)),
           ("beta1 and beta2", dict(beta2=nan)), ("eps >= 0", dict(eps=-1e-8)), ("eps >= 0", dict(eps=nan)),
           ("lr >= 0", dict(lr=-1.0)), ("lr >= 0", dict(lr=float("inf"))), ("weight_decay >= 0", dict(wd=-0.01)),
           ("decay_steps >= 0", dict(T=-1)), ("bad mode", dict(mode=2)), ("bad mode", dict(mode=-1)),
           ("negative numel", dict(numel=(ctypes.c_longlong * 2)(8, -1))),
           ("null tensor pointer", dict(m=(ctypes.c_void_p * 2)(None, None))),
           ("must not alias", dict(p=same, m=same))]
    for word, over in bad:
        status, msg, host = _step(L, **over)
        assert status == -1 and "ffc_optim_step" in msg and word in msg, (over, status, msg)
        assert all(x == 0.0 for h in host for x in h), "a refused call wrote"
    for word, args in (("state", (None, 1)), ("n_states >= 1", (ctypes.addressof(p1[0]), 0)),
                       ("n_states >= 1", (ctypes.addressof(p1[0]), -2))):
        assert L.ffc_optim_tick(args[0], args[1], None) == -1
        msg = L.ffc_last_error().decode()
        assert "ffc_optim_tick" in msg and word in msg, msg


def test_constructor_rejections_without_a_device():
    from fastfourierconvolution_amd import FusedAdam, FusedAdamW
    import fastfourierconvolution_amd as F
    assert "FusedAdamW" in F.__all__ and "FusedAdam" in F.__all__
    assert issubclass(FusedAdamW, torch.optim.AdamW) and issubclass(FusedAdam, torch.optim.Adam)
    w = torch.nn.Parameter(torch.zeros(3))
    for cls in (FusedAdamW, FusedAdam):
        with pytest.raises(NotImplementedError, match="GPU only"):
            cls([w])
        with pytest.raises(NotImplementedError, match="amsgrad"):
            cls([w], amsgrad=True)
        with pytest.raises(NotImplementedError, match="maximize"):
            cls([w], maximize=True)
        with pytest.raises(ValueError, match="decay_steps"):
            cls([w], decay_steps=0)
