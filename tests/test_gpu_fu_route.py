"""The C entry points a Fourier-unit call launches, row by row of tests/fu_route_cases.py: the ordered calls
through rt.lib() of the third call (two warm-up calls first; host-side queries left out), each with its
null optional pointers and its pass / kgroups integers, equal a literal list; the list equals what the
row's expected rt.FuRoute stands for (fu_route_cases.implied); and the route the call asked rt.fu_route for
is the expected one.

The lists in fu_route_cases.SEQUENCES came from the parent of the commit that introduced rt.fu_route: they
were recorded there with collect() of this file, which touches only rt.lib, FourierUnitSN._run and
SpectralTransform.spectral and so runs on that commit as it stands (the router import and the route
cross-check are guarded).  A kernel re-routed, a launch reordered, added or dropped, a fold moved to
another kernel or a BN finalized elsewhere shows up as a changed list.

A refusal row raises before anything is launched; nothing here makes a kernel fail.
"""
import contextlib
import io

import pytest
import torch

import fastfourierconvolution_amd as F
from fastfourierconvolution_amd import _runtime as rt
from fu_route_cases import BY_ID, QUERY_SUFFIXES, SEQUENCES, implied, note

HAS_ROUTER = hasattr(rt, "fu_route")


class Recorder:
    """stands in for rt.lib(): every entry point called through it is noted (fu_route_cases.note), then run"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name.endswith(QUERY_SUFFIXES):
            return fn

        def call(*args):
            self.calls.append(note(name, args))
            return fn(*args)
        return call


def build(row, device):
    """-> (call, module) of a row; call() runs it once"""
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        if row.kind == "fu":
            mod = F.FourierUnitSN(row.C, row.C)
        else:
            mod = F.SpectralTransform(16, 2 * row.C, 2 if (row.pool or row.up == 2) else 1, 1, row.lfu, row.up == 2)
    mod = mod.to(device).train(row.train)
    if row.kind == "fu":
        mod.mix_precision = row.mix
        t = torch.randn(row.B, row.C, row.H // row.up, row.H // row.up, device=device)
        return (lambda: mod._run(t, up=row.up)), mod
    mod.run_lfu = row.lfu
    if row.momentum_none:
        mod.bn1.momentum = None
    h = row.H * 2 if row.pool else row.H // row.up
    x = torch.randn(row.B, 16, h, h, device=device)
    return (lambda: mod.spectral(x)), mod


def collect(row, monkeypatch, routes=None):
    """-> the noted calls of the row's third call; routes: receives what rt.fu_route answered during it"""
    for k, v in row.sw.items():
        monkeypatch.setattr(rt, k, v)
    call, _ = build(row, "cuda")
    with torch.no_grad():
        call()
        call()
        rec = Recorder(rt.lib())
        monkeypatch.setattr(rt, "lib", lambda: rec)
        if routes is not None:
            inner = rt.fu_route
            monkeypatch.setattr(rt, "fu_route", lambda *a, **k: routes.append((inner(*a, **k), a)) or routes[-1][0])
        call()
    torch.cuda.synchronize()
    return rec.calls


@pytest.mark.gpu
@pytest.mark.parametrize("rid", [r.id for r in BY_ID.values() if r.raises is None])
def test_launches_are_the_recorded_ones(rid, monkeypatch):
    row = BY_ID[rid]
    routes = [] if HAS_ROUTER else None
    got = collect(row, monkeypatch, routes)
    print(got)
    assert got == SEQUENCES[rid]
    own = [c for c in got if c.startswith(("ffc_fu_forward", "ffc_fu2d_"))]
    if row.lfu:   # the local Fourier unit's launches come first (a fused unit on the quadrant stack)
        n = 2 if row.train else 1
        assert all(c.startswith("ffc_fu_forward_ex4") for c in own[:n])
        own = own[n:]
    assert own == implied(row.route, row.kind == "st", row.mix == "fp16")
    if row.kind == "st":
        names = [c.split("[")[0] for c in got]
        assert ("ffc_st_prologue_ex3" in names) == (row.conv1 == "prologue")
        assert ("ffc_pw_gate_conv" in names) == (row.conv1 == "pw_gate")
    if HAS_ROUTER:
        route, args = routes[0]   # the main unit's (a local Fourier unit asks after it)
        assert route._asdict() == row.route
        if row.kind == "st":
            assert args[-1].nrows == row.nrows


@pytest.mark.parametrize("rid", [r.id for r in BY_ID.values() if r.raises is not None])
def test_refusals_launch_nothing(rid, monkeypatch):
    """a plane or precision no path runs: the NotImplementedError, before any launch (runs without a device:
    the tensor is never touched)"""
    row = BY_ID[rid]
    call, _ = build(row, "cuda" if torch.cuda.is_available() else "cpu")
    rec = Recorder(rt.lib())
    monkeypatch.setattr(rt, "lib", lambda: rec)
    with pytest.raises(NotImplementedError) as e:
        call()
    assert str(e.value).startswith(row.raises)
    assert rec.calls == []
